"""The stage-2 dataset loader (models/dataset.py:1407-1456) without imageio or OpenCV: `load_datadir` and `to8b`.

A data directory holds cam_dict_norm.json -- {image name: {"K": 16 floats, "W2C": 16 floats, ...}} -- and one picture per entry
under `folder_name`.  Names are ordered by the integer in front of their four-character extension when every name has one, by
the plain string otherwise, as the reference orders them.  For the stem of every name the first of STEM.png, STEM.jpg, STEM.exr
that exists is read: .png / .jpg through PIL as uint8 / 255, .exr through iron_amd.envmap's reader as clip(x^(1/2.2), 0, 1).

This module is not part of install_as_models(): `models.dataset` keeps resolving to the caller's own file.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _lib
from .export_materials import to8b  # noqa: F401  (the reference's models.dataset.to8b)


def ordered_names(names):
    """The reference's ordering of the camera dictionary's keys (models/dataset.py:1409-1413)."""
    names = list(names)
    try:
        return sorted(names, key=lambda x: int(x[:-4]))
    except ValueError:
        return sorted(names)


def read_image(fpath) -> np.ndarray:
    """-> float32 [H, W, C] (or [H, W]) in 0 .. 1: an 8-bit .png / .jpg divided by 255, an .exr gamma-corrected and clipped."""
    ext = os.path.splitext(fpath)[1].lower()
    if ext in (".png", ".jpg"):
        from PIL import Image
        with Image.open(fpath) as im:
            a = np.asarray(im)
        if a.dtype != np.uint8:
            raise _lib.IronError("%s: expected an 8-bit picture, got %s (mode %s)" % (fpath, a.dtype, im.mode))
        return a.astype(np.float32) / 255.0
    if ext == ".exr":
        from .envmap import read_envmap
        return np.clip(np.power(read_envmap(fpath), 1.0 / 2.2), 0, 1)
    raise _lib.IronError("%s: must use .png, .jpg or .exr images as inputs" % fpath)


def load_datadir(datadir, folder_name='image'):
    """-> (image_fpaths, gt_images float32 [N, H, W, C], Ks float32 [N, 4, 4], W2Cs float32 [N, 4, 4]), CPU tensors."""
    with open(os.path.join(datadir, "cam_dict_norm.json")) as fp:
        cam_dict = json.load(fp)
    image_fpaths, gt_images, Ks, W2Cs = [], [], [], []
    for x in ordered_names(cam_dict.keys()):
        filename = x.split('.')[0]
        for ext in (".png", ".jpg", ".exr"):
            fpath = os.path.join(datadir, folder_name, filename + ext)
            if os.path.exists(fpath):
                break
        else:
            raise _lib.IronError("%s: no %s.png, .jpg or .exr under %s" % (x, filename, os.path.join(datadir, folder_name)))
        image_fpaths.append(fpath)
        gt_images.append(torch.from_numpy(np.ascontiguousarray(read_image(fpath))))
        Ks.append(torch.from_numpy(np.array(cam_dict[x]["K"]).reshape((4, 4)).astype(np.float32)))
        W2Cs.append(torch.from_numpy(np.array(cam_dict[x]["W2C"]).reshape((4, 4)).astype(np.float32)))
    if not gt_images:
        raise _lib.IronError("%s: cam_dict_norm.json lists no image" % datadir)
    shapes = {tuple(im.shape) for im in gt_images}
    if len(shapes) != 1:
        raise _lib.IronError("%s: the images differ in shape (%s); they are stacked into one tensor" % (datadir, sorted(shapes)))
    return image_fpaths, torch.stack(gt_images, dim=0), torch.stack(Ks, dim=0), torch.stack(W2Cs, dim=0)
