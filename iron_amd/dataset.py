"""The stage-2 dataset loader (models/dataset.py:1407-1456) without imageio or OpenCV: `load_datadir` and `to8b`; and the stage-1
dataset (models/dataset.py:95-373) with its batches made on the device: `VolumeDataset` (at the end of the file).

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


class VolumeDataset:
    """The stage-1 dataset (models/dataset.py:95-373, the `Dataset` class the committed confs describe) with its batches made on
    the device (csrc/volume.hip).

    Built from a data directory -- VolumeDataset(conf["dataset"]) or VolumeDataset(data_dir=..., folder_name=...), read through
    load_datadir -- or from tensors: images [N, H, W, C >= 3] (uint8, or float in 0 .. 1), Ks and W2Cs [N, 4, 4], optional masks
    [N, H, W] or [N, H, W, Cm].  The pictures stay on the device as uint8: v / 255.0f in fp32 equals the reference's
    (v / 255.0).astype(float32) for all 256 values.  Masks are read from DIR/mask/NAME.png when mask_weight > 0 and that folder
    exists; without masks the mask is 1 everywhere, as in the reference (no_mask = True).

    intrinsics_all_inv = torch.inverse(K) and pose_all = inverse(W2C) per view are formed in fp32 as the reference forms them
    (the pose: numpy's inverse of the float64 W2C, rounded to float32).  gen_rays_between, the video output and the NIR / RGB
    dual data sets are not built."""

    def __init__(self, conf=None, data_dir=None, folder_name=None, images=None, Ks=None, W2Cs=None, masks=None, mask_weight=0.0,
                 device=None):
        if not torch.cuda.is_available():
            raise _lib.IronError("VolumeDataset needs a GPU (iron_amd has no CPU path)")
        self.device = dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if conf is not None:
            data_dir = conf["data_dir"] if data_dir is None else data_dir
            folder_name = (conf["folder_name"] if "folder_name" in conf else "image") if folder_name is None else folder_name
        folder_name = "image" if folder_name is None else folder_name
        self.data_dir, self.folder_name = data_dir, folder_name
        if images is None:
            if data_dir is None:
                raise _lib.IronError("VolumeDataset: give a data directory or images, Ks, W2Cs")
            self.images_lis, images, Ks, W2Cs = load_datadir(data_dir, folder_name)
            if masks is None and mask_weight > 0 and os.path.isdir(os.path.join(data_dir, "mask")):
                masks = torch.stack([torch.from_numpy(np.ascontiguousarray(read_image(os.path.join(
                    data_dir, "mask", os.path.splitext(os.path.basename(p))[0] + ".png")))) for p in self.images_lis], dim=0)
        else:
            if Ks is None or W2Cs is None or len(Ks) != len(images) or len(W2Cs) != len(images):
                raise _lib.IronError("VolumeDataset: images, Ks and W2Cs must have one entry per view")
            self.images_lis = ["view_%d" % i for i in range(len(images))]

        def to_u8(t, name, min_c):
            t = torch.as_tensor(t)
            if t.dim() == 3:
                t = t.unsqueeze(-1)
            if t.dim() != 4 or t.shape[-1] < min_c:
                raise _lib.IronError("VolumeDataset: %s must be [N, H, W, C >= %d], got %s" % (name, min_c, tuple(t.shape)))
            if t.dtype != torch.uint8:
                t = (t.to(dev, torch.float32) * 255.0).round().clamp(0.0, 255.0).to(torch.uint8)
            return t.to(dev).contiguous()
        self.images_u8 = to_u8(images, "images", 3)
        self.n_images, self.H, self.W = (int(x) for x in self.images_u8.shape[:3])
        self.image_pixels = self.H * self.W
        self.masks_u8 = None
        if masks is not None:
            self.masks_u8 = to_u8(masks, "masks", 1)
            if tuple(self.masks_u8.shape[:3]) != (self.n_images, self.H, self.W):
                raise _lib.IronError("VolumeDataset: masks must be [%d, %d, %d(, Cm)], got %s"
                                     % (self.n_images, self.H, self.W, tuple(self.masks_u8.shape)))
        Ks = torch.as_tensor(np.asarray(Ks) if not torch.is_tensor(Ks) else Ks).detach().cpu()
        W2Cs = torch.as_tensor(np.asarray(W2Cs) if not torch.is_tensor(W2Cs) else W2Cs).detach().cpu()
        if tuple(Ks.shape) != (self.n_images, 4, 4) or tuple(W2Cs.shape) != (self.n_images, 4, 4):
            raise _lib.IronError("VolumeDataset: Ks and W2Cs must be [%d, 4, 4]" % self.n_images)
        self.intrinsics_all = Ks.to(torch.float32).to(dev)                                              # :219, 228
        self.intrinsics_all_inv = torch.inverse(self.intrinsics_all).contiguous()                        # :229
        self.pose_all = torch.from_numpy(np.linalg.inv(W2Cs.numpy().astype(np.float64)).astype(np.float32)).to(dev).contiguous()  # :218
        self.world_mats_np = [m for m in W2Cs.numpy().astype(np.float32)]
        self.scale_mats_np = [np.eye(4, dtype=np.float32) for _ in range(self.n_images)]
        self.focal = self.intrinsics_all[0][0, 0]
        self.object_bbox_min = np.array([-1.01, -1.01, -1.01])                                           # :235-242
        self.object_bbox_max = np.array([1.01, 1.01, 1.01])

    def _view(self, img_idx) -> int:
        i = int(img_idx)
        if not 0 <= i < self.n_images:
            raise _lib.IronError("VolumeDataset: view %d of %d" % (i, self.n_images))
        return i

    def rays_at_pixels(self, img_idx, pixels_x, pixels_y):
        """The batch of the given pixels (device int64 columns and rows [B]) -> (data [B, 10], near [B, 1], far [B, 1])."""
        i = self._view(img_idx)
        dev = self.device
        px = pixels_x.to(dev, torch.int64).contiguous().reshape(-1)
        py = pixels_y.to(dev, torch.int64).contiguous().reshape(-1)
        if px.shape != py.shape:
            raise _lib.IronError("VolumeDataset: pixels_x and pixels_y must have one length")
        n = px.shape[0]
        data = torch.empty((n, 10), dtype=torch.float32, device=dev)
        near, far = torch.empty((n, 1), dtype=torch.float32, device=dev), torch.empty((n, 1), dtype=torch.float32, device=dev)
        mask = None if self.masks_u8 is None else self.masks_u8[i]
        with torch.cuda.device(dev):
            _lib.check(_lib.load().iron_volume_rays(self.images_u8[i].data_ptr(), self.H, self.W, self.images_u8.shape[-1], _lib.ptr(mask),
                                                    0 if mask is None else mask.shape[-1], self.intrinsics_all_inv[i].data_ptr(),
                                                    self.pose_all[i].data_ptr(), px.data_ptr(), py.data_ptr(), n, data.data_ptr(),
                                                    near.data_ptr(), far.data_ptr(), _lib.stream_ptr(dev)))
        return data, near, far

    def gen_random_rays_with_bounds(self, img_idx, batch_size, generator=None):
        """gen_random_rays_at and near_far_from_sphere of its rays from one launch -> (data [B, 10], near [B, 1], far [B, 1])."""
        pixels_x = torch.randint(low=0, high=self.W, size=[batch_size], device=self.device, generator=generator)   # :290-291
        pixels_y = torch.randint(low=0, high=self.H, size=[batch_size], device=self.device, generator=generator)
        return self.rays_at_pixels(img_idx, pixels_x, pixels_y)

    def gen_random_rays_at(self, img_idx, batch_size, generator=None):
        """models/dataset.py:286-300: random rays in world space from one camera -> [batch_size, 10] = rays_o, rays_d, colour, mask.
        The pixels come from torch.randint on the device (`generator`: a device generator, None = the device's default one); no
        picture is indexed on the host, nothing is copied to the device and nothing waits for it."""
        return self.gen_random_rays_with_bounds(img_idx, batch_size, generator)[0]

    def gen_rays_at(self, img_idx, resolution_level=1):
        """models/dataset.py:271-284 -> rays_o, rays_d [H // l, W // l, 3].  The two coordinate rows are torch.linspace's, made on
        the device and handed to the kernel (the symmetric formula is torch's own, not restated)."""
        i = self._view(img_idx)
        l = int(resolution_level)
        dev = self.device
        cols, rows = self.W // l, self.H // l
        tx = torch.linspace(0, self.W - 1, cols, device=dev)
        ty = torch.linspace(0, self.H - 1, rows, device=dev)
        rays_o = torch.empty((rows, cols, 3), dtype=torch.float32, device=dev)
        rays_d = torch.empty((rows, cols, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().iron_volume_rays_grid(self.intrinsics_all_inv[i].data_ptr(), self.pose_all[i].data_ptr(), tx.data_ptr(),
                                                         ty.data_ptr(), rows, cols, rays_o.data_ptr(), rays_d.data_ptr(),
                                                         _lib.stream_ptr(dev)))
        return rays_o, rays_d

    def near_far_from_sphere(self, rays_o, rays_d, *_ignored):
        """models/dataset.py:335-361: mid -+ 1 with mid = 0.5 (-b) / a."""
        a = torch.sum(rays_d ** 2, dim=-1, keepdim=True)
        b = 2.0 * torch.sum(rays_o * rays_d, dim=-1, keepdim=True)
        mid = 0.5 * (-b) / a
        return mid - 1.0, mid + 1.0

    def image_at(self, idx, resolution_level):
        """uint8 [H // l, W // l, 3], resized through PIL: a picture for the eye (not bit-equal to the reference's cv2.resize)."""
        from PIL import Image
        i = self._view(idx)
        l = int(resolution_level)
        img = self.images_u8[i, :, :, :3].cpu().numpy()
        if l == 1:
            return img
        return np.asarray(Image.fromarray(img).resize((self.W // l, self.H // l), Image.BILINEAR))
