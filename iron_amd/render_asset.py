"""Flash renders of an exported asset for every camera of a camera JSON: the loop of the reference's
render_synthetic_data/render_rgb_flash_mat.py (Mitsuba's roughplastic with diffuseReflectance / specularReflectance / alpha bitmaps
on model.obj, a point light at the camera origin), on the HIP kernels of iron_amd.mesh_render.

    python -m iron_amd.render_asset --mesh M.obj --textures DIR --cam_dict cam_dict_norm.json --out DIR [--light 20] [--spp-axis S]

For every entry NAME of the camera JSON ({"K": 16 floats, "W2C": 16 floats, "img_size": [W, H]}) it writes OUT/image/STEM.exr (a
float32 STEM.npy when imageio has no EXR plugin, like export_materials) and the 8-bit OUT/image/STEM.png, plus OUT/light.txt.

Two deviations from the reference's renders, on purpose: direct illumination only (Mitsuba's path integrator adds the
interreflections), and a box pixel filter over the --spp-axis^2 regular samples of a pixel, not Mitsuba's Gaussian.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from .export_materials import _exr_writer, _write_exr, _write_png, to8b
from .mesh_render import MeshAsset, render_asset_camera
from .raytracer import Camera


def _order(name):
    stem = os.path.splitext(name)[0]
    return (0, int(stem), name) if stem.isdigit() else (1, 0, name)


def render_cam_dict(asset, cam_dict, out_dir, light=20.0, samples_per_axis=1):
    """-> {image name: float32 [H, W, 3] numpy colour}, written as described in the module docstring."""
    os.makedirs(os.path.join(out_dir, "image"), exist_ok=True)
    with open(os.path.join(out_dir, "light.txt"), "w") as fp:
        fp.write("%s\n" % float(light))
    writer, note, images = _exr_writer(), [], {}
    for name in sorted(cam_dict.keys(), key=_order):
        entry = cam_dict[name]
        K = torch.tensor(entry["K"], dtype=torch.float32).reshape(4, 4).to(asset.device)
        W2C = torch.tensor(entry["W2C"], dtype=torch.float32).reshape(4, 4).to(asset.device)
        W, H = (int(x) for x in entry["img_size"])
        res = render_asset_camera(Camera(W, H, K, W2C), asset, light, samples_per_axis=samples_per_axis)
        img = res["color"].cpu().numpy()
        stem = os.path.splitext(name)[0]
        _write_exr(os.path.join(out_dir, "image", stem + ".exr"), img, writer, note)
        _write_png(os.path.join(out_dir, "image", stem + ".png"), to8b(img))
        images[name] = img
    return images


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True)
    ap.add_argument("--textures", required=True)
    ap.add_argument("--cam_dict", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--light", type=float, default=20.0)
    ap.add_argument("--spp-axis", type=int, default=1, dest="spp_axis")
    ap.add_argument("--normals", choices=("vertex", "face"), default="vertex")
    a = ap.parse_args(argv)
    with open(a.cam_dict) as fp:
        cam_dict = json.load(fp)
    asset = MeshAsset.load(a.mesh, a.textures, normals=a.normals)
    images = render_cam_dict(asset, cam_dict, a.out, light=a.light, samples_per_axis=a.spp_axis)
    print("rendered %d views into %s" % (len(images), os.path.join(a.out, "image")))


if __name__ == "__main__":
    main()
