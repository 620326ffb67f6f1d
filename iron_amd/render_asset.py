"""Flash renders of an exported asset for every camera of a camera JSON: the loop of the reference's
render_synthetic_data/render_rgb_flash_mat.py (Mitsuba's roughplastic with diffuseReflectance / specularReflectance / alpha bitmaps
on model.obj, a point light at the camera origin), on the HIP kernels of iron_amd.mesh_render.

    python -m iron_amd.render_asset --mesh M.obj --textures DIR --cam_dict cam_dict_norm.json --out DIR [--light 20] [--spp-axis S]
                                    [--envmap FILE [--n-light N] [--n-brdf N] [--seed S] [--background] [--max-depth D] [--n-paths P]]

For every entry NAME of the camera JSON ({"K": 16 floats, "W2C": 16 floats, "img_size": [W, H]}) it writes OUT/image/STEM.exr (a
float32 STEM.npy when imageio has no EXR plugin, like export_materials) and the 8-bit OUT/image/STEM.png, plus OUT/light.txt.

With --envmap FILE (.npy, Radiance .hdr, or .exr when imageio reads it) the same loop is the reference's
test_mitsuba/render_rgb_envmap_mat.py instead: the asset under that lat-long environment map (mesh_render.render_asset_env; direct
illumination with visibility, --n-light environment samples and --n-brdf BRDF samples per ray; with --max-depth D > 1 also the
interreflections, by --n-paths paths per ray of at most D surface vertices, the primary hit included).  The files are the same, the
.png being the reference script's clip(x^(1/2.2)); light.txt is not written.

Deviations from the reference's renders, on purpose: the flash render and the default environment render (--max-depth 1) are direct
illumination only, and the interreflections of --max-depth D stop at a fixed depth where Mitsuba's path integrator plays Russian
roulette; a box pixel filter over the --spp-axis^2 regular samples of a pixel, not Mitsuba's Gaussian.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from .export_materials import _exr_writer, _write_exr, _write_png, to8b
from .envmap import EnvMap, read_envmap
from .mesh_render import MeshAsset, render_asset_camera, render_asset_env
from .raytracer import Camera


def _order(name):
    stem = os.path.splitext(name)[0]
    return (0, int(stem), name) if stem.isdigit() else (1, 0, name)


def render_cam_dict(asset, cam_dict, out_dir, light=20.0, samples_per_axis=1, envmap=None, env_args=None):
    """-> {image name: float32 [H, W, 3] numpy colour}, written as described in the module docstring.  envmap (EnvMap): the
    environment render with the keywords env_args of render_asset_env, in place of the flash."""
    os.makedirs(os.path.join(out_dir, "image"), exist_ok=True)
    if envmap is None:
        with open(os.path.join(out_dir, "light.txt"), "w") as fp:
            fp.write("%s\n" % float(light))
    writer, note, images = _exr_writer(), [], {}
    for name in sorted(cam_dict.keys(), key=_order):
        entry = cam_dict[name]
        K = torch.tensor(entry["K"], dtype=torch.float32).reshape(4, 4).to(asset.device)
        W2C = torch.tensor(entry["W2C"], dtype=torch.float32).reshape(4, 4).to(asset.device)
        W, H = (int(x) for x in entry["img_size"])
        if envmap is None:
            res = render_asset_camera(Camera(W, H, K, W2C), asset, light, samples_per_axis=samples_per_axis)
        else:
            res = render_asset_env(Camera(W, H, K, W2C), asset, envmap, samples_per_axis=samples_per_axis, **(env_args or {}))
        img = res["color"].cpu().numpy()
        stem = os.path.splitext(name)[0]
        _write_exr(os.path.join(out_dir, "image", stem + ".exr"), img, writer, note)
        _write_png(os.path.join(out_dir, "image", stem + ".png"), to8b(img) if envmap is None else to8b_gamma(img))
        images[name] = img
    return images


def to8b_gamma(img):
    """The reference envmap script's 8-bit image: clip(x^(1/2.2), 0, 1) * 255."""
    return (np.clip(np.power(np.maximum(img, 0.0), 1.0 / 2.2), 0.0, 1.0) * 255.0).astype(np.uint8)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True)
    ap.add_argument("--textures", required=True)
    ap.add_argument("--cam_dict", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--light", type=float, default=20.0)
    ap.add_argument("--spp-axis", type=int, default=1, dest="spp_axis")
    ap.add_argument("--normals", choices=("vertex", "face"), default="vertex")
    ap.add_argument("--envmap", default=None, help="lat-long environment map (.npy, .hdr, .exr): relight under it instead of the flash")
    ap.add_argument("--n-light", type=int, default=64, dest="n_light")
    ap.add_argument("--n-brdf", type=int, default=64, dest="n_brdf")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--background", action="store_true", help="show the map where a ray misses the asset")
    ap.add_argument("--max-depth", type=int, default=1, dest="max_depth",
                    help="largest number of surface vertices on a light path, the primary hit included (1 .. 8; 1: direct light only)")
    ap.add_argument("--n-paths", type=int, default=64, dest="n_paths", help="paths per ray for --max-depth > 1 (1 .. 65536)")
    a = ap.parse_args(argv)
    if a.envmap is None and (a.background or a.seed != 0 or a.n_light != 64 or a.n_brdf != 64 or a.max_depth != 1 or a.n_paths != 64):
        ap.error("--n-light, --n-brdf, --seed, --background, --max-depth and --n-paths need --envmap")
    if not 1 <= a.max_depth <= 8 or not 1 <= a.n_paths <= 1 << 16:
        ap.error("--max-depth must lie in 1 .. 8 and --n-paths in 1 .. 65536")
    if a.n_light < 0 or a.n_brdf < 0 or a.n_light + a.n_brdf == 0:
        ap.error("--n-light and --n-brdf must be >= 0 and not both 0")
    return a


def main(argv=None) -> None:
    a = parse_args(argv)
    with open(a.cam_dict) as fp:
        cam_dict = json.load(fp)
    asset = MeshAsset.load(a.mesh, a.textures, normals=a.normals)
    envmap = None if a.envmap is None else EnvMap(read_envmap(a.envmap), device=asset.device)
    images = render_cam_dict(asset, cam_dict, a.out, light=a.light, samples_per_axis=a.spp_axis, envmap=envmap,
                             env_args={"n_light": a.n_light, "n_brdf": a.n_brdf, "seed": a.seed, "background": a.background,
                                       "max_depth": a.max_depth, "n_paths": a.n_paths})
    print("rendered %d views into %s" % (len(images), os.path.join(a.out, "image")))


if __name__ == "__main__":
    main()
