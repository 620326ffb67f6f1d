"""Environment-map relighting of a trained neural scene for every camera of a camera JSON (iron_amd.neural_relight):

    python -m iron_amd.relight --ckpt CKPT.pth --cam_dict cam_dict_norm.json --envmap FILE --out DIR
                               [--n-light N] [--n-brdf N] [--seed S] [--samples-per-axis A] [--background] [--shadow-eps E]
                               [--max-depth D] [--n-paths P]

CKPT.pth is a stage-2 checkpoint: a dictionary of state-dicts under the keys sdf_network, diffuse_albedo_network,
specular_albedo_network and specular_roughness_network (render_surface.py:669-671; point_light_network and anything else in it is
ignored), loaded into the `ggx` networks of iron_amd.network_conf.  FILE is a lat-long environment map (.npy, Radiance .hdr, or .exr
when imageio reads it).  For every entry NAME of the camera JSON ({"K": 16 floats, "W2C": 16 floats, "img_size": [W, H]}) it writes
what `python -m iron_amd.render_asset --envmap` writes, through the same writers: OUT/image/STEM.exr (a float32 STEM.npy when
imageio has no EXR plugin) and the 8-bit OUT/image/STEM.png = clip(x^(1/2.2)).  --max-depth D > 1 adds the interreflections by
P paths per ray of at most D surface vertices.
"""
from __future__ import annotations

import argparse
import json
import os

import torch

from .envmap import EnvMap, read_envmap
from .export_materials import _exr_writer, _write_exr, _write_png
from .network_conf import init_rendering_network_dict, init_sdf_network_dict
from .neural_relight import relight_camera
from .raytracer import Camera, RayTracer
from .render_asset import _order, to8b_gamma

MATERIAL_KEYS = ("diffuse_albedo_network", "specular_albedo_network", "specular_roughness_network")


def load_networks(ckpt_path, device):
    """-> (sdf_network, color_network_dict) with the checkpoint's parameters, on `device`."""
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    missing = [k for k in ("sdf_network",) + MATERIAL_KEYS if k not in ckpt]
    if missing:
        raise SystemExit("%s: not a stage-2 checkpoint, it lacks %s" % (ckpt_path, ", ".join(missing)))
    sdf_network = init_sdf_network_dict(device)
    nets = init_rendering_network_dict("ggx", device)
    sdf_network.load_state_dict(ckpt["sdf_network"])
    for k in MATERIAL_KEYS:
        nets[k].load_state_dict(ckpt[k])
    return sdf_network, nets


def relight_cam_dict(sdf_network, nets, cam_dict, envmap, out_dir, samples_per_axis=1, **kw):
    """-> {image name: float32 [H, W, 3] numpy colour}, written as described in the module docstring; kw: relight_camera's."""
    os.makedirs(os.path.join(out_dir, "image"), exist_ok=True)
    dev = envmap.device
    raytracer = RayTracer()
    writer, note, images = _exr_writer(), [], {}
    for name in sorted(cam_dict.keys(), key=_order):
        entry = cam_dict[name]
        K = torch.tensor(entry["K"], dtype=torch.float32).reshape(4, 4).to(dev)
        W2C = torch.tensor(entry["W2C"], dtype=torch.float32).reshape(4, 4).to(dev)
        W, H = (int(x) for x in entry["img_size"])
        res = relight_camera(Camera(W, H, K, W2C), sdf_network, raytracer, nets, envmap, samples_per_axis=samples_per_axis, **kw)
        img = res["color"].cpu().numpy()
        stem = os.path.splitext(name)[0]
        _write_exr(os.path.join(out_dir, "image", stem + ".exr"), img, writer, note)
        _write_png(os.path.join(out_dir, "image", stem + ".png"), to8b_gamma(img))
        images[name] = img
    return images


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt", required=True, help="stage-2 checkpoint (.pth)")
    ap.add_argument("--cam_dict", required=True)
    ap.add_argument("--envmap", required=True, help="lat-long environment map (.npy, .hdr, .exr)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--n-light", type=int, default=64, dest="n_light")
    ap.add_argument("--n-brdf", type=int, default=64, dest="n_brdf")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--samples-per-axis", type=int, default=1, dest="samples_per_axis")
    ap.add_argument("--background", action="store_true", help="show the map where a ray misses the scene")
    ap.add_argument("--shadow-eps", type=float, default=1e-3, dest="shadow_eps", help="offset of a shadow ray's origin along the normal")
    ap.add_argument("--max-depth", type=int, default=1, dest="max_depth",
                    help="largest number of surface vertices on a light path, the primary hit included (1: direct light only)")
    ap.add_argument("--n-paths", type=int, default=64, dest="n_paths", help="paths per ray for the interreflections (--max-depth > 1)")
    a = ap.parse_args(argv)
    if not 1 <= a.max_depth <= 8 or not 1 <= a.n_paths <= 1 << 16:
        ap.error("--max-depth must be in 1 .. 8 and --n-paths in 1 .. 65536")
    if a.n_light < 0 or a.n_brdf < 0 or a.n_light + a.n_brdf == 0:
        ap.error("--n-light and --n-brdf must be >= 0 and not both 0")
    if a.samples_per_axis < 1 or not a.shadow_eps >= 0:
        ap.error("--samples-per-axis must be >= 1 and --shadow-eps >= 0")
    return a


def main(argv=None) -> None:
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("iron_amd.relight needs a GPU (iron_amd has no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    with open(a.cam_dict) as fp:
        cam_dict = json.load(fp)
    sdf_network, nets = load_networks(a.ckpt, dev)
    envmap = EnvMap(read_envmap(a.envmap), device=dev)
    images = relight_cam_dict(sdf_network, nets, cam_dict, envmap, a.out, samples_per_axis=a.samples_per_axis, n_light=a.n_light,
                              n_brdf=a.n_brdf, seed=a.seed, background=a.background, shadow_eps=a.shadow_eps, max_depth=a.max_depth,
                              n_paths=a.n_paths)
    print("relit %d views into %s" % (len(images), os.path.join(a.out, "image")))


if __name__ == "__main__":
    main()
