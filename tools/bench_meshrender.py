"""Asset flash render on the GPU (csrc/meshrender.hip, iron_amd/mesh_render.py): times on scene S0's 512^3 extract_geometry mesh
at 800x800 from the fixture camera, by device events (median of --reps after a warm-up run): the BVH build, the ray cast under
both lane assignments (row-major, which mesh_render uses, and one 8x8 pixel tile per wave, built here: the kernel alone on rays
already in that order, and with the gathers that reorder the rays and restore the results), the vertex normals, the shading
kernel, and the whole render_asset_camera frame with 1 and 2x2 samples per pixel.  For scale, `render_camera_ms` is the neural frame (sphere tracing +
GGX shading of the networks, no silhouette pass) of the same camera.  The material texture is synthetic (2048^2 random values, all
texels marked baked): the timing does not depend on its contents.  Prints one JSON line.

    python tools/bench_meshrender.py [--reps 5] [--res 512] [--size 800]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def timed(fn, reps):
    fn()  # warm-up
    ms = []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn()
        e[1].record()
        torch.cuda.synchronize()
        ms.append(e[0].elapsed_time(e[1]))
    return round(med(ms), 4)


def tile_order(H, W, dev):
    """(perm, inverse) int64 [H * W]: lane j takes pixel perm[j], so that 64 consecutive lanes (one wave) cover one 8x8 pixel tile
    (partial tiles at the right and lower borders are packed densely)."""
    y = torch.arange(H, device=dev).unsqueeze(1).expand(H, W)
    x = torch.arange(W, device=dev).unsqueeze(0).expand(H, W)
    rank = ((y // 8) * ((W + 7) // 8) + x // 8) * 64 + (y % 8) * 8 + x % 8
    perm = torch.argsort(rank.reshape(-1), stable=True)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(H * W, device=dev)
    return perm, inv


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshrender needs a GPU")
    from iron_amd import mesh_render, scenes
    from iron_amd.mesh_distance import MeshBVH
    from iron_amd.mesh_render import MeshAsset, render_asset_camera, vertex_normals
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    from iron_amd.renderer import NeuSRenderer
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    from iron_amd.uv_unwrap import smart_uv_project

    dev = torch.device("cuda", 0)
    sys.modules["mcubes"] = None  # the device path of extract_geometry
    nets = {k: v.to(dev) for k, v in scenes.build_networks("S0").items()}
    r = NeuSRenderer(None, nets["sdf_network"], None, None, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=0.0)
    v, f = r.extract_geometry(torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]), resolution=a.res, threshold=0.0)
    v, f = torch.as_tensor(v, dtype=torch.float32).to(dev), torch.as_tensor(f).to(dev)
    uvs, fuv = smart_uv_project(v, f)
    mat = torch.rand((2048, 2048, 7), device=dev) * 0.9 + 0.05
    weight = torch.ones((2048, 2048), device=dev)
    res = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "faces": int(f.shape[0]), "verts": int(v.shape[0]),
           "image": [a.size, a.size]}

    res["bvh_build_ms"] = timed(lambda: MeshBVH(v, f), a.reps)
    res["vertex_normals_ms"] = timed(lambda: vertex_normals(v, f), a.reps)
    asset = MeshAsset(v, f, uvs, fuv, mat, weight=weight)
    K, W2C = scenes.fixture_camera_matrices(a.size, a.size)
    cam = Camera(a.size, a.size, K.to(dev), W2C.to(dev))
    ray_o, ray_d, _ = cam.get_rays(cam.get_uv())
    o, d = ray_o.reshape(-1, 3).contiguous(), ray_d.reshape(-1, 3).contiguous()
    n = o.shape[0]
    perm, inv = tile_order(a.size, a.size, dev)
    op, dp = o[perm].contiguous(), d[perm].contiguous()

    def tile_with_gathers():
        t, fi, b = asset.bvh.raycast(o[perm], d[perm])
        return t[inv], fi[inv], b[inv]

    cast = {"row_ms": timed(lambda: asset.bvh.raycast(o, d), a.reps), "tile_kernel_ms": timed(lambda: asset.bvh.raycast(op, dp), a.reps),
            "tile_with_gathers_ms": timed(tile_with_gathers, a.reps)}
    for k in list(cast):
        cast[k.replace("_ms", "_mrays_per_s")] = round(n / (cast[k] * 1e-3) / 1e6, 1)
    t, fi, b = asset.bvh.raycast(o, d)
    cast["hits"] = int((fi >= 0).sum())
    t2, f2, b2 = tile_with_gathers()
    cast["orders_agree_bitwise"] = bool(torch.equal(t, t2) and torch.equal(fi, f2) and torch.equal(b, b2))
    res["raycast"] = cast
    tables = mesh_render._mts_tables(dev)
    res["shade_ms"] = timed(lambda: asset.shade(o, d, t, fi, b, 20.0, tables), a.reps)
    res["frame_ms"] = timed(lambda: render_asset_camera(cam, asset, 20.0), a.reps)
    res["frame_2x2_ms"] = timed(lambda: render_asset_camera(cam, asset, 20.0, samples_per_axis=2), a.reps)
    fn = make_render_fn(GGXColocatedRenderer(use_cuda=True))
    tracer = RayTracer()
    res["render_camera_ms"] = timed(lambda: render_camera(cam, nets["sdf_network"], tracer, nets, fn, fill_holes=False, handle_edges=False,
                                                          is_training=False), a.reps)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
