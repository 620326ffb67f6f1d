"""Environment render on the GPU (csrc/envlight.hip, iron_amd/envmap.py, iron_amd/mesh_render.py): times on scene
S0's 512^3 extract_geometry mesh at 800x800 from the fixture camera, by device events (median of --reps after a warm-up run): the
distribution build of a 512 x 1024 map, `occluded` against `raycast` on the camera's primary rays (alternating in one run), the
integrator at 64 + 64 and 256 + 256 samples per pixel with its shadow rays per second (the shadow rays are counted from the
visibility dump of a separate, untimed run: a sample below the horizon casts none), the path integrator for interreflections
 at 64 paths per pixel and depth 2 and 4 with the rays it casts per second (bounce rays and shadow rays, counted from
its dumps likewise), and whole render_asset_env frames.  The map and the material texture are synthetic (a smooth sky with a small sun; random materials): the timing depends on them only through
where the samples go.  Writes one JSON line to profiles/envlight_bench.json and prints it.

    python tools/bench_envlight.py [--reps 5] [--res 512] [--size 800]
"""
from __future__ import annotations

import argparse
import json
import math
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


def sky(He, We, dev):
    """a smooth sky, brighter towards the zenith, with a sun of 2 x 4 texels at 5e3"""
    v = (torch.arange(He, device=dev, dtype=torch.float32) + 0.5) / He
    img = (0.2 + 0.8 * torch.cos(math.pi * v).clamp_min(0))[:, None, None].expand(He, We, 3).contiguous()
    img = img * torch.tensor([0.6, 0.8, 1.0], device=dev)
    img[He // 5:He // 5 + 2, We // 3:We // 3 + 4] = 5e3
    return img


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envlight_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_envlight needs a GPU")
    from iron_amd import mesh_render, scenes
    from iron_amd.envmap import EnvMap
    from iron_amd.mesh_render import MeshAsset, render_asset_env
    from iron_amd.raytracer import Camera
    from iron_amd.renderer import NeuSRenderer
    from iron_amd.uv_unwrap import smart_uv_project

    dev = torch.device("cuda", 0)
    sys.modules["mcubes"] = None  # the device path of extract_geometry
    nets = {k: v.to(dev) for k, v in scenes.build_networks("S0").items()}
    r = NeuSRenderer(None, nets["sdf_network"], None, None, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=0.0)
    v, f = r.extract_geometry(torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]), resolution=a.res, threshold=0.0)
    v, f = torch.as_tensor(v, dtype=torch.float32).to(dev), torch.as_tensor(f).to(dev)
    uvs, fuv = smart_uv_project(v, f)
    mat = torch.rand((2048, 2048, 7), device=dev) * 0.9 + 0.05
    asset = MeshAsset(v, f, uvs, fuv, mat, weight=torch.ones((2048, 2048), device=dev))
    res = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "faces": int(f.shape[0]), "verts": int(v.shape[0]),
           "image": [a.size, a.size], "envmap": [512, 1024]}

    img = sky(512, 1024, dev)
    res["distribution_build_ms"] = timed(lambda: EnvMap(img), a.reps)
    env = EnvMap(img)
    K, W2C = scenes.fixture_camera_matrices(a.size, a.size)
    cam = Camera(a.size, a.size, K.to(dev), W2C.to(dev))
    ray_o, ray_d, _ = cam.get_rays(cam.get_uv())
    o, d = ray_o.reshape(-1, 3).contiguous(), ray_d.reshape(-1, 3).contiguous()
    n = o.shape[0]

    # occluded against raycast on the primary rays, alternating in one run
    bvh = asset.bvh
    bvh.raycast(o, d), bvh.occluded(o, d)
    pairs = [(timed(lambda: bvh.raycast(o, d), 1), timed(lambda: bvh.occluded(o, d), 1)) for _ in range(a.reps)]
    t, fi, b = bvh.raycast(o, d)
    cast = {"raycast_ms": med([p[0] for p in pairs]), "occluded_ms": med([p[1] for p in pairs]), "hits": int((fi >= 0).sum()),
            "agree": bool(torch.equal(bvh.occluded(o, d).bool(), fi >= 0))}
    cast["raycast_mrays_per_s"] = round(n / (cast["raycast_ms"] * 1e-3) / 1e6, 1)
    cast["occluded_mrays_per_s"] = round(n / (cast["occluded_ms"] * 1e-3) / 1e6, 1)
    res["primary_rays"] = cast

    tables = mesh_render._mts_tables(dev)
    res["integrator"] = {}
    for nl, nb in ((64, 64), (256, 256)):
        ms = timed(lambda: asset.shade_env(o, d, t, fi, b, env, tables, n_light=nl, n_brdf=nb), a.reps)
        # the shadow rays of the frame, from the dumps of a strip of rows at a time (the whole frame's dump would not fit comfortably)
        rays, visible = 0, 0
        rows = max(1, (1 << 22) // ((nl + nb) * a.size))
        for y0 in range(0, a.size, rows):
            s = slice(y0 * a.size, min(y0 + rows, a.size) * a.size)
            out = asset.shade_env(o[s], d[s], t[s], fi[s], b[s], env, tables, n_light=nl, n_brdf=nb, dump=True,
                                  pixel_idx=torch.arange(s.start, s.stop, device=dev, dtype=torch.int32))
            w, nrm = out["dump_dir"], out["normal"]
            hit = fi[s] >= 0
            # a shadow ray is cast for a sample above the shading horizon on the viewer's side of the face; count the first condition,
            # which the dump allows (the second removes few more on a closed mesh seen from outside)
            rays += int((((w * nrm[:, None, :]).sum(-1) > 0) & hit[:, None]).sum())
            visible += int(out["dump_vis"].sum())
        res["integrator"]["%d+%d" % (nl, nb)] = {"ms": ms, "samples": int((fi >= 0).sum()) * (nl + nb), "shadow_rays": rays,
                                                "visible": visible, "shadow_mrays_per_s": round(rays / (ms * 1e-3) / 1e6, 1)}
    # the interreflections: 64 paths per pixel, at most 2 and 4 surface vertices per path (incoherent secondary rays)
    res["indirect"] = {}
    vf = v[f.long()]
    face_n = torch.nn.functional.normalize(torch.cross(vf[:, 1] - vf[:, 0], vf[:, 2] - vf[:, 0], dim=-1), dim=-1)
    for depth in (2, 4):
        ms = timed(lambda: asset.shade_env_indirect(o, d, t, fi, b, env, tables, n_paths=64, max_depth=depth), a.reps)
        bounce, bounce_hits, shadow, visible, reached = 0, 0, 0, 0, [0] * depth
        rows = max(1, (1 << 21) // (64 * depth * a.size))
        for y0 in range(0, a.size, rows):
            s = slice(y0 * a.size, min(y0 + rows, a.size) * a.size)
            out = asset.shade_env_indirect(o[s], d[s], t[s], fi[s], b[s], env, tables, n_paths=64, max_depth=depth, dump=True,
                                           pixel_idx=torch.arange(s.start, s.stop, device=dev, dtype=torch.int32))
            face, wl = out["dump_face"], out["dump_light_dir"]
            bounce += int((face != -2).sum())  # every vertex whose BRDF sample counts casts one closest-hit ray
            bounce_hits += int((face >= 0).sum())
            # a shadow ray is cast for a light sample above the shading horizon on the front side of the vertex's face; count the
            # second condition, which the dump allows (the face is the one the bounce ray of the vertex before reached)
            own = face[:, :, :-1].clamp(min=0).long()
            shadow += int((((wl[:, :, 1:] * face_n[own]).sum(-1) > 0) & (wl[:, :, 1:] != 0).any(-1)).sum())
            visible += int(out["dump_light_vis"].sum())
            live = torch.cat([(fi[s] >= 0)[:, None, None].expand(-1, 64, 1), (out["dump_throughput"][:, :, :-1] != 0).any(-1)], 2)
            for j in range(depth):
                reached[j] += int(live[:, :, j].sum())
        paths = int((fi >= 0).sum()) * 64
        res["indirect"]["64x%d" % depth] = {"ms": ms, "paths": paths, "bounce_rays": bounce, "bounce_hits": bounce_hits, "shadow_rays": shadow,
                                            "visible": visible, "mrays_per_s": round((bounce + shadow) / (ms * 1e-3) / 1e6, 1),
                                            # the share of a hit pixel's path slots still under way at vertex j: the rest idle
                                            "live_share_per_vertex": [round(r / max(paths, 1), 4) for r in reached]}
    res["frame_64+64_depth2_64_ms"] = timed(lambda: render_asset_env(cam, asset, env, max_depth=2, n_paths=64), a.reps)
    res["frame_64+64_depth4_64_ms"] = timed(lambda: render_asset_env(cam, asset, env, max_depth=4, n_paths=64), a.reps)
    res["frame_64+64_ms"] = timed(lambda: render_asset_env(cam, asset, env), a.reps)
    res["frame_256+256_ms"] = timed(lambda: render_asset_env(cam, asset, env, n_light=256, n_brdf=256), a.reps)
    res["frame_64+64_2x2_ms"] = timed(lambda: render_asset_env(cam, asset, env, samples_per_axis=2), a.reps)
    line = json.dumps(res, sort_keys=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
