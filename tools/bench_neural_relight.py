"""Environment-map relighting of the neural scene on the GPU (iron_amd/neural_relight.py, csrc/envlight.hip k_nenv_*, RayTracer.occluded;
DESIGN.md §19): relight_camera on scene S0 and on the field bumpy04_s1 of tests/_hard_fields.py (S0's material networks on both)
from the fixture camera at 400 x 400 and 800 x 800 with 64 + 64 samples per pixel, under the synthetic sky of tools/bench_envlight.py.
Per frame, by device event pairs around the stages (the median frame of --reps after a warm-up): ms for the G-buffer, the emit (which
includes the host's read of the shadow-ray count per block), the trace and the resolve; shadow rays per second of the trace stage
and of the frame; the share of shadow rays occluded; SDF evaluations per shadow ray from the tracer's counters (a separate, untimed
run: a call that collects the counters evaluates every sample the screen lists, so the figure is an upper bound of the timed run's).
The same at shadow_eps 3e-4 and 3e-3 beside the default 1e-3, at 400 x 400, with the PSNR of each image against the default's.

Export loss, S0: the mesh is exported (export_mesh on a --export-res^3 grid, export_uv, export_materials at 2048^2) and rendered by
render_asset_env with the same camera, map, counts, seed and samples_per_axis; PSNR and SSIM (iron_amd.image_metrics, on the 8-bit
clip(x^(1/2.2)) images both command lines write) of the asset's render against the neural relight.  export_mesh writes its faces
wound inwards (marching cubes' winding on an SDF that is positive outside) and the environment integrator leaves back-facing hits
black, so the asset is compared with every face turned round; the mean colour of the asset as written is reported beside it.  Writes one JSON line to
profiles/neural_relight_bench.json and prints it.

--arm indirect measures the interreflections instead: the same two fields at the first of --sizes, 64 + 64 direct
samples and 64 paths per pixel at max_depth 2 and 4.  Per frame (the median of --reps after a warm-up, device event pairs): ms per
stage of the direct pass and of the path pass (path_emit includes the host's read of the two ray counts per block and depth), the
direct stages' sum beside the whole frame, bounce rays per second of the bounce stage (forward with chunk = 1) and shadow rays per
second of the path pass's occlusion stage beside the direct pass's, the alive share of the paths at every depth, and SDF evaluations
per bounce ray from the tracer's counters (a separate, untimed run).  It writes its line as the second line of the same file and leaves
the first as it is.

    python tools/bench_neural_relight.py [--reps 3] [--export-res 256] [--sizes 400 800] [--no-export] [--arm direct|indirect]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bench_envlight import sky  # noqa: E402


def to8(img):
    """the 8-bit image of the command lines: clip(x^(1/2.2)) * 255, on the device"""
    return (img.clamp_min(0).pow(1.0 / 2.2).clamp(0, 1) * 255.0).to(torch.uint8)


def frame(cam, sdf, tr, nets, env, reps, **kw):
    """relight_camera `reps` times after a warm-up -> (the median frame's figures, the last image)"""
    from iron_amd.neural_relight import relight_camera
    relight_camera(cam, sdf, tr, nets, env, **kw)
    runs = []
    for _ in range(reps):
        stats = {}
        res = relight_camera(cam, sdf, tr, nets, env, stats=stats, **kw)
        runs.append(stats)
    runs.sort(key=lambda s: sum(s["ms"].values()))
    s = runs[len(runs) // 2]
    ms = {k: round(v, 3) for k, v in s["ms"].items()}
    total = sum(s["ms"].values())
    rays = s["shadow_rays"]
    out = {"ms": ms, "frame_ms": round(total, 3), "hits": int(res["convergent_mask"].sum()), "shadow_rays": rays, "occluded": s["occluded"],
           "occluded_share": round(s["occluded"] / max(rays, 1), 5),
           "trace_mrays_per_s": round(rays / max(s["ms"]["trace"], 1e-9) / 1e3, 2),
           "frame_mrays_per_s": round(rays / max(total, 1e-9) / 1e3, 2)}
    return out, res["color"]


DIRECT_STAGES = ("gbuffer", "emit", "trace", "resolve")


def indirect_frame(cam, sdf, tr, nets, env, reps, depth, n_paths=64):
    """relight_camera with the interreflections, `reps` times after a warm-up -> the median frame's figures"""
    from iron_amd.neural_relight import relight_camera
    kw = dict(max_depth=depth, n_paths=n_paths)
    relight_camera(cam, sdf, tr, nets, env, **kw)
    runs = []
    for _ in range(reps):
        stats = {}
        res = relight_camera(cam, sdf, tr, nets, env, stats=stats, **kw)
        runs.append(stats)
    runs.sort(key=lambda s: sum(s["ms"].values()))
    s = runs[len(runs) // 2]
    total, direct = sum(s["ms"].values()), sum(s["ms"][k] for k in DIRECT_STAGES)
    paths = max(s["alive"][0], 1)
    counters = {"trace_stats": True}   # the tracer's counters, untimed
    relight_camera(cam, sdf, tr, nets, env, stats=counters, **kw)
    return {"ms": {k: round(v, 3) for k, v in s["ms"].items()}, "frame_ms": round(total, 3), "direct_ms": round(direct, 3),
            "indirect_ms": round(total - direct, 3), "hits": int(res["convergent_mask"].sum()), "n_paths": n_paths, "max_depth": depth,
            "bounce_rays": s["bounce_rays"], "bounce_hits": s["bounce_hits"], "indirect_shadow_rays": s["indirect_shadow_rays"],
            "indirect_occluded": s["indirect_occluded"], "direct_shadow_rays": s["shadow_rays"],
            "bounce_mrays_per_s": round(s["bounce_rays"] / max(s["ms"]["path_bounce"], 1e-9) / 1e3, 2),
            "indirect_shadow_mrays_per_s": round(s["indirect_shadow_rays"] / max(s["ms"]["path_shadow"], 1e-9) / 1e3, 2),
            "direct_shadow_mrays_per_s": round(s["shadow_rays"] / max(s["ms"]["trace"], 1e-9) / 1e3, 2),
            "alive_share": [round(a / paths, 5) for a in s["alive"]],
            "evals_per_bounce_ray": round(counters["bounce_tracer"]["n_evals"] / max(counters["bounce_rays"], 1), 3),
            "mean_indirect": round(float(res["indirect_color"].mean()), 6), "mean_color": round(float(res["color"].mean()), 6)}


def write_line(path, line, at):
    """`line` as line `at` of the file, the other lines kept"""
    lines = []
    if os.path.exists(path):
        with open(path) as fp:
            lines = [x for x in fp.read().split("\n") if x]
    while len(lines) <= at:
        lines.append("{}")
    lines[at] = line
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fp:
        fp.write("\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("direct", "indirect"), default="direct")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--export-res", type=int, default=256, dest="export_res")
    ap.add_argument("--sizes", type=int, nargs="+", default=[400, 800])
    ap.add_argument("--no-export", action="store_true", dest="no_export")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neural_relight_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_neural_relight needs a GPU")
    import _hard_fields as HF
    from iron_amd import image_metrics, scenes
    from iron_amd.envmap import EnvMap
    from iron_amd.neural_relight import relight_camera
    from iron_amd.raytracer import Camera, RayTracer

    dev = torch.device("cuda", 0)
    nets = {k: v.to(dev) for k, v in scenes.build_networks("S0").items()}
    fields = {"S0": nets["sdf_network"], "bumpy04_s1": HF.build("bumpy04_s1").to(dev)}
    env = EnvMap(sky(512, 1024, dev))
    tr = RayTracer()
    res = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "samples": [64, 64], "envmap": [512, 1024], "frames": {}, "shadow_eps": {}}

    def camera(size):
        K, W2C = scenes.fixture_camera_matrices(size, size)
        return Camera(size, size, K.to(dev), W2C.to(dev))

    if a.arm == "indirect":
        res = {"arm": "indirect", "device": res["device"], "reps": a.reps, "samples": [64, 64], "envmap": [512, 1024], "size": a.sizes[0],
               "frames": {}}
        for name, sdf in fields.items():
            for depth in (2, 4):
                res["frames"]["%s_%d_depth%d" % (name, a.sizes[0], depth)] = indirect_frame(camera(a.sizes[0]), sdf, tr, nets, env, a.reps, depth)
        line = json.dumps(res, sort_keys=True)
        write_line(a.out, line, 1)
        print(line)
        return

    for name, sdf in fields.items():
        for size in a.sizes:
            row, _ = frame(camera(size), sdf, tr, nets, env, a.reps)
            stats = {"trace_stats": True}   # the tracer's counters, untimed
            relight_camera(camera(size), sdf, tr, nets, env, stats=stats)
            row["evals_per_shadow_ray"] = round(stats["tracer"]["n_evals"] / max(stats["shadow_rays"], 1), 3)
            row["sampled_share"] = round(stats["tracer"]["n_sampler"] / max(stats["shadow_rays"], 1), 5)
            res["frames"]["%s_%d" % (name, size)] = row
        # the offset of the shadow rays' origins: a parameter; what it changes
        cam = camera(a.sizes[0])
        base = None
        for eps in (1e-3, 3e-4, 3e-3):
            row, img = frame(cam, sdf, tr, nets, env, 1, shadow_eps=eps)
            if base is None:
                base = img
            res["shadow_eps"]["%s_%d_%g" % (name, a.sizes[0], eps)] = {
                "shadow_rays": row["shadow_rays"], "occluded_share": row["occluded_share"], "frame_ms": row["frame_ms"],
                "mean_color": round(float(img.mean()), 6), "psnr_vs_default": round(image_metrics.psnr(to8(img), to8(base)), 3)}

    if not a.no_export:
        from iron_amd.export_materials import export_materials, read_obj
        from iron_amd.export_mesh import export_mesh
        from iron_amd.export_uv import export_uv
        from iron_amd.mesh_render import MeshAsset, render_asset_env
        from iron_amd.rendering_func import MaterialPredictor
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "mesh.obj")
            with torch.no_grad():
                export_mesh(lambda x: nets["sdf_network"](x)[..., 0], path, resolution=a.export_res)
            export_uv(path, path)
            baked = export_materials(path, MaterialPredictor(nets["sdf_network"], nets), os.path.join(tmp, "out"), seed=3)
            v, t, f, ft = read_obj(path)
            # export_mesh keeps marching cubes' winding: the normals of an SDF that is positive outside point INTO the surface
            # (iron_amd/export_mesh.py), and the environment integrator leaves a back-facing hit black.  The comparison below is made
            # on the asset with every face turned round; the asset as written is reported once, for the record.
            as_written = MeshAsset(v, f, t, ft, baked["material"], weight=baked["weight"], device=dev)
            asset = MeshAsset(v, f[:, [0, 2, 1]], t, ft[:, [0, 2, 1]], baked["material"], weight=baked["weight"], device=dev)
        loss = {"export_res": a.export_res, "faces": int(len(f)), "texture": [2048, 2048], "winding": "turned outwards for the comparison"}
        kw = dict(n_light=64, n_brdf=64, seed=0, samples_per_axis=1)
        loss["as_written_mean_color_%d" % a.sizes[0]] = round(float(render_asset_env(camera(a.sizes[0]), as_written, env, **kw)["color"].mean()), 6)
        for size in a.sizes:
            cam = camera(size)
            mesh_img = render_asset_env(cam, asset, env, **kw)
            for eps in (1e-3, 3e-4, 3e-3):
                neural = relight_camera(cam, nets["sdf_network"], tr, nets, env, shadow_eps=eps, **kw)
                both = neural["convergent_mask"] & mesh_img["convergent_mask"]
                p8, t8 = to8(mesh_img["color"]), to8(neural["color"])
                loss["%d_%g" % (size, eps)] = {
                    "psnr": round(image_metrics.psnr(p8, t8), 3), "ssim": round(image_metrics.skimage_ssim(p8, t8), 5),
                    "mask_flips": int((neural["convergent_mask"] != mesh_img["convergent_mask"]).sum()),
                    "mean_color_neural": round(float(neural["color"][both].mean()), 6),
                    "mean_color_asset": round(float(mesh_img["color"][both].mean()), 6)}
        res["export_loss_S0"] = loss
    line = json.dumps(res, sort_keys=True)
    write_line(a.out, line, 0)
    print(line)


if __name__ == "__main__":
    main()
