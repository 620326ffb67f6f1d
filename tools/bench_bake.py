"""Material texture bake on the GPU (csrc/texbake.hip, iron_amd.texture_bake): stage times of export_materials' bake on scene
S0 -- n_rounds of sample_surface(n_samples) into a texture_H x texture_W atlas -- split into counts (iron_bake_count, which
waits once for the total), sampling, material query (rendering_func.query_materials over MaterialPredictor), splat and
resolve.  The mesh is S0's marching-cubes mesh at --res^3 with a per-triangle UV atlas (tests/_bake_oracle.atlas; at 512^3 the
cells are below a texel, which changes nothing in the cost).  Each stage is timed by wall clock between device
synchronisations.  Prints one JSON line.

    python tools/bench_bake.py [--res 512] [--rounds 5] [--samples 5000000] [--tex 2048] [--reps 2]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_bake.py --reps 1` (kernels k_bake_*).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _bake_oracle as O  # noqa: E402
from iron_amd import scenes  # noqa: E402
from iron_amd.mesh import extract_geometry_gpu  # noqa: E402
from iron_amd.rendering_func import MaterialPredictor, query_materials  # noqa: E402
from iron_amd.texture_bake import SplatAccumulator, _count, _mesh, _sample  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=5_000_000)
    ap.add_argument("--tex", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--max-num-pts", type=int, default=320000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nets = {k: n.to(dev) for k, n in scenes.build_networks("S0").items()}
    sdf = nets["sdf_network"]
    with torch.no_grad():
        verts, tris = extract_geometry_gpu(torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), a.res, 0.0, lambda p: -sdf.sdf(p))
    uvs, fuv = O.atlas(len(tris), a.tex, 0.0)
    v, f, t, ft = _mesh(verts.float(), tris, uvs, fuv, dev)
    pred = MaterialPredictor(sdf, nets)

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    reps = []
    for rep in range(a.reps + 1):   # the first pass warms up allocator and code objects
        ms = dict(counts=0.0, sampling=0.0, material_query=0.0, splat=0.0, resolve=0.0)
        acc = SplatAccumulator(a.tex, a.tex, 7, max_samples=a.rounds * (a.samples + len(tris)), device=dev)
        n_total = 0
        for r in range(a.rounds):
            (ws, total), dt = sync_time(lambda: _count(v, f, ft, t.shape[0], a.samples, 0, r))
            ms["counts"] += dt
            (pts, uv, _), dt = sync_time(lambda: _sample(v, f, t, ft, ws, total, 0, r))
            ms["sampling"] += dt
            mat, dt = sync_time(lambda: query_materials(pred, pts, a.max_num_pts))
            ms["material_query"] += dt
            _, dt = sync_time(lambda: acc.add(pts, uv, mat))
            ms["splat"] += dt
            n_total += total
            del ws, pts, uv, mat
        _, dt = sync_time(acc.resolve)
        ms["resolve"] += dt
        if rep:
            reps.append(ms)
        del acc
    best = {k: min(m[k] for m in reps) for k in reps[0]}
    native = best["counts"] + best["sampling"] + best["splat"] + best["resolve"]
    out = {"tool": "bench_bake", "scene": "S0", "mc_res": a.res, "faces": int(len(tris)), "rounds": a.rounds,
           "samples_per_round": a.samples, "samples_total": int(n_total), "texture": [a.tex, a.tex],
           "stage_ms": {k: round(x, 3) for k, x in best.items()},
           "bake_kernels_ms": round(native, 3), "bake_kernels_over_query": round(native / best["material_query"], 4),
           "splat_taps_per_s": round(5 * n_total / (best["splat"] * 1e-3), 1),
           "splat_atomic_bytes_per_s": round(5 * n_total * 11 * 8 / (best["splat"] * 1e-3), 1),
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
