"""Point-to-mesh distance on the GPU (csrc/meshdist.hip): BVH build time split into Morton keys / sort (torch.sort) / hierarchy /
boxes, query time per direction and Mqueries/s, and the end-to-end chamfer_distance, by hipEvents (median of --reps after a warm-up
run).  Meshes: an analytic sphere and the dense gyroid of tools/bench_mesh.py at 256^3 and 512^3, each against the level set
0.25 of the same field (a nearby surface), and scene S0's extract_geometry mesh at 512^3 against its own at 256^3.  For
scale, `cpu_reference` is the fp64 brute force of tests/_meshdist_oracle.py on the CPU (every face per query) on a small query
subsample, extrapolated to all the queries of one direction and marked as an extrapolation.  Prints one JSON line.

    python tools/bench_meshdist.py [--reps 5] [--res 256 512] [--s0 1]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_mesh import field  # noqa: E402
from iron_amd.mesh import marching_cubes  # noqa: E402
from iron_amd.mesh_distance import MeshBVH, chamfer_distance  # noqa: E402


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def time_build(v, f, reps):
    out = {"keys_ms": [], "sort_ms": [], "hierarchy_ms": [], "boxes_ms": [], "build_ms": []}
    bvh = MeshBVH(v, f)  # warm-up
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        ws, keys = bvh._keys()
        e[1].record()
        sk = bvh._sort(keys)
        e[2].record()
        bvh.workspace = ws
        bvh._hierarchy(sk)
        e[3].record()
        bvh._boxes(sk)  # ends with the one host wait of the build
        e[4].record()
        torch.cuda.synchronize()
        for k, (a, b) in zip(("keys_ms", "sort_ms", "hierarchy_ms", "boxes_ms", "build_ms"), ((0, 1), (1, 2), (2, 3), (3, 4), (0, 4))):
            out[k].append(e[a].elapsed_time(e[b]))
    return bvh, {k: round(med(x), 4) for k, x in out.items()}


def time_query(bvh, pts, reps):
    bvh.query(pts)
    ms = []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        bvh.query(pts)
        e[1].record()
        torch.cuda.synchronize()
        ms.append(e[0].elapsed_time(e[1]))
    m = med(ms)
    return {"queries": int(pts.shape[0]), "query_ms": round(m, 4), "mqueries_per_s": round(pts.shape[0] / (m * 1e-3) / 1e6, 1)}


def time_chamfer(va, fa, vb, fb, reps):
    chamfer_distance(va, fa, vb, fb)
    ms, val = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val = chamfer_distance(va, fa, vb, fb)  # returns a host float: the device work is done
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"chamfer_ms": round(med(ms), 3), "chamfer": val}


def cpu_reference(v, f, pts, n_sub=64):
    """The fp64 brute force of tests/_meshdist_oracle.py (every face per query) on the CPU, on n_sub queries."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _meshdist_oracle as O
    V = torch.from_numpy(v.cpu().numpy().astype(np.float64))
    F = torch.from_numpy(f.cpu().numpy().astype(np.int64))
    P = torch.from_numpy(pts[:n_sub].cpu().numpy().astype(np.float64))
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.perf_counter()
    O.point_mesh_squared_distance(P, V, F)
    s = time.perf_counter() - t0
    return {"subsample_queries": int(P.shape[0]), "subsample_s": round(s, 3),
            "extrapolated_s_one_direction": round(s * pts.shape[0] / P.shape[0], 1), "is_extrapolation": True,
            "method": "fp64 brute force over all faces, torch CPU"}


def pair(name, va, fa, vb, fb, reps, res, cpu=False):
    ba, build_a = time_build(va, fa, reps)
    bb, build_b = time_build(vb, fb, reps)
    row = {"faces_a": int(fa.shape[0]), "verts_a": int(va.shape[0]), "faces_b": int(fb.shape[0]), "verts_b": int(vb.shape[0]),
           "build_a": build_a, "build_b": build_b, "query_a_to_b": time_query(bb, va, reps), "query_b_to_a": time_query(ba, vb, reps)}
    row.update(time_chamfer(va, fa, vb, fb, reps))
    if cpu:
        row["cpu_reference"] = cpu_reference(vb, fb, va)
    res[name] = row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--s0", type=int, default=1, help="0: skip scene S0's 512^3 vs 256^3 pair")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshdist needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "pairs": {}}
    for n in a.res:
        for kind in ("sphere", "gyroid"):
            u = field(kind, n, dev)
            va, fa = marching_cubes(u)
            vb, fb = marching_cubes(u, threshold=0.25)  # the neighbouring level set: a nearby surface of the same density
            del u
            pair("%s_%d" % (kind, n), va, fa, vb, fb, a.reps, res["pairs"], cpu=(kind == "sphere" and n == a.res[0]))
            del va, fa, vb, fb
            torch.cuda.empty_cache()
    if a.s0:
        from iron_amd import scenes
        from iron_amd.renderer import NeuSRenderer
        sys.modules["mcubes"] = None  # the device path of extract_geometry
        sdf = scenes.build_networks("S0")["sdf_network"].to(dev)
        r = NeuSRenderer(None, sdf, None, None, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=0.0)
        lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
        meshes = {}
        for n in (512, 256):
            v, t = r.extract_geometry(lo, hi, resolution=n, threshold=0.0)
            meshes[n] = (torch.as_tensor(v, dtype=torch.float32).to(dev), torch.as_tensor(t).to(dev))
        pair("S0_512_vs_256", *meshes[512], *meshes[256], a.reps, res["pairs"])
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
