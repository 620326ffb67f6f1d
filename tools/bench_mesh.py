"""Marching cubes on the GPU (csrc/mcubes.hip): device time of iron_mc_count (count pass + block-sum scan + the 16-byte
readback) and iron_mc_emit (vertex + triangle passes) by hipEvents, at 256^3 and 512^3 on an analytic sphere and on a dense
gyroid; then NeuSRenderer.extract_geometry at 512^3 on scene S0's SDF (PyMCubes hidden, so the device path runs), split
into field evaluation and marching cubes, next to extract_fields' host-copy path.  Prints one JSON line.

    python tools/bench_mesh.py [--reps 5] [--res 256 512] [--e2e-res 512]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py --reps 1` (kernels k_mc_*).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from iron_amd import _lib  # noqa: E402


def field(kind: str, n: int, dev) -> torch.Tensor:
    g = torch.arange(n, dtype=torch.float32, device=dev)
    if kind == "sphere":
        c = g - (n - 1) / 2.0
        return 0.4 * n - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    w = 2.0 * math.pi / 8.0  # gyroid, period 8 cells: a large share of the cells is active
    s, co = torch.sin(g * w), torch.cos(g * w)
    return (s[:, None, None] * co[None, :, None] + s[None, :, None] * co[None, None, :] + s[None, None, :] * co[:, None, None]).contiguous()


def time_mc(u: torch.Tensor, reps: int) -> dict:
    lib = _lib.load()
    dev = u.device
    nx, ny, nz = u.shape
    nbytes = C.c_size_t(0)
    _lib.check(lib.iron_mc_workspace_bytes(nx, ny, nz, C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    nv, nt = C.c_int64(0), C.c_int64(0)
    st = _lib.stream_ptr(dev)
    _lib.check(lib.iron_mc_count(u.data_ptr(), nx, ny, nz, 0.0, ws.data_ptr(), C.byref(nv), C.byref(nt), st))
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
    tris = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
    count_ms, emit_ms = [], []
    for _ in range(reps + 1):  # the first round warms up
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _lib.check(lib.iron_mc_count(u.data_ptr(), nx, ny, nz, 0.0, ws.data_ptr(), C.byref(nv), C.byref(nt), st))
        e[1].record()
        _lib.check(lib.iron_mc_emit(u.data_ptr(), nx, ny, nz, 0.0, ws.data_ptr(), verts.data_ptr(), tris.data_ptr(), st))
        e[2].record()
        torch.cuda.synchronize()
        count_ms.append(e[0].elapsed_time(e[1]))
        emit_ms.append(e[1].elapsed_time(e[2]))
    count_ms, emit_ms = sorted(count_ms[1:]), sorted(emit_ms[1:])
    med = lambda x: x[len(x) // 2]  # noqa: E731
    n = nx * ny * nz
    return {"points": n, "verts": nv.value, "tris": nt.value, "workspace_mb": round(nbytes.value / 2 ** 20, 1),
            "count_scan_ms": round(med(count_ms), 4), "emit_ms": round(med(emit_ms), 4),
            "total_ms": round(med(count_ms) + med(emit_ms), 4), "count_scan_ms_min": round(count_ms[0], 4),
            "field_read_gbps": round(4.0 * n / (med(count_ms) * 1e-3) / 1e9, 1)}


def e2e(res: int, reps: int) -> dict:
    from iron_amd import scenes
    from iron_amd.mesh import extract_fields_gpu, marching_cubes
    from iron_amd.renderer import NeuSRenderer, extract_fields
    sys.modules["mcubes"] = None  # the device path of extract_geometry
    dev = torch.device("cuda", 0)
    sdf = scenes.build_networks("S0")["sdf_network"].to(dev)
    r = NeuSRenderer(None, sdf, None, None, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=0.0)
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    q = lambda p: -sdf.sdf(p)  # noqa: E731
    r.extract_geometry(lo, hi, resolution=64, threshold=0.0)  # warm-up: code objects, allocator
    out = {"res": res, "field_ms": [], "mc_ms": [], "extract_geometry_ms": [], "extract_fields_host_ms": []}
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u = extract_fields_gpu(lo, hi, res, q)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        v, t = marching_cubes(u)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del u, v, t
        verts, tris = r.extract_geometry(lo, hi, resolution=res, threshold=0.0)
        t3 = time.perf_counter()
        out["field_ms"].append((t1 - t0) * 1e3)
        out["mc_ms"].append((t2 - t1) * 1e3)
        out["extract_geometry_ms"].append((t3 - t2) * 1e3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    extract_fields(lo, hi, res, q)
    out["extract_fields_host_ms"].append((time.perf_counter() - t0) * 1e3)
    for k in ("field_ms", "mc_ms", "extract_geometry_ms", "extract_fields_host_ms"):
        x = sorted(out[k])
        out[k] = round(x[len(x) // 2], 2)
    out["verts"], out["tris"] = int(len(verts)), int(len(tris))
    out["sdf_evals"] = res ** 3
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--e2e-res", type=int, default=512, help="0: skip the extract_geometry timing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "mc": {}}
    for n in a.res:
        for kind in ("sphere", "gyroid"):
            u = field(kind, n, dev)
            res["mc"]["%s_%d" % (kind, n)] = time_mc(u, a.reps)
            del u
            torch.cuda.empty_cache()
    if a.e2e_res > 0:
        res["extract_geometry_S0"] = e2e(a.e2e_res, max(1, min(a.reps, 3)))
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
