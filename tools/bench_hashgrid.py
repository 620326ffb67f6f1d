"""Hash-grid encoding on the GPU (csrc/hashgrid.hip, csrc/hashgrid_train.hip; iron_amd.hashgrid): device time of encode, encode + J,
backward (d_table + d_x) and backward-backward (d_dy + the second-order d_table) on the check configuration (L 16, F 2, 2^19
entries, N 16, b 1.3819: 6 098 120 entries, 48.8 MB of fp32) at n = 2^16, 2^18 and 2^20 uniform points.

Beside each time: the bytes gathered from the table per second (8 corners x F floats per point and level; the backward reads the
table twice -- d_x walks the levels per point -- and adds 8 F 64-bit integer atomics per point and level, reported as atomic bytes
per second).  For scale the line carries the one gather rate measured on this part so far, 8.6 TB/s chip-wide for uniformly random
1 152-byte rows of a 38 MB table served from the Infinity Cache; 8-byte random gathers and 64-bit integer atomics have no measured
rate to compare with, so these figures are measurements, not a distance to a target.  Times are hipEvent medians over --reps
launches after --warmup.  Prints one JSON line.

    python tools/bench_hashgrid.py [--reps 20] [--warmup 3] [--ns 65536,262144,1048576]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from iron_amd import hashgrid  # noqa: E402

CHECK = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.3819)
INFINITY_CACHE_ROW_GATHER_TBS = 8.6   # 1 152-B rows, 38 MB table, uniformly random


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns", default="65536,262144,1048576")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    enc = hashgrid.HashEncoding(**CHECK).to(dev)
    L, F = enc.n_levels, enc.n_features_per_level
    g = torch.Generator().manual_seed(0)
    table = (torch.rand(enc.n_params * F, generator=g) * 0.2 - 0.1).to(dev)
    out = {"config": CHECK, "n_params": enc.n_params, "table_MB": round(enc.n_params * F * 4 / 1e6, 1),
           "infinity_cache_row_gather_TBs": INFINITY_CACHE_ROW_GATHER_TBS, "runs": []}
    for n in [int(v) for v in a.ns.split(",")]:
        x = torch.rand(n, 3, generator=g).to(dev)
        dy = (torch.rand(n, L * F, generator=g) * 2 - 1).to(dev)
        gx = (torch.rand(n, 3, generator=g) * 2 - 1).to(dev)
        d, P = enc.desc, enc.n_params
        gather = n * L * 8 * F * 4                      # bytes read from the table by one walk of every (point, level)
        atomics = n * L * 8 * F * 8                     # bytes added by the 64-bit integer atomics of one scatter
        ms = {
            "encode": timed(lambda: hashgrid.encode(d, P, x, table), a.reps, a.warmup),
            "encode_jacobian": timed(lambda: hashgrid.encode(d, P, x, table, jacobian=True), a.reps, a.warmup),
            "backward": timed(lambda: hashgrid.backward(d, P, x, table, dy), a.reps, a.warmup),
            "backward_table_only": timed(lambda: hashgrid.backward(d, P, x, table, dy, want_x=False), a.reps, a.warmup),
            "backward_x_only": timed(lambda: hashgrid.backward(d, P, x, table, dy, want_table=False), a.reps, a.warmup),
            "backward_backward": timed(lambda: hashgrid.backward_backward(d, P, x, table, dy, gx), a.reps, a.warmup),
        }
        run = {"n": n, "ms": {k: round(v, 4) for k, v in ms.items()},
               "gather_TBs": {"encode": round(gather / ms["encode"] / 1e9, 3),
                              "encode_jacobian": round(gather / ms["encode_jacobian"] / 1e9, 3),
                              "backward_x_only": round(gather / ms["backward_x_only"] / 1e9, 3),
                              "backward_backward": round(gather / ms["backward_backward"] / 1e9, 3)},
               "atomic_TBs": {"backward_table_only": round(atomics / ms["backward_table_only"] / 1e9, 3),
                              "backward_backward": round(atomics / ms["backward_backward"] / 1e9, 3)},
               "store_TBs": {"encode": round(n * L * F * 4 / ms["encode"] / 1e9, 3),
                             "encode_jacobian": round(n * L * F * 16 / ms["encode_jacobian"] / 1e9, 3)}}
        out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
