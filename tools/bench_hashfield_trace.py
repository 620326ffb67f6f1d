"""The device-resident tracer of the hash-grid field (csrc/hashgrid_trace.hip; TCNNSDF.as_traced) beside the callable
paths it leaves in place, on §28's frame: an --size x --size view (800) of the sphere-fitted 2 x 32 field (tests/test_gpu_hashgrid_fit.py:
make_field, fit), tracer defaults.  Three arms, alternating frame by frame after the warm-up:

    plain      SDFCallable(lambda x: field.sdf(x / 2 + 1/2)[..., 0])     the plain torch path under the callable tracer
    callable   field.as_callable(0.5, 0.5)                              the fused evaluation under the callable tracer (§28)
    traced     field.as_traced(0.5, 0.5)                                the field inside the tracer's kernels (§30)

A frame's time is the host clock from the call to the end of a device synchronise; reported are the median and the quartiles of
--frames frames (at least 9).  For the traced arm also: the host time to enqueue the frame (the call returns before the kernels
end), the hipEvent time per field-evaluating kernel from a separate pass with the library's event pairs on (iron_profile_*; the
rest of the frame -- scans, list kernels, memsets, gaps -- is the median frame minus their sum), and the ratio of lane evaluations
issued to evaluations that belonged to a live ray, which is what the wave-owns-64-rays loops pay for divergence.  The outputs of
the callable and the traced arm are compared bit for bit before anything is timed.  Prints one JSON line.

    python tools/bench_hashfield_trace.py [--size 800] [--frames 15] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from iron_amd import _lib, scenes  # noqa: E402
from iron_amd import raytracer as rt  # noqa: E402


def quartiles(xs):
    s = sorted(xs)
    n = len(s)
    return {"median": round(s[n // 2], 4), "q25": round(s[n // 4], 4), "q75": round(s[(3 * n) // 4], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="fitting steps of the field")
    a = ap.parse_args()
    if a.frames < 9:
        raise SystemExit("bench_hashfield_trace: at least 9 frames")
    if not torch.cuda.is_available():
        raise SystemExit("bench_hashfield_trace needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    from test_gpu_hashgrid_fit import fit, make_field
    with tempfile.TemporaryDirectory() as tmp:
        field = make_field(os.path.join(tmp, "fit.json")).to(dev)

    def f(p):
        sdf, _, grad = field.get_all(p, is_training=True)
        return sdf, grad
    first, last = fit(list(field.parameters()), f, dev, steps=a.steps)
    K, W2C = scenes.fixture_camera_matrices(a.size, a.size)
    cam = rt.Camera(a.size, a.size, K.to(dev), W2C.to(dev))
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = rt.intersect_sphere(o, d, 1.0)
    tracer = rt.RayTracer()
    with torch.no_grad():
        arms = {"plain": rt.SDFCallable(lambda x: field.sdf(x * 0.5 + 0.5)[..., 0]),
                "callable": field.as_callable(0.5, 0.5),
                "traced": field.as_traced(0.5, 0.5)}
        want = tracer(arms["callable"], o, d, near, far, hit, collect_stats=True)
        ref_stats = dict(tracer.last_stats)
        got = tracer(arms["traced"], o, d, near, far, hit, collect_stats=True)
        stats = dict(tracer.last_stats)
        for k in want:
            x, y = want[k], got[k]
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            if not torch.equal(x, y):
                raise SystemExit("bench_hashfield_trace: %s of the traced arm differs from the callable arm" % k)
        for _ in range(a.warmup):
            for sdf in arms.values():
                tracer(sdf, o, d, near, far, hit)
        torch.cuda.synchronize()
        wall = {k: [] for k in arms}
        enqueue = []
        for _ in range(a.frames):
            for k, sdf in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tracer(sdf, o, d, near, far, hit)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                if k == "traced":
                    enqueue.append((t1 - t0) * 1e3)
        # the per-kernel split, in a pass of its own: the event pairs cost host time
        _lib.profile_enable(True)
        _lib.profile_read()
        for _ in range(a.frames):
            tracer(arms["traced"], o, d, near, far, hit)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        _lib.profile_enable(False)
    kernels = {k: round(prof[k][0] / a.frames, 4) for k in ("sphere", "sampler", "bisect_a", "bisect_b")}
    res = {"tool": "bench_hashfield_trace", "size": a.size, "rays": int(o.shape[0]), "frames": a.frames, "fit_loss": [first, last],
           "hits": int(want["convergent_mask"].sum()), "bitwise_equal": True,
           "wall_ms": {k: quartiles(v) for k, v in wall.items()},
           "traced_q75_below_callable_q25": quartiles(wall["traced"])["q75"] < quartiles(wall["callable"])["q25"],
           "traced_enqueue_ms": quartiles(enqueue),
           "traced_kernel_ms": kernels,
           "traced_rest_ms": round(quartiles(wall["traced"])["median"] - sum(kernels.values()), 4),
           "traced_stats": stats, "callable_stats": ref_stats,
           "issued_over_live": round(stats["n_evals_issued"] / max(stats["n_evals"], 1), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
