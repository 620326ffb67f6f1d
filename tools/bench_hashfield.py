"""Fused hash-grid field evaluation (csrc/hashgrid_field.hip; TCNNSDF.eval_fused) beside the plain path it leaves in
place, on the check configuration of §27 (L 16, F 2, 2^19 entries, N 16, b 1.3819) with a 64-neuron, 2-hidden-layer ReLU head, at
n = 2^16, 2^18 and 2^20 uniform points.  Arms, alternating in one process, hipEvent medians over --reps after --warmup:

    plain_sdf / plain_get_all     field.sdf(x) under no_grad / field.get_all(x, is_training=False): encode, GEMMs, autograd
    fused / fused_grad            eval_fused(x) / eval_fused(x, gradient=True): one launch each
    encode                        iron_hashgrid_encode alone: the floor of any evaluation that walks the table once

Beside the times: kernel launches per call of each arm (counted by torch.profiler in one extra call after the timing).  The second
part traces an --size x --size view of the sphere-fitted field (tests/test_gpu_hashgrid_fit.py: make_field, fit) through a plain
callable and through as_callable(0.5, 0.5), with the split of tools/bench_trace_callable.py.  Prints one JSON line.

    python tools/bench_hashfield.py [--reps 20] [--warmup 3] [--ns 65536,262144,1048576] [--size 800] [--frames 5]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from iron_amd import hashgrid, tcnn_fields  # noqa: E402
from iron_amd import raytracer as rt  # noqa: E402
from iron_amd import scenes  # noqa: E402

CHECK = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.3819)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(fn):
    """kernel launches of one call, or None where the profiler is not available"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and not e.name.startswith(("Memcpy", "Memset")))
    except Exception as exc:   # noqa: BLE001
        print("bench_hashfield: launch count unavailable (%s)" % (exc,), file=sys.stderr)
        return None


def check_field(tmp, dev):
    conf = {"encoding": dict(CHECK, otype="HashGrid"),
            "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}}
    path = os.path.join(tmp, "check.json")
    with open(path, "w") as f:
        json.dump(conf, f)
    torch.manual_seed(0)
    field = tcnn_fields.TCNNSDF(path).to(dev)
    with torch.no_grad():
        field.sdf_encoding.params.uniform_(-0.1, 0.1)
    return field


def evaluation_part(a, dev, tmp):
    field = check_field(tmp, dev)
    enc = field.sdf_encoding
    g = torch.Generator().manual_seed(0)
    runs = []
    for n in [int(v) for v in a.ns.split(",")]:
        x = torch.rand(n, 3, generator=g).to(dev)

        def plain_sdf():
            with torch.no_grad():
                return field.sdf(x)

        arms = {"plain_sdf": plain_sdf,
                "plain_get_all": lambda: field.get_all(x, is_training=False),
                "fused": lambda: field.eval_fused(x),
                "fused_grad": lambda: field.eval_fused(x, gradient=True),
                "encode": lambda: hashgrid.encode(enc.desc, enc.n_params, x, enc.params.detach())}
        for _ in range(a.warmup):
            for fn in arms.values():
                fn()
        ms = {k: [] for k in arms}
        for _ in range(a.reps):                       # the arms alternate: clock and cache state are shared
            for k, fn in arms.items():
                ms[k].append(event_ms(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        x.requires_grad_(False)
        runs.append({"n": n, "ms": {k: round(v, 4) for k, v in med.items()},
                     "launches": {k: launches(fn) for k, fn in arms.items()},
                     "fused_over_encode": round(med["fused"] / med["encode"], 3),
                     "plain_sdf_over_fused": round(med["plain_sdf"] / med["fused"], 2),
                     "plain_get_all_over_fused_grad": round(med["plain_get_all"] / med["fused_grad"], 2)})
    return runs


def traced_part(a, dev, tmp):
    from bench_trace_callable import _TimedLib
    from test_gpu_hashgrid_fit import fit, make_field
    with torch.enable_grad():
        field = make_field(os.path.join(tmp, "fit.json")).to(dev)

        def f(p):
            sdf, _, grad = field.get_all(p, is_training=True)
            return sdf, grad
        first, last = fit(list(field.parameters()), f, dev)
    K, W2C = scenes.fixture_camera_matrices(a.size, a.size)
    cam = rt.Camera(a.size, a.size, K.to(dev), W2C.to(dev))
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = rt.intersect_sphere(o, d, 1.0)
    log = {"host_wait_s": 0.0, "kernel_events": [], "fn_events": [], "calls": 0, "evals": 0}

    def timed_fn(inner):
        def fn(x):
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea.record()
            v = inner(x)
            eb.record()
            log["fn_events"].append((ea, eb))
            log["calls"] += 1
            log["evals"] += int(x.shape[0])
            return v
        return fn

    init = rt._AnyTrace.__init__

    def timed_init(self, *args, **kw):
        init(self, *args, **kw)
        self.lib = _TimedLib(self.lib, log)
    rt._AnyTrace.__init__ = timed_init
    try:
        tracer = rt.RayTracer()
        fused = field.as_callable(0.5, 0.5)
        with torch.no_grad():
            arms = {"plain": rt.SDFCallable(timed_fn(lambda x: field.sdf(x * 0.5 + 0.5)[..., 0])),
                    "fused": rt.SDFCallable(timed_fn(fused.fn))}
            for _ in range(a.trace_warmup):
                for c in arms.values():
                    tracer(c, o, d, near, far, hit)
            torch.cuda.synchronize()
            parts = {k: [] for k in arms}
            for _ in range(a.frames):
                for k, c in arms.items():
                    log.update({"host_wait_s": 0.0, "kernel_events": [], "fn_events": [], "calls": 0, "evals": 0})
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = tracer(c, o, d, near, far, hit)
                    torch.cuda.synchronize()
                    parts[k].append({"wall_ms": (time.perf_counter() - t0) * 1e3,
                                     "in_callable_ms": sum(x.elapsed_time(y) for x, y in log["fn_events"]),
                                     "bookkeeping_ms": sum(x.elapsed_time(y) for x, y in log["kernel_events"]),
                                     "host_wait_ms": log["host_wait_s"] * 1e3, "calls": log["calls"], "evals": log["evals"],
                                     "hits": int(out["convergent_mask"].sum())})
    finally:
        rt._AnyTrace.__init__ = init

    def med(xs):
        return sorted(xs)[len(xs) // 2]
    res = {"size": a.size, "rays": int(o.shape[0]), "frames": a.frames, "fit_loss": [first, last]}
    for k, ps in parts.items():
        res[k] = {q: round(med([p[q] for p in ps]), 3) for q in ("wall_ms", "in_callable_ms", "bookkeeping_ms", "host_wait_ms")}
        res[k].update({q: ps[-1][q] for q in ("calls", "evals", "hits")})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns", default="65536,262144,1048576")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--trace-warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hashfield needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        out = {"tool": "bench_hashfield", "config": CHECK, "head": {"n_neurons": 64, "n_hidden_layers": 2, "activation": "ReLU"},
               "runs": evaluation_part(a, dev, tmp), "trace": traced_part(a, dev, tmp)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
