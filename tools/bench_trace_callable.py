"""The callable tracer beside the fused one: an 800 x 800 view of S0 traced as SDFCallable(lambda x: sdf(x)[..., 0]) -- the reference's
own evaluation schedule, every batch a call of the network's forward -- and as SDFHandle(sdf) on the fused HIP tracer, alternating,
after a warm-up of both.  Per frame it reports

    wall_ms           host clock around the call, ending in a device synchronise
    in_callable_ms    device time between an event recorded in front of each call of the function and one behind it
    bookkeeping_ms    device time of the iron_trace_any_* launches, an event pair around each entry (the counted read excluded)
    host_wait_ms      host clock inside iron_trace_any_read: the host waiting for the count it decides the next step on
    calls / evals     calls of the function, points handed to it

The three parts do not add up to the wall time: while the host waits the device drains, and between two launches it idles.

Run:  python tools/bench_trace_callable.py [--size 800] [--frames 5] [--warmup 2]     (prints one JSON line at the end)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
torch.set_grad_enabled(False)
from iron_amd import raytracer as rt  # noqa: E402
from iron_amd import scenes  # noqa: E402


class _TimedLib:
    """The library as _AnyTrace sees it: an event pair around every iron_trace_any_* entry, the host clock around the read."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("iron_trace_any_") or name == "iron_trace_any_workspace_bytes":
            return fn
        log = self._log

        def timed(*args):
            if name == "iron_trace_any_read":
                t0 = time.perf_counter()
                rc = fn(*args)
                log["host_wait_s"] += time.perf_counter() - t0
                return rc
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            log["kernel_events"].append((a, b))
            return rc
        return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trace_callable needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    sdf = scenes.build_networks("S0")["sdf_network"].to(dev)
    K, W2C = scenes.fixture_camera_matrices(args.size, args.size)
    cam = rt.Camera(args.size, args.size, K.to(dev), W2C.to(dev))
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = rt.intersect_sphere(o, d, 1.0)

    log = {"host_wait_s": 0.0, "kernel_events": [], "fn_events": [], "calls": 0, "evals": 0}

    def fn(x):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        v = sdf(x)[..., 0]
        b.record()
        log["fn_events"].append((a, b))
        log["calls"] += 1
        log["evals"] += int(x.shape[0])
        return v

    init = rt._AnyTrace.__init__

    def timed_init(self, *a, **k):
        init(self, *a, **k)
        self.lib = _TimedLib(self.lib, log)
    rt._AnyTrace.__init__ = timed_init

    tracer = rt.RayTracer()
    runs = {"callable": lambda: tracer(rt.SDFCallable(fn), o, d, near, far, hit),
            "fused": lambda: tracer(rt.SDFHandle(sdf), o, d, near, far, hit)}
    for _ in range(args.warmup):
        for run in runs.values():
            out = run()
    torch.cuda.synchronize()
    wall = {k: [] for k in runs}
    parts = []
    for _ in range(args.frames):
        for name, run in runs.items():
            log.update({"host_wait_s": 0.0, "kernel_events": [], "fn_events": [], "calls": 0, "evals": 0})
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            if name == "callable":
                parts.append({"in_callable_ms": sum(a.elapsed_time(b) for a, b in log["fn_events"]),
                              "bookkeeping_ms": sum(a.elapsed_time(b) for a, b in log["kernel_events"]),
                              "host_wait_ms": log["host_wait_s"] * 1e3, "calls": log["calls"], "evals": log["evals"],
                              "hits": int(out["convergent_mask"].sum())})

    def med(xs):
        return sorted(xs)[len(xs) // 2]
    result = {"tool": "bench_trace_callable", "scene": "S0", "size": args.size, "rays": int(o.shape[0]), "frames": args.frames,
              "callable_wall_ms": round(med(wall["callable"]), 3), "fused_wall_ms": round(med(wall["fused"]), 3),
              "callable_wall_ms_all": [round(x, 2) for x in wall["callable"]], "fused_wall_ms_all": [round(x, 2) for x in wall["fused"]]}
    for k in ("in_callable_ms", "bookkeeping_ms", "host_wait_ms"):
        result[k] = round(med([p[k] for p in parts]), 3)
    result.update({"calls": parts[-1]["calls"], "evals": parts[-1]["evals"], "hits": parts[-1]["hits"]})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
