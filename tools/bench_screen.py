"""Isolated cost of the dense sampler's screen: the batched SDF value kernel on the h2 core (k_sdf_values_h2, three products
per MAC) against the same kernel on the screen (k_sdf_values_h1, sdf_hidden_stack_h1: one product per MAC), N points of the
tracer's unit ball, hipEvent timing, interleaved.  Also prints the screen's error against h2 on those points."""
import argparse
import json
import os
import sys

import torch
torch.set_grad_enabled(False)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iron_amd import _lib, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 22)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--scene", default="S0")
ap.add_argument("--json", default=None)
a = ap.parse_args()

lib = _lib.load()
net = scenes.build_networks(a.scene)["sdf_network"].cuda()
g = torch.Generator(device="cpu").manual_seed(0)
x = torch.randn(a.n, 3, generator=g)
x = (x / x.norm(dim=1, keepdim=True) * torch.rand(a.n, 1, generator=g) ** (1 / 3)).cuda().contiguous()
h = net.hip_net()
st = _lib.stream_ptr(x.device)
out2 = torch.empty(a.n, device="cuda")
out1 = torch.empty(a.n, device="cuda")


def h2():
    _lib.check(lib.iron_sdf_forward(h.handle, x.data_ptr(), a.n, out2.data_ptr(), 1, st))


def h1():
    _lib.check(lib.iron_sdf_screen_forward(h.handle, x.data_ptr(), a.n, out1.data_ptr(), st))


for f in (h2, h1, h2, h1):
    f()
torch.cuda.synchronize()
t = {"h2": [], "h1": []}
for _ in range(a.iters):
    for name, f in (("h2", h2), ("h1", h1)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        t[name].append(e0.elapsed_time(e1))
m2, m1 = sorted(t["h2"])[len(t["h2"]) // 2], sorted(t["h1"])[len(t["h1"]) // 2]
d = (out1 - out2).abs()
res = {"n": a.n, "scene": a.scene, "h2_ms": m2, "h1_ms": m1, "ratio": m1 / m2, "h2_all": t["h2"], "h1_all": t["h1"],
       "max_err": d.max().item(), "median_err": d.median().item(), "finite": bool(torch.isfinite(out1).all().item())}
for thr in (1e-3, 3e-3, 1e-2):
    res["frac_abs_le_%g" % thr] = (out1.abs() <= thr).float().mean().item()
print(json.dumps(res))
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
