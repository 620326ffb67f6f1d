"""CPU emulation of the screen with a packed-fp16 epilogue: a candidate for csrc/mlp_h2.h, measured and not adopted.

tools/screen_margin.py emulates the screen whose hidden activations are softplus_100 in fp32, rounded once to fp16.  With the
packed-fp16 epilogue every hidden layer but the last rounds the accumulator to fp16 FIRST and computes softplus_100 on fp16 halves,
each instruction rounding its result to fp16:

    zh = fp16(z) | e = fp16(zh * c1h) | e = fp16(2^-|e|) | e = fp16(1 + e) | e = fp16(log2 e) | out = fp16(e * c2h + max(zh, 0))

with c1h = fp16(100 log2 e) = 144.25 and c2h = fp16(ln 2 / 100); the last step is one fused multiply-add.  (v_exp_f16 / v_log_f16
are within an ulp of the exact function; the emulation rounds the exact value.)  The last hidden layer keeps the fp32 form.

The --gate comparison is why the kernel keeps the fp32 epilogue: rounding the accumulator to fp16 before softplus re-rounds
every hidden activation, and the screen's output moves by about as much as its own fp16 error (median 6e-5 on S0, 3.5e-4 on a
generalised net), beyond what tests/test_gpu_screen_stream.py allows against tools/screen_margin.py.

    python3 tools/screen_margin_f16.py [--res 200] [--scenes S0,S1,S3] [--gen 1]     # margin report, as tools/screen_margin.py
    python3 tools/screen_margin_f16.py --gate                                          # against the fp32-epilogue emulation
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_margin as SM  # noqa: E402
from oracle import iron_ref as R  # noqa: E402

C1H = float(np.float16(100.0 * np.log2(np.e)))
C2H = float(np.float16(np.log(2.0) / 100.0))


def _h(t):
    return t.half().double()


def softplus100_f16(z):
    """The packed-fp16 epilogue of one hidden activation: fp32 accumulator in, fp16-valued tensor (as float32) out."""
    zh = _h(z)
    e = _h(zh * C1H)
    e = _h(torch.exp2(-e.abs()))
    e = _h(1.0 + e)
    e = _h(torch.log2(e))
    return _h(e * C2H + zh.clamp_min(0.0)).float()


@torch.no_grad()
def screen_forward(sd, spec, x):
    """The screen's SDF value of x [M,3] with the packed-fp16 epilogue (tools/screen_margin.py's screen_forward otherwise)."""
    inputs = R.positional_encoding(x * spec.scale, spec.multires) if spec.multires > 0 else x * spec.scale
    pe = SM._hr(inputs)
    h = pe
    n = spec.n_linear
    for l in range(n):
        w, b = R.effective_weight(sd, l)
        if l in spec.skip_in:
            h = torch.cat([h, pe], dim=-1)
            w = w / np.sqrt(2)
        if l < n - 1:
            w = SM._hr(w)
        h = F.linear(h, w, b)
        if l < n - 2:
            h = softplus100_f16(h)
        elif l == n - 2:
            h = R.softplus100(h)
    return h[..., 0] / spec.scale


@torch.no_grad()
def delta_of(sd, spec):
    x = SM.calibration_points()
    err = (screen_forward(sd, spec, x) - R.sdf_forward(sd, spec, x)[:, 0]).abs()
    err = err[torch.isfinite(err)]
    return max(SM.K_SCREEN * float(err.max()), SM.FLOOR)


@torch.no_grad()
def margin_report(sd, spec, res):
    delta = delta_of(sd, spec)
    x, f32 = SM.sampler_points(sd, spec, res)
    f1 = screen_forward(sd, spec, x)
    err = (f1 - f32).abs()
    fin = torch.isfinite(err)
    mx = float(err[fin].max())
    return {"samples": int(x.shape[0]), "max_err": mx, "median_err": float(err[fin].median()), "delta": delta,
            "coverage": delta / mx, "uncertain": float((f1.abs() <= delta).float().mean()),
            "le_1e-3": float((f1.abs() <= 1e-3).float().mean()), "le_1e-2": float((f1.abs() <= 1e-2).float().mean())}


def gate_points(n=100_000, seed=0):
    """The points tests/test_gpu_screen_stream.py compares the device screen on: the calibration set and n unit-ball points."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    x = x / x.norm(dim=1, keepdim=True) * torch.rand(n, 1, generator=g) ** (1 / 3)
    return torch.cat([SM.calibration_points(), x.float()], 0).contiguous()


@torch.no_grad()
def gate(sd, spec, x):
    """|fp16-epilogue emulation - fp32-epilogue emulation| on x: median and max."""
    d = (screen_forward(sd, spec, x) - SM.screen_forward(sd, spec, x)).abs()
    return {"median": float(d.median()), "max": float(d.max()), "finite": bool(torch.isfinite(d).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--scenes", default="S0,S1,S3")
    ap.add_argument("--gen", type=int, default=1)
    ap.add_argument("--gate", action="store_true", help="compare with the fp32-epilogue emulation on the GPU test's points")
    a = ap.parse_args()
    nets = [(s, SM.scene_net(s), 0) for s in a.scenes.split(",") if s] + [("gen%d" % g, SM.generalised_net(g), 1) for g in range(a.gen)]
    for name, (sd, spec), seed in nets:
        r = gate(sd, spec, gate_points(seed=seed)) if a.gate else margin_report(sd, spec, a.res)
        print(name, json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
