"""Image evaluation metrics on the GPU (csrc/imgmetrics.hip, iron_amd.image_metrics): upload of an 8-bit pair, squared error, SSIM,
every LPIPS stage, the LPIPS forward in one call and the whole pair (evaluate_pair, host float out), at 800x800 and 512x512, by
hipEvents (median of --reps after a warm-up run of every shape).  LPIPS weights are seeded (He-scaled): the time does not depend on
their values.  For scale only, `torch_ops` holds the same three numbers from stock torch operators on the same card
(F.avg_pool2d for the window means, F.conv2d / F.max_pool2d for the AlexNet stack, both in fp32): information, no ratio is
promised.  `gflop` counts 2 x M x N x K of the five convolutions for both images, before the three-product split.  Prints one JSON line.

    python tools/bench_imgmetrics.py [--reps 20] [--sizes 800 512]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from iron_amd import image_metrics as M  # noqa: E402


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def seeded_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    cw = [torch.randn((co, ci, k, k), generator=g) * float(np.sqrt(2.0 / (ci * k * k))) for ci, co, k, _, _ in M.ALEX_LAYERS]
    cb = [torch.randn((co,), generator=g) * 0.05 for _, co, _, _, _ in M.ALEX_LAYERS]
    lw = [torch.rand((co,), generator=g) * 2.0 for _, co, _, _, _ in M.ALEX_LAYERS]
    return cw, cb, lw


def images(n, seed):
    """A smooth synthetic photo-like pair, uint8 [n, n, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64) / n
    base = np.stack([0.5 + 0.4 * np.sin(7 * x + 3 * y), 0.5 + 0.4 * np.cos(5 * x * y + 1), 0.3 + 0.6 * x * (1 - y)], axis=2)
    a = np.clip(np.rint(base * 255), 0, 255).astype(np.uint8)
    b = np.clip(np.rint((base + rng.normal(0, 0.05, base.shape)) * 255), 0, 255).astype(np.uint8)
    return a, b


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(med(ms), 4)


def conv_gflop(n):
    h = w = n
    total = 0.0
    for l, (ci, co, k, s, p) in enumerate(M.ALEX_LAYERS):
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        total += 2.0 * 2 * h * w * co * (k * k * ci)
        if M.ALEX_POOL_AFTER[l]:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return total / 1e9


def torch_ops(a, b, cw, cb, lw, reps):
    """The same three numbers from stock torch operators in fp32 (for scale)."""
    dev = a.device
    cw, cb, lw = [t.to(dev) for t in cw], [t.to(dev) for t in cb], [t.to(dev) for t in lw]
    shift = torch.tensor([-.030, -.088, -.188], device=dev).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], device=dev).view(1, 3, 1, 1)

    def chw(u):
        return (u.float() / 255.0).permute(2, 0, 1)[None]

    def mse():
        return ((chw(a) - chw(b)) ** 2).mean()

    def ssim():
        x, y = chw(a), chw(b)
        ux, uy = F.avg_pool2d(x, 11, 1), F.avg_pool2d(y, 11, 1)
        vx, vy, vxy = F.avg_pool2d(x * x, 11, 1) - ux * ux, F.avg_pool2d(y * y, 11, 1) - uy * uy, F.avg_pool2d(x * y, 11, 1) - ux * uy
        return (((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))).mean()

    def lpips():
        x = (torch.cat([chw(a), chw(b)]) * 2 - 1 - shift) / scale
        total = 0.0
        for l, (_, _, _, s, p) in enumerate(M.ALEX_LAYERS):
            x = F.relu(F.conv2d(x, cw[l], cb[l], stride=s, padding=p))
            n = x / (torch.sqrt((x * x).sum(dim=1, keepdim=True)) + 1e-10)
            total = total + (((n[0:1] - n[1:2]) ** 2) * lw[l].view(1, -1, 1, 1)).sum(dim=1).mean()
            if M.ALEX_POOL_AFTER[l]:
                x = F.max_pool2d(x, 3, 2)
        return total

    return {"mse_ms": timed(mse, reps), "ssim_ms": timed(ssim, reps), "lpips_ms": timed(lpips, reps),
            "method": "torch fp32: avg_pool2d window means, conv2d / max_pool2d stack"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 512])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_imgmetrics needs a GPU")
    dev = torch.device("cuda", 0)
    cw, cb, lw = seeded_weights()
    lp = M.LPIPS.from_state(cw, cb, lw, device=dev)
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "sizes": {}}
    for n in args.sizes:
        a_np, b_np = images(n, n)
        a, b = torch.from_numpy(a_np).to(dev), torch.from_numpy(b_np).to(dev)
        pa, pb = torch.from_numpy(a_np).pin_memory(), torch.from_numpy(b_np).pin_memory()
        row = {"gflop": round(conv_gflop(n), 2)}
        row["upload_ms"] = timed(lambda: (pa.to(dev, non_blocking=True), pb.to(dev, non_blocking=True)), args.reps)
        row["sqerr_ms"] = timed(lambda: M.squared_error_device(a, b), args.reps)
        row["ssim_ms"] = timed(lambda: M.skimage_ssim_device(a, b), args.reps)
        row["lpips_forward_ms"] = timed(lambda: lp.lpips_device(a, b), args.reps)
        row["lpips_conv_tflops"] = round(row["gflop"] / row["lpips_forward_ms"], 2)
        # every stage: the staged forward with an event pair around each library call
        stages = {}
        for rep in range(args.reps + 1):
            ev = []

            def stage(name, fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev.append((name, e0, e1))

            lp.run_staged(a, b, stage=stage)
            torch.cuda.synchronize()
            if rep:  # the first pass is the warm-up
                for name, e0, e1 in ev:
                    stages.setdefault(name, []).append(e0.elapsed_time(e1))
        row["lpips_stages_ms"] = {k: round(med(v), 4) for k, v in stages.items()}
        # the whole pair as the command runs it: numpy in, three Python floats out (upload, three metrics, one host wait)
        M.evaluate_pair(a_np, b_np, lpips=lp)
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals = M.evaluate_pair(a_np, b_np, lpips=lp)
            ms.append((time.perf_counter() - t0) * 1e3)
        row["evaluate_pair_ms"] = round(med(ms), 3)
        row["values"] = {"psnr": vals[0], "ssim": vals[1], "lpips_seeded_weights": vals[2]}
        row["torch_ops"] = torch_ops(a, b, cw, cb, lw, args.reps)
        res["sizes"]["%dx%d" % (n, n)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
