"""Forward + backward time of the stage-2 image losses (pyramid L2 + masked SSIM, as render_surface.py:597-598 calls them):
the HIP path of iron_amd.image_losses against the torch restatement of tests/_loss_oracle.py (F.conv2d, avg_pool2d, the
erosion as a max-pool of the inverted mask) on the same GPU, timed with device events after a warmup.

    python tools/bench_losses.py [--sizes 512,800] [--iters 200] [--warmup 20] [--only native|torch] [--out FILE]

Prints one JSON line.  For launch counts run it once under `rocprofv3 --kernel-trace --stats -- python tools/bench_losses.py
--iters 1 --warmup 1 --only native` (and --only torch), separately from the timing run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from iron_amd.image_losses import PyramidL2Loss, ssim_loss_fn  # noqa: E402
import _loss_oracle as O  # noqa: E402


def torch_ssim(X, Y, mask, win_size=11):
    """The oracle's SSIM with the erosion as a max-pool of the inverted mask (what a torch user without kornia would write)."""
    r = win_size // 2
    keep = -F.max_pool2d(-mask.float(), win_size, stride=1, padding=r) > 0.5
    win = O.gauss_1d(win_size, 1.5).unsqueeze(0).to(X)
    mu1, mu2 = O._blur(X, win), O._blur(Y, win)
    s11 = O._blur(X * X, win) - mu1 * mu1
    s22 = O._blur(Y * Y, win) - mu2 * mu2
    s12 = O._blur(X * Y, win) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + 1e-4) / (mu1 * mu1 + mu2 * mu2 + 1e-4) * (2 * s12 + 9e-4) / (s11 + s22 + 9e-4)).mean(1, keepdim=True)
    smap = F.pad(smap, (r, r, r, r), value=1.0)
    return 1.0 - smap[keep].mean()


def make(size, dev):
    gen = torch.Generator().manual_seed(size)
    pred = torch.rand(1, 3, size, size, generator=gen).to(dev)
    gt = (pred.cpu() + 0.1 * torch.randn(1, 3, size, size, generator=gen)).clamp(0, 1).to(dev)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, size), torch.linspace(-1, 1, size), indexing="ij")
    mask = ((yy ** 2 + xx ** 2) < 0.7)[None, None].to(dev)
    return pred.requires_grad_(True), gt, mask


def step_native(pyr, pred, gt, mask):
    pred.grad = None
    loss = pyr(pred, gt) + 0.5 * ssim_loss_fn(pred, gt, mask)
    loss.backward()


def step_torch(pred, gt, mask):
    pred.grad = None
    loss = O.pyramid_l2(pred, gt) + 0.5 * torch_ssim(pred, gt, mask)
    loss.backward()


def time_it(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,800")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=("native", "torch"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_losses needs a GPU")
    dev = torch.device("cuda", 0)
    pyr = PyramidL2Loss()
    out = {"metric": "image_losses_fwd_bwd_us", "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "sizes": {}}
    for size in [int(s) for s in a.sizes.split(",")]:
        pred, gt, mask = make(size, dev)
        row = {}
        # alternate the two paths so drift on a shared host hits both
        for rep in range(2):
            if a.only in (None, "native"):
                row.setdefault("native_us", []).append(time_it(lambda: step_native(pyr, pred, gt, mask), a.iters, a.warmup))
            if a.only in (None, "torch"):
                row.setdefault("torch_us", []).append(time_it(lambda: step_torch(pred, gt, mask), a.iters, a.warmup))
        for k in list(row):
            row[k] = round(min(row[k]), 2)
        if "native_us" in row and "torch_us" in row:
            row["speedup"] = round(row["torch_us"] / row["native_us"], 2)
        out["sizes"][str(size)] = row
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
