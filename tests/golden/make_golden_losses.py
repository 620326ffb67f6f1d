"""Golden vectors G20 for the stage-2 image losses -- BUILD CONTAINER ONLY (imports the reference's models/image_losses.py; needs
scipy for its pyramid filter).

kornia is not installed: make_golden registers an empty placeholder, and this script gives it a `morphology.erosion` that is
tests/_loss_oracle.erosion (a restatement of kornia's flat-kernel geodesic erosion).  The masked SSIM cases therefore pin the
rest of ssim_loss_fn but not kornia itself: they are marked "erosion unpinned" in the archive's metadata, as closing / sobel
are for G8.

The input images and masks (uint8; X = u8 / 255 in float32 on the CPU) are not stored: they are rebuilt from the integer-only
recipe of tests/_loss_oracle.py (g20_images / g20_mask), and the archive keeps a SHA-256 of each.  Per case and loss: the
reference's value and input gradients from autograd in fp64 (the module cast to double) and in fp32.  Gradients are kept at 512
fixed sample indices, together with max|grad| of the fp64 run and the largest fp32-vs-fp64 difference over the whole array.  Also recorded: the pyramid filter `f`, the SSIM window, and the
inspect.signature of the module's public names (as JSON).

The archive is written with fixed zip timestamps, so a re-run reproduces g20_image_losses.npz bit for bit.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_losses.py
"""
from __future__ import annotations

import inspect
import io
import json
import os
import sys
import types
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (for _loss_oracle)
import make_golden as MG  # noqa: E402,F401  (placeholder kornia / icecream, reference on sys.path)

import _loss_oracle as O  # noqa: E402

_morph = types.ModuleType("kornia.morphology")
_morph.erosion = O.erosion
sys.modules["kornia"].morphology = _morph
sys.modules["kornia.morphology"] = _morph

import models.image_losses as IL  # noqa: E402  (reference)

OUT = os.path.join(HERE, "g20_image_losses.npz")
N_SAMPLES = 512


def to_f32(u8):
    return torch.from_numpy(u8).float() / 255.0


def run(kind, xu, yu, mu, dtype):
    x = to_f32(xu).to(dtype).requires_grad_(True)
    y = to_f32(yu).to(dtype).requires_grad_(True)
    if kind == "pyr":
        mod = IL.PyramidL2Loss(use_cuda=False)
        mod.f = mod.f.to(dtype)
        loss = mod(x, y)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = IL.ssim_loss_fn(x, y, None if mu is None else torch.from_numpy(mu).bool())
    dx, dy = torch.autograd.grad(loss, (x, y))
    return float(loss.detach()), dx.double().numpy().reshape(-1), dy.double().numpy().reshape(-1)


def describe(fn):
    return [{"name": p.name, "kind": p.kind.name, "default": None if p.default is inspect._empty else repr(p.default)}
            for p in inspect.signature(fn).parameters.values()]


def main():
    torch.set_num_threads(8)
    rng = np.random.default_rng(20)
    rec, meta = {}, {"cases": {}, "erosion": "unpinned: kornia is absent; kornia.morphology.erosion was tests/_loss_oracle.erosion"}
    imgs = {name: O.g20_images(name) for name in list(O.G20_IMAGES) + ["near96"]}
    masks = {name: O.g20_mask(name) for name in O.G20_MASKS}
    for name, (x, y) in imgs.items():
        rec["sha256__img__%s__x" % name] = np.array(O.sha256(x))
        rec["sha256__img__%s__y" % name] = np.array(O.sha256(y))
    for name, m in masks.items():
        rec["sha256__mask__%s" % name] = np.array(O.sha256(m))

    cases = [("s512", None, ("pyr", "ssim")), ("s96", None, ("pyr", "ssim")), ("s37x53", None, ("pyr", "ssim")),
             ("b2_64", None, ("pyr", "ssim")), ("s8x64", None, ("ssim",)), ("near96", None, ("pyr", "ssim")),
             ("s96", "holes96", ("ssim",)), ("s96", "border96", ("ssim",)), ("s512", "holes512", ("ssim",)),
             ("s512", "border512", ("ssim",))]
    for img, mname, kinds in cases:
        case = img if mname is None else "%s__%s" % (img, mname)
        xu, yu = imgs[img]
        mu = None if mname is None else masks[mname]
        n = xu.size
        idx = np.sort(rng.choice(n, N_SAMPLES, replace=False))
        rec["case__%s__idx" % case] = idx.astype(np.int32)
        meta["cases"][case] = {"image": img, "mask": mname, "losses": list(kinds), "shape": list(xu.shape),
                               "erosion": "unpinned" if mname else None}
        for kind in kinds:
            l64, dx64, dy64 = run(kind, xu, yu, mu, torch.float64)
            l32, dx32, dy32 = run(kind, xu, yu, mu, torch.float32)
            p = "case__%s__%s__" % (case, kind)
            rec[p + "loss64"], rec[p + "loss32"] = np.float64(l64), np.float64(l32)
            for g, g64, g32 in (("dx", dx64, dx32), ("dy", dy64, dy32)):
                rec[p + g + "64"] = g64[idx]
                rec[p + g + "32"] = g32[idx].astype(np.float32)
                rec[p + g + "max64"] = np.float64(np.abs(g64).max())
                rec[p + g + "gap"] = np.float64(np.abs(g32 - g64).max())
            print("%-22s %-4s loss64 %.10e  fp32 gap %.2e  grad gap %.2e / max %.2e" % (
                case, kind, l64, abs(l32 - l64), rec[p + "dxgap"], rec[p + "dxmax64"]))

    rec["pyramid_f"] = IL.PyramidL2Loss(use_cuda=False).f.numpy()
    rec["ssim_win"] = IL._fspecial_gauss_1d(11, 1.5).numpy()
    sigs = {"PyramidL2Loss": {"type": "class", "methods": {"__init__": describe(IL.PyramidL2Loss.__init__),
                                                           "forward": describe(IL.PyramidL2Loss.forward)}},
            "_fspecial_gauss_1d": {"type": "function", "params": describe(IL._fspecial_gauss_1d)},
            "gaussian_filter": {"type": "function", "params": describe(IL.gaussian_filter)},
            "ssim_loss_fn": {"type": "function", "params": describe(IL.ssim_loss_fn)}}
    rec["signatures_json"] = np.array(json.dumps(sigs, sort_keys=True))
    rec["meta_json"] = np.array(json.dumps(meta, sort_keys=True))

    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(rec[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
