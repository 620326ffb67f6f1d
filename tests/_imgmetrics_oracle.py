"""Restatement of evaluation/eval_image_folder.py's three metrics, the yardstick of iron_amd.image_metrics.

The reference script runs at import (it reads sys.argv and builds the LPIPS network at top level) and needs skimage, imageio and
lpips, so it cannot be called to record goldens.  What it computes is restated here, on the CPU:

  * psnr            eval_image_folder.py:22, 49: mse2psnr(np.mean((pred - trgt) ** 2)).
  * skimage_ssim    eval_image_folder.py:10-17 -> skimage.metrics.structural_similarity(data_range=1.0, win_size=11,
                    use_sample_covariance=False); `gaussian_weights` is not passed, so the window is scipy.ndimage.uniform_filter
                    (size 11; the very call skimage makes), `sigma` is inert, and `k1` / `k2` in lower case fall back to skimage's
                    K1 = 0.01, K2 = 0.03.  cov_norm = 1, S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), the
                    mean of S with a border of (11 - 1) // 2 = 5 pixels cropped, taken in float64 as skimage does.  The arithmetic
                    runs in the dtype of the arrays (skimage keeps float32 images in float32).
  * lpips           eval_image_folder.py:33, 55-57 -> lpips.LPIPS(net='alex'), version 0.1, on 2 x - 1.  Written from the published
                    description (the scaling layer, torchvision's AlexNet feature stack with taps after the five ReLUs, unit-normalised
                    channels with eps 1e-10, squared difference, bias-free 1x1 `lin` convolutions, spatial mean, sum); it has NOT been
                    compared with the lpips package.  torch-CPU conv2d / max_pool2d in the dtype asked for.
"""
from __future__ import annotations

import io

import numpy as np
import torch
import torch.nn.functional as F
from scipy.ndimage import uniform_filter

ALEX_LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_AFTER = (True, True, False, False, False)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def psnr(pred, trgt) -> float:
    mse = np.mean((pred - trgt) ** 2, dtype=np.float64)
    return float(-10. * np.log(mse + 1e-10) / np.log(10.))


def ssim_map(x, y):
    """S of one channel pair [H, W] (float32 or float64 arrays; the arithmetic runs in their dtype), border of 5 cropped."""
    if min(x.shape) < 11:
        raise ValueError("win_size exceeds image extent")
    C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
    ux, uy = uniform_filter(x, size=11), uniform_filter(y, size=11)
    uxx, uyy, uxy = uniform_filter(x * x, size=11), uniform_filter(y * y, size=11), uniform_filter(x * y, size=11)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S[5:-5, 5:-5]


def skimage_ssim(pred, trgt) -> float:
    """The mean over the three channels, as the script's loop."""
    ssim = 0.
    for ch in range(3):
        ssim += float(ssim_map(np.ascontiguousarray(trgt[:, :, ch]), np.ascontiguousarray(pred[:, :, ch])).mean(dtype=np.float64))
    return ssim / 3.


def lpips_input(img, dtype=torch.float64):
    """[H, W, 3] in [0, 1] -> [1, 3, H, W]: 2 x - 1, then the scaling layer."""
    x = torch.as_tensor(np.ascontiguousarray(img)).to(dtype).permute(2, 0, 1)[None] * 2. - 1.
    return (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)


def conv_relu(x, l, conv_w, conv_b):
    _, _, _, s, p = ALEX_LAYERS[l]
    return F.relu(F.conv2d(x, conv_w[l].to(x.dtype), conv_b[l].to(x.dtype), stride=s, padding=p))


def lpips_features(img, conv_w, conv_b, dtype=torch.float64):
    """The five tap maps [1, C, h, w] of one image."""
    x = lpips_input(img, dtype)
    taps = []
    for l in range(5):
        x = conv_relu(x, l, conv_w, conv_b)
        taps.append(x)
        if POOL_AFTER[l]:
            x = F.max_pool2d(x, 3, 2)
    return taps


def lpips_from_features(f0, f1, lin_w) -> float:
    total = 0.
    for l in range(5):
        a, b = f0[l], f1[l]
        na = a / (torch.sqrt((a ** 2).sum(dim=1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt((b ** 2).sum(dim=1, keepdim=True)) + 1e-10)
        d = ((na - nb) ** 2 * lin_w[l].to(a.dtype).view(1, -1, 1, 1)).sum(dim=1, keepdim=True)
        total = total + d.mean(dim=(2, 3), keepdim=True)
    return float(total.item())


def lpips(pred, trgt, conv_w, conv_b, lin_w, dtype=torch.float64) -> float:
    return lpips_from_features(lpips_features(pred, conv_w, conv_b, dtype), lpips_features(trgt, conv_w, conv_b, dtype), lin_w)


def naive_features(img, conv_w, conv_b):
    """lpips_features in fp64 by explicit loops over the output pixels (numpy; toy sizes only): an independent convolution."""
    x = lpips_input(img, torch.float64)[0].numpy()
    taps = []
    for l, (_, cout, k, s, p) in enumerate(ALEX_LAYERS):
        w, b = conv_w[l].double().numpy(), conv_b[l].double().numpy()
        xp = np.pad(x, ((0, 0), (p, p), (p, p)))
        ho, wo = (xp.shape[1] - k) // s + 1, (xp.shape[2] - k) // s + 1
        y = np.zeros((cout, ho, wo))
        for i in range(ho):
            for j in range(wo):
                patch = xp[:, i * s:i * s + k, j * s:j * s + k]
                for o in range(cout):
                    y[o, i, j] = max((patch * w[o]).sum() + b[o], 0.0)
        taps.append(torch.from_numpy(y)[None])
        x = y
        if POOL_AFTER[l]:
            ho, wo = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
            z = np.zeros((cout, ho, wo))
            for i in range(ho):
                for j in range(wo):
                    z[:, i, j] = x[:, 2 * i:2 * i + 3, 2 * j:2 * j + 3].max(axis=(1, 2))
            x = z
    return taps


def seeded_lpips_weights(seed: int = 0):
    """(conv_w, conv_b, lin_w): He-scaled convolutions, small biases, non-negative lin weights (as in the package), fp32 CPU."""
    g = torch.Generator().manual_seed(seed)
    conv_w, conv_b, lin_w = [], [], []
    for cin, cout, k, _, _ in ALEX_LAYERS:
        conv_w.append(torch.randn((cout, cin, k, k), generator=g) * float(np.sqrt(2.0 / (cin * k * k))))
        conv_b.append(torch.randn((cout,), generator=g) * 0.05)
        lin_w.append(torch.rand((cout,), generator=g) * 2.0)
    return conv_w, conv_b, lin_w


def write_checkpoints(alexnet_pth, lin_pth, conv_w, conv_b, lin_w):
    """Synthetic checkpoint files with the key names of torchvision's AlexNet and the lpips package's alex.pth."""
    idx = (0, 3, 6, 8, 10)
    alex = {}
    for l in range(5):
        alex["features.%d.weight" % idx[l]] = conv_w[l].clone()
        alex["features.%d.bias" % idx[l]] = conv_b[l].clone()
    alex["classifier.1.weight"] = torch.zeros(4, 4)  # the real checkpoint has more keys than the loader reads
    torch.save(alex, alexnet_pth)
    torch.save({"lin%d.model.1.weight" % l: lin_w[l].clone().view(1, -1, 1, 1) for l in range(5)}, lin_pth)


# ---- test images ----------------------------------------------------------------------------------------------------------------
def sized_image(photo_u8, H, W):
    """The fixture tiled / cropped to H x W (uint8 [H, W, 3])."""
    ry, rx = -(-H // photo_u8.shape[0]), -(-W // photo_u8.shape[1])
    return np.ascontiguousarray(np.tile(photo_u8, (ry, rx, 1))[:H, :W])


def partners(img_u8, seed: int = 0):
    """Degraded versions of an 8-bit image: additive noise (sigma 0.05), a 5x5 box blur, a PIL JPEG round trip at
    quality 60, and a half-black mask (as rendered backgrounds are)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    x = img_u8.astype(np.float64) / 255.
    out = {}
    out["noise"] = np.clip(np.rint((x + rng.normal(0.0, 0.05, x.shape)) * 255.), 0, 255).astype(np.uint8)
    out["blur"] = np.clip(np.rint(uniform_filter(x, size=(5, 5, 1), mode="nearest") * 255.), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img_u8).save(buf, format="JPEG", quality=60)
    buf.seek(0)
    out["jpeg"] = np.ascontiguousarray(np.asarray(Image.open(buf).convert("RGB"), dtype=np.uint8))
    m = img_u8.copy()
    m[:, : img_u8.shape[1] // 2] = 0
    out["mask"] = m
    return out
