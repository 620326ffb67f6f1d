"""Torch restatement of the reference's stage-2 image losses (models/image_losses.py) for the tests: PyramidL2Loss and
ssim_loss_fn with plain F.conv2d / F.avg_pool2d, and the kornia erosion the SSIM mask goes through (kornia is not a
dependency).  Runs on any device and dtype; differentiable through torch autograd.  Test infrastructure only, like
_mc_oracle.py."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def pyramid_taps() -> np.ndarray:
    """scipy.ndimage.gaussian_filter(dirac7x7, 1.0) in float32, in closed form (see iron_amd.image_losses.pyramid_taps)."""
    x = np.arange(-4, 5, dtype=np.float64)
    phi = np.exp(-0.5 * x ** 2)
    phi = phi / phi.sum()
    g = np.zeros(7, dtype=np.float64)
    for p, v in zip(range(-1, 8), phi):
        g[-p - 1 if p < 0 else (13 - p if p > 6 else p)] += v
    return (g[None, :] * g.astype(np.float32).astype(np.float64)[:, None]).astype(np.float32)


def pyramid_filter(dtype=torch.float32, device="cpu") -> torch.Tensor:
    f = torch.zeros(3, 3, 7, 7, dtype=torch.float32)
    gf = torch.from_numpy(pyramid_taps())
    for c in range(3):
        f[c, c] = gf
    return f.to(device=device, dtype=dtype)


def pyramid_l2(pred, trgt, f=None):
    f = pyramid_filter(pred.dtype, pred.device) if f is None else f.to(pred)
    d = pred - trgt
    h, w = pred.shape[-2:]
    loss = d.pow(2).sum() / (h * w)
    for k in range(1, 5):
        d = F.avg_pool2d(F.conv2d(d, f, padding=3), 2)
        s = float(2 ** k)
        loss = loss + d.pow(2).sum() / ((h / s) * (w / s))
    return loss


def gauss_1d(size, sigma) -> torch.Tensor:
    """The reference's _fspecial_gauss_1d: float32, [1, 1, size]."""
    coords = torch.arange(size, dtype=torch.float)
    coords -= size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.unsqueeze(0).unsqueeze(0)


def erosion(mask: torch.Tensor, kernel: torch.Tensor) -> torch.Tensor:
    """kornia.morphology.erosion(mask, kernel) for a flat all-ones kernel with the default geodesic border: the minimum over
    the in-image part of the window (pixels outside the image never win).  Unfold form, as kornia computes it."""
    kh, kw = kernel.shape
    big = torch.finfo(mask.dtype).max
    x = F.pad(mask, (kw // 2, (kw - 1) // 2, kh // 2, (kh - 1) // 2), mode="constant", value=big)
    x = x.unfold(2, kh, 1).unfold(3, kw, 1)
    return x.amin(dim=(-2, -1))


def min_filter(mask: torch.Tensor, k: int) -> torch.Tensor:
    """An independent statement of the same erosion: a max-pool of the inverted mask (max_pool2d pads with -inf)."""
    return -F.max_pool2d(-mask, k, stride=1, padding=k // 2)


def _blur(x, win):
    c = x.shape[1]
    win = win.repeat([c, 1, 1, 1])
    out = x
    for i, s in enumerate(x.shape[2:]):
        if s >= win.shape[-1]:
            out = F.conv2d(out, weight=win.transpose(2 + i, -1), stride=1, padding=0, groups=c)
    return out


def ssim(X, Y, mask=None, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    win = gauss_1d(win_size, win_sigma).unsqueeze(0).to(X.device, dtype=X.dtype)  # [1, 1, 1, ws]
    C1 = (K[0] * data_range) ** 2
    C2 = (K[1] * data_range) ** 2
    mu1, mu2 = _blur(X, win), _blur(Y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11 = _blur(X * X, win) - mu1_sq
    s22 = _blur(Y * Y, win) - mu2_sq
    s12 = _blur(X * Y, win) - mu1_mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    m = (((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs).mean(dim=1, keepdim=True)
    if mask is not None:
        r = win_size // 2
        m = F.pad(m, (r, r, r, r), mode="constant", value=1.0)
        keep = erosion(mask.float(), torch.ones(win_size, win_size, device=mask.device)) > 0.5
        m = m[keep]
    return 1.0 - m.mean()


# ---- G20 inputs -------------------------------------------------------------------------------------------------------------
# The golden images and masks are not stored: they are rebuilt from this recipe, which uses integer arithmetic only, so every
# numpy on every host makes the same bytes (G20 records a SHA-256 of each to catch any drift).

_M32 = np.uint64(0xFFFFFFFF)


def _hash(n: int, seed: int) -> np.ndarray:
    """A 32-bit integer hash of the indices 0..n-1 under `seed` (uint64 arithmetic, no overflow)."""
    x = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64((seed * 0x85EBCA77) & 0xFFFFFFFF)) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def _ints(seed: int, n: int, lo: int, hi: int) -> np.ndarray:
    """n integers in [lo, hi]."""
    return (_hash(n, seed) % np.uint64(hi - lo + 1)).astype(np.int64) + lo


def recipe_image(seed: int, b: int, h: int, w: int) -> np.ndarray:
    """A render-like uint8 image [b, 3, h, w]: a shading gradient, six paraboloid blobs, noise of +-4 levels."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    out = np.zeros((b, 3, h, w), dtype=np.int64)
    for p in range(3 * b):
        r = _ints(seed * 1000 + p, 32, 0, 1 << 20)
        v = 60 + (yy * (r[0] % 121 - 60)) // max(h, 1) + (xx * (r[1] % 121 - 60)) // max(w, 1)
        for k in range(6):
            cy, cx = r[2 + 4 * k] % h, r[3 + 4 * k] % w
            s2 = (r[4 + 4 * k] % (max(h, w) // 2) + 3) ** 2
            amp = r[5 + 4 * k] % 251 - 100
            d2 = (yy - cy) ** 2 + (xx - cx) ** 2
            v = v + amp * np.maximum(s2 - d2, 0) // s2
        out.reshape(3 * b, h, w)[p] = v + _ints(seed * 1000 + 500 + p, h * w, -4, 4).reshape(h, w)
    return np.clip(out, 0, 255).astype(np.uint8)


def recipe_perturb(seed: int, x: np.ndarray, amp: int) -> np.ndarray:
    """x plus uniform integer noise in [-amp, amp], clipped."""
    y = x.astype(np.int64) + _ints(seed, x.size, -amp, amp).reshape(x.shape)
    return np.clip(y, 0, 255).astype(np.uint8)


def recipe_near(seed: int, x: np.ndarray) -> np.ndarray:
    """pred ~ gt: 2 % of the values moved by one level."""
    r = _hash(x.size, seed).reshape(x.shape)
    step = np.where(r % np.uint64(50) == 0, np.where((r >> np.uint64(8)) & np.uint64(1), 1, -1), 0)
    return np.clip(x.astype(np.int64) + step, 0, 255).astype(np.uint8)


def recipe_mask(seed: int, b: int, h: int, w: int, border: bool) -> np.ndarray:
    """A silhouette with five holes and a speckle of single missing pixels, uint8 [b, 1, h, w]; `border`: the object runs off the
    left and bottom edges."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    m = np.zeros((b, 1, h, w), dtype=np.uint8)
    for i in range(b):
        cy, cx, ry, rx = (3 * h // 4, w // 5, 9 * h // 20, 27 * w // 50) if border else (h // 2, w // 2, h // 3, 2 * w // 5)
        inside = (yy - cy) ** 2 * rx * rx + (xx - cx) ** 2 * ry * ry < ry * ry * rx * rx
        r = _ints(seed * 100 + i, 15, 0, 1 << 20)
        for k in range(5):
            hy, hx = h // 5 + r[3 * k] % (3 * h // 5), w // 5 + r[3 * k + 1] % (3 * w // 5)
            hr = 2 + r[3 * k + 2] % max(h // 16, 1)
            inside &= (yy - hy) ** 2 + (xx - hx) ** 2 > hr * hr
        inside &= (_hash(h * w, seed * 100 + 50 + i) % np.uint64(500) != 0).reshape(h, w)
        m[i, 0] = inside
    return m


G20_IMAGES = {"s512": (1, 1, 512, 512), "s96": (2, 1, 96, 96), "s37x53": (3, 1, 37, 53), "b2_64": (4, 2, 64, 64), "s8x64": (5, 1, 8, 64)}
G20_MASKS = {"holes96": (7, 96, False), "border96": (8, 96, True), "holes512": (9, 512, False), "border512": (10, 512, True)}


def g20_images(name: str):
    """(x, y) uint8 [b, 3, h, w] of the G20 image `name` ("near96": the s96 image and a one-level perturbation of it)."""
    if name == "near96":
        x = g20_images("s96")[0]
        return x, recipe_near(60, x)
    seed, b, h, w = G20_IMAGES[name]
    x = recipe_image(seed, b, h, w)
    return x, recipe_perturb(seed + 100, x, 6)


def g20_mask(name: str) -> np.ndarray:
    seed, size, border = G20_MASKS[name]
    return recipe_mask(seed, 1, size, size, border)


def sha256(a: np.ndarray) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
