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


def pyramid_l2(pred, trgt, f=None, divisors="real", per_image=False):
    """`divisors="floor"` and `per_image` are for tests/test_image_losses_oracle.py and the per-pixel GPU tests: the first is a
    WRONG restatement (level k divided by its floor-pooled size), the second returns one loss per image of the batch."""
    f = pyramid_filter(pred.dtype, pred.device) if f is None else f.to(pred)
    d = pred - trgt
    h, w = pred.shape[-2:]
    total = (lambda v: v.sum(dim=(1, 2, 3))) if per_image else (lambda v: v.sum())
    loss = total(d.pow(2)) / (h * w)
    for k in range(1, 5):
        d = F.avg_pool2d(F.conv2d(d, f, padding=3), 2)
        s = float(2 ** k)
        loss = loss + total(d.pow(2)) / ((h / s) * (w / s) if divisors == "real" else (h >> k) * (w >> k))
    return loss


def pyramid_l2_grad(pred, trgt, scale=1.0, adjoint="zero"):
    """d(scale * pyramid_l2)/d pred written out as the kernels compute it: g_4 = 2 w_4 d_4, g_k = 2 w_k d_k + conv^T(pool^T g_{k+1});
    the taps are point symmetric, so conv^T is the same zero-padded correlation, and pool^T gives 1/4 to each pixel of a 2x2 block
    and 0 to the row / column the floor dropped.  `adjoint="clamp"` is a WRONG restatement: the dropped row / column is fed from
    the last pooled one."""
    f = pyramid_filter(pred.dtype, pred.device)
    h, w = pred.shape[-2:]
    d = [pred - trgt]
    for k in range(1, 5):
        d.append(F.avg_pool2d(F.conv2d(d[-1], f, padding=3), 2))
    g = (2.0 * scale / ((h / 16.0) * (w / 16.0))) * d[4]
    for k in range(3, -1, -1):
        hk, wk = d[k].shape[-2:]
        up = 0.25 * g.repeat_interleave(2, -2).repeat_interleave(2, -1)
        pad = (0, wk - up.shape[-1], 0, hk - up.shape[-2])
        up = F.pad(up, pad) if adjoint == "zero" else F.pad(up, pad, mode="replicate")
        s = float(2 ** k)
        g = (2.0 * scale / ((h / s) * (w / s))) * d[k] + F.conv2d(up, f, padding=3)
    return g


def gauss_1d(size, sigma) -> torch.Tensor:
    """The reference's _fspecial_gauss_1d: float32, [1, 1, size]."""
    coords = torch.arange(size, dtype=torch.float)
    coords -= size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.unsqueeze(0).unsqueeze(0)


def erosion(mask: torch.Tensor, kernel: torch.Tensor, pad_value=None) -> torch.Tensor:
    """kornia.morphology.erosion(mask, kernel) for a flat all-ones kernel with the default geodesic border: the minimum over
    the in-image part of the window (pixels outside the image never win).  Unfold form, as kornia computes it.  `pad_value=0.0` is
    a WRONG restatement for the tests (out-of-image pixels count as zero)."""
    kh, kw = kernel.shape
    big = torch.finfo(mask.dtype).max if pad_value is None else pad_value
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


def ssim_map(X, Y, win_size=11, data_range=1.0, win_sigma=1.5, K=(0.01, 0.03)):
    """The per-pixel channel-mean SSIM map [B, 1, H', W'] that ssim() averages."""
    win = gauss_1d(win_size, win_sigma).unsqueeze(0).to(X.device, dtype=X.dtype)  # [1, 1, 1, ws]
    C1 = (K[0] * data_range) ** 2
    C2 = (K[1] * data_range) ** 2
    mu1, mu2 = _blur(X, win), _blur(Y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11 = _blur(X * X, win) - mu1_sq
    s22 = _blur(Y * Y, win) - mu2_sq
    s12 = _blur(X * Y, win) - mu1_mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    return (((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs).mean(dim=1, keepdim=True)


def keep_map(mask, win_size, pad_value=None):
    """The pixels ssim() keeps: the win x win erosion of mask.float(), bool [B, 1, H, W]."""
    return erosion(mask.float(), torch.ones(win_size, win_size, device=mask.device), pad_value) > 0.5


def ssim(X, Y, mask=None, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03), band_value=1.0, erode_pad=None):
    """`band_value` and `erode_pad` other than the defaults are WRONG restatements for the tests."""
    m = ssim_map(X, Y, win_size, data_range, win_sigma, K)
    if mask is not None:
        r = win_size // 2
        m = F.pad(m, (r, r, r, r), mode="constant", value=band_value)
        keep = keep_map(mask, win_size, erode_pad)
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


# ---- per-pixel cases (tests/test_image_losses_oracle.py on the CPU, tests/test_gpu_image_loss_pixels.py on the GPU) -------------------
# Shapes sit on the kernels' seams: 32-px pyramid tiles per level, 16x32 SSIM tiles of the valid map, 32-px erosion tiles.

PYR_SIZES = [(16, 16), (17, 31), (35, 33), (66, 130), (64, 64)]
SSIM_SHAPES = [(26, 42, 11), (27, 43, 11), (43, 75, 11), (36, 52, 21), (37, 53, 21), (18, 34, 3), (19, 35, 3), (16, 32, 1), (17, 33, 1),
               (40, 40, 7)]
SSIM_PASS_THROUGH = [(8, 45, 11), (45, 8, 11)]  # unmasked only: one axis shorter than the window
MARGIN = 4.0                                    # over the fp32 oracle's own worst pixel, as for the shading rows
SSIM_TILE, ERODE_TILE, PYR_TILE = (16, 32), (32, 32), (32, 32)
# float-mask values on and around the 0.5 threshold at 27x43, win 11: 0.5, -1 and NaN drop their 11x11 neighbourhood, the rest stays
THRESHOLD_PIXELS = {(3, 5): 0.5, (3, 37): -1.0, (23, 21): float("nan"), (14, 5): float(np.nextafter(np.float32(0.5), np.float32(1.0))),
                    (14, 37): 2.0}


def case_images(seed: int, b: int, c: int, h: int, w: int):
    """(x, y) float32 [b, c, h, w] in [0, 1]: recipe_image planes and their recipe_perturb of +-6 levels."""
    planes = recipe_image(seed, (b * c + 2) // 3, h, w).reshape(-1, h, w)[:b * c].reshape(b, c, h, w)
    xu = np.ascontiguousarray(planes)
    yu = recipe_perturb(seed + 100, xu, 6)
    return torch.from_numpy(xu).float() / 255.0, torch.from_numpy(yu).float() / 255.0


def det_mask(b: int, h: int, w: int) -> torch.Tensor:
    """All ones, a hole at the centre pixel, the bottom row zero: bool [b, 1, h, w]."""
    m = torch.ones(b, 1, h, w, dtype=torch.bool)
    m[:, :, h // 2, w // 2] = False
    m[:, :, h - 1, :] = False
    return m


def valid_box(h: int, w: int, win: int) -> torch.Tensor:
    """bool [h, w]: the pixels of the image that carry a valid-map value (the rest is the border band)."""
    r = win // 2
    v = torch.zeros(h, w, dtype=torch.bool)
    v[r:h - r, r:w - r] = True
    return v


def mask_stats(mask: torch.Tensor, win: int) -> dict:
    """What a mask keeps: the share of the valid map, the kept band pixels, the dropped pixels (all images of the batch)."""
    keep = keep_map(mask, win)
    h, w = mask.shape[-2:]
    v = valid_box(h, w, win)
    return {"valid_kept": float(keep[..., v].sum()) / (mask.shape[0] * int(v.sum())), "band_kept": int(keep[..., ~v].sum()),
            "dropped": int((~keep).sum())}


def probe_mask(h: int, w: int, win: int, q):
    """Ones on the win x win block whose erosion keeps pixel q = (qy, qx) of the valid map.  The geodesic erosion keeps more than the
    centre when the block touches the image border, so this returns (mask bool [1, 1, h, w], kept set bool [h, w], n_band) and
    asserts, from the restated erosion alone, that exactly one kept pixel lies in the valid map: q."""
    r = win // 2
    qy, qx = q
    assert 0 <= qy <= h - win and 0 <= qx <= w - win, (h, w, win, q)
    m = torch.zeros(1, 1, h, w, dtype=torch.bool)
    m[:, :, qy:qy + win, qx:qx + win] = True
    keep = keep_map(m, win)[0, 0]
    v = valid_box(h, w, win)
    inside = (keep & v).nonzero().tolist()
    assert inside == [[qy + r, qx + r]], (h, w, win, q, inside)
    return m, keep, int((keep & ~v).sum())


def ssim_probe_points(h: int, w: int, win: int):
    """Valid-map pixels for the single-pixel probes: the corners, both sides of the 16-row / 32-column tile seams, both sides of
    the erosion's 32-px seams (image rows / columns 31 | 32), one interior pixel."""
    hv, wv, r = h - win + 1, w - win + 1, win // 2
    my, mx = hv // 2, wv // 2
    pts = [(0, 0), (0, wv - 1), (hv - 1, 0), (hv - 1, wv - 1), (my, mx)]
    pts += [(y, mx) for y in (15, 16)] + [(my, x) for x in (31, 32)] + [(15, 31), (16, 32)]
    pts += [(y - r, wv // 3) for y in (31, 32)] + [(hv // 3, x - r) for x in (31, 32)]
    out = []
    for p in pts:
        if 0 <= p[0] < hv and 0 <= p[1] < wv and p not in out:
            out.append(p)
    return out


def impulse(h: int, w: int, p, amp=(0.75, -0.5, 0.3)):
    """(X, Y) float32 [1, 3, h, w] with X - Y a three-channel impulse at p (Y = 0)."""
    x = torch.zeros(1, 3, h, w)
    for c, a in enumerate(amp):
        x[0, c, p[0], p[1]] = a
    return x, torch.zeros(1, 3, h, w)


def impulse_points(h: int, w: int):
    """Rows and columns {0, 1, mid, 31, 32, 63, 64, last - 1, last}, clipped to the image: both sides of every 32-px tile seam of
    level 0 (and, pooled, of the levels under it), the borders, and the rows / columns the floor pooling drops."""
    def axis(n):
        return sorted({v for v in (0, 1, n // 2, 31, 32, 63, 64, n - 2, n - 1) if 0 <= v < n})
    return [(y, x) for y in axis(h) for x in axis(w)]


def evaluate(case: dict, dtype) -> dict:
    """The restatement on one case in `dtype`, as float64 numpy.  case: kind "pyr" | "ssim" | "blur", x, y float32 tensors,
    mask (or None), win, scale (the upstream gradient of the loss)."""
    kind, win = case["kind"], case.get("win", 11)
    x = case["x"].detach().to(dtype).clone()
    if kind == "blur":
        return {"out": _blur(x, gauss_1d(win, 1.5).unsqueeze(0).to(dtype)).double().numpy()}
    x = x.requires_grad_(True)
    y = case["y"].detach().to(dtype).clone().requires_grad_(True)
    loss = pyramid_l2(x, y) if kind == "pyr" else ssim(x, y, case.get("mask"), win_size=win)
    dx, dy = torch.autograd.grad(case.get("scale", 1.0) * loss, (x, y))
    return {"loss": np.float64(loss.detach().double().numpy()), "dx": dx.double().numpy(), "dy": dy.double().numpy()}


def floors(case: dict):
    """(ref64, ref32, F): the fp64 and fp32 runs of the restatement on the same fp32 inputs and, per output, F = the largest
    |fp32 - fp64| over its pixels.  Recomputed wherever the tests run."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r64, r32 = evaluate(case, torch.float64), evaluate(case, torch.float32)
    return r64, r32, {k: float(np.abs(r32[k] - r64[k]).max()) for k in r64}


def ulp32(v) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


class Verdict:
    """ok: every pixel within margin * max(F, 2 ulp32|ref|); ratio, index, where: the worst pixel's error over its bound at
    margin 1, its index, and its place relative to the image border and the nearest tile seam."""

    def __init__(self, ok, ratio, index, where):
        self.ok, self.ratio, self.index, self.where = ok, ratio, index, where

    def __repr__(self):
        return "%s worst %.3g x bound at %s (%s)" % ("ok" if self.ok else "FAIL", self.ratio, self.index, self.where)


def judge(got, ref64, F: float, margin: float, tile=None, origin=(0, 0)) -> Verdict:
    """|got - ref64| <= margin * max(F, 2 ulp32(|ref64|)) at every pixel.  `tile` (rows, columns) and `origin` (the image
    coordinate of tile (0, 0)'s first pixel) only word the report."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = np.maximum(float(F), 2.0 * ulp32(ref))
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    ok = bool((err <= margin * bound).all())
    ratio = err / bound
    flat = int(np.argmax(ratio))
    index = tuple(int(i) for i in np.unravel_index(flat, ref.shape)) if ref.ndim else ()
    where = "scalar"
    if ref.ndim >= 2:
        (y, x), (h, w) = index[-2:], ref.shape[-2:]
        where = "%d px from the top/bottom border, %d px from the left/right border" % (min(y, h - 1 - y), min(x, w - 1 - x))
        if tile is not None:
            ty, tx = (y - origin[0]) % tile[0], (x - origin[1]) % tile[1]
            where += "; row %d of its %d-row tile, column %d of its %d-column tile (seam distance %d, %d)" % (
                ty, tile[0], tx, tile[1], min(ty, tile[0] - 1 - ty), min(tx, tile[1] - 1 - tx))
    return Verdict(ok, float(ratio.reshape(-1)[flat]), index, where)
