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

The second half holds the per-operator references of tests/test_gpu_imgmetrics_kernels.py (csrc/imgmetrics.hip kernel by kernel):
conv_reference (fp64, with the per-element error scale S), conv_split_emulation (a numpy model of k_conv_h2's split-fp16
arithmetic), prepare_reference, ssim_map_direct, tap_reference.  The convolution's per-element contract is
|got - ref| <= C_CONV * EPS32 * S with EPS32 = 2^-24.  The emulation's worst ratio over CONV_CASES against the fp64 reference is
4.418; C_CONV = 8.84 is twice that, measured on the CPU and never on the kernel (for scale: torch's own fp32 CPU conv2d reaches 6.9 on the same cases).
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


def lpips_layer_term(a, b, lin):
    """One layer's term of the distance, [1, 1, 1, 1]: a, b [1, C, h, w] tap maps, lin [C]."""
    na = a / (torch.sqrt((a ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    nb = b / (torch.sqrt((b ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    d = ((na - nb) ** 2 * lin.to(a.dtype).view(1, -1, 1, 1)).sum(dim=1, keepdim=True)
    return d.mean(dim=(2, 3), keepdim=True)


def lpips_from_features(f0, f1, lin_w) -> float:
    total = 0.
    for l in range(5):
        total = total + lpips_layer_term(f0[l], f1[l], lin_w[l])
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


# ---- per-operator references (tests/test_gpu_imgmetrics_kernels.py; DESIGN.md §14, "Operator by operator") ----------------------
EPS32 = 2.0 ** -24   # fp32's unit roundoff: the unit of the convolution's per-element bound
# (B, H, W, Cin, Cout, ksize, stride, pad) and the branch of k_conv_h2 each one is there for
CONV_CASES = (
    (1, 7, 9, 3, 5, 3, 1, 1),       # slow gather, K = 27 < one k-tile and K % 4 != 0 (scalar weight fetch), Cout 5, M = 63 < 128
    (2, 8, 8, 4, 64, 3, 1, 1),      # K = 36: the vector weight fetch with a guarded last chunk; M = 128 exactly
    (1, 3, 43, 32, 64, 1, 1, 0),    # FAST, ksize 1, K = 32 (one k-tile, no prefetch), M = 129
    (1, 13, 11, 32, 70, 3, 2, 0),   # FAST, Cout 70 (a second column block of 6), stride 2, no padding
    (3, 9, 10, 64, 33, 5, 1, 4),    # FAST, B = 3, pad = ksize - 1, M = 546: two image boundaries inside row tiles
    (2, 31, 31, 3, 64, 11, 4, 2),   # AlexNet's conv1 at the smallest legal image
    (1, 5, 40, 96, 192, 1, 1, 0),   # FAST, Cin 96, M = 200
    (1, 6, 6, 12, 8, 1, 3, 0),      # slow gather at Cin 12, K = 12, stride > ksize, M = 4
    (2, 12, 12, 5, 130, 4, 3, 3),   # an even ksize, Cout 130: three column blocks, the last of 2
    (1, 6, 7, 384, 65, 3, 1, 1),    # K = 3456: the longest accumulation in use; Cout 65
)
# |got - ref| <= C_CONV * EPS32 * S per output element, S = conv(|x|, |w|) + |b|.  C_CONV is twice the worst ratio of
# conv_split_emulation against conv_reference over CONV_CASES (the house rule of _hashgrid_oracle.K): the emulation's figure is
# 4.418 (the ninth case, K = 80), measured on the CPU by tests/test_imgmetrics_oracle.py::test_conv_emulation_sets_c_conv, which
# fails once the constant is less than twice or more than four times that figure.  It is never taken from what the kernel gives.
C_CONV = 8.84


def conv_case(i: int):
    """(x [B,H,W,Cin], w [Cout,k,k,Cin], b [Cout]) of CONV_CASES[i], fp32 numpy.  Activations are ReLU-like (a normal clipped below at
    -0.3) times a per-pixel scale from {1e-3, 1, 30}, so patches mix magnitudes and small values' high pieces are fp16 subnormals;
    weights are He-scaled, biases 0.05 sigma."""
    B, H, W, Cin, Cout, ks, _, _ = CONV_CASES[i]
    rng = np.random.default_rng(100 + i)
    x = np.maximum(rng.standard_normal((B, H, W, Cin)), -0.3).astype(np.float32) * rng.choice([1e-3, 1.0, 30.0], size=(B, H, W, 1)).astype(np.float32)
    w = (rng.standard_normal((Cout, ks, ks, Cin)) * np.sqrt(2.0 / (Cin * ks * ks))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.05).astype(np.float32)
    return x, w, b


def conv_reference(x, w, b, ksize, stride, pad):
    """x [B,H,W,Cin], w [Cout,k,k,Cin], b [Cout] (fp32 arrays or tensors) -> (relu(conv(x, w) + b), S), fp64 tensors [B,Ho,Wo,Cout],
    with S = conv(|x|, |w|) + |b| the scale of each element's rounding error.  ReLU is 1-Lipschitz, so the bound C eps S on the
    pre-activation holds after it and no output is left out near the kink."""
    xt = torch.as_tensor(x).double().permute(0, 3, 1, 2)
    wt = torch.as_tensor(w).double().permute(0, 3, 1, 2)
    bt = torch.as_tensor(b).double()
    assert wt.shape[2] == ksize and wt.shape[3] == ksize and wt.shape[1] == xt.shape[1]
    y = F.relu(F.conv2d(xt, wt, bt, stride=stride, padding=pad))
    S = F.conv2d(xt.abs(), wt.abs(), bt.abs(), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous(), S.permute(0, 2, 3, 1).contiguous()


def _split_h2(v):
    """fp32 -> the fp16 pieces of cv_split8 as fp64 arrays: hi = fp16(v), lo = fp16((v - f32(hi)) * 2048)."""
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def conv_split_emulation(x, w, b, ksize, stride, pad):
    """k_conv_h2's arithmetic in numpy -> fp32 [B,Ho,Wo,Cout].  Patches in (ky, kx, c) order (zero padding, K padded with zeros to a
    multiple of 16: a padded k-step adds exact zeros), both operands split into fp16 pieces, and per 16-wide k-step the three MFMA
    products in the kernel's order (hi*lo and lo*hi into acc_lo, hi*hi into acc_hi), each an exact block product (fp64 holds a sum
    of sixteen 22-bit products) rounded once into its fp32 accumulator; then fma(acc_lo, 1/2048, acc_hi), + bias, ReLU."""
    x, w, b = np.asarray(x, np.float32), np.asarray(w, np.float32), np.asarray(b, np.float32)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    A = np.stack([xp[:, i * stride:i * stride + ksize, j * stride:j * stride + ksize, :].reshape(B, -1)
                  for i in range(Ho) for j in range(Wo)], axis=1).reshape(B * Ho * Wo, -1)
    Wm = w.reshape(Cout, -1)
    K = A.shape[1]
    Kp = -(-K // 16) * 16
    A, Wm = np.pad(A, ((0, 0), (0, Kp - K))), np.pad(Wm, ((0, 0), (0, Kp - K)))
    ah, al = _split_h2(A)
    bh, bl = _split_h2(Wm)
    acc_hi = np.zeros((A.shape[0], Cout), np.float32)
    acc_lo = np.zeros_like(acc_hi)
    for k in range(0, Kp, 16):
        s = slice(k, k + 16)
        acc_lo = (acc_lo.astype(np.float64) + ah[:, s] @ bl[:, s].T).astype(np.float32)
        acc_hi = (acc_hi.astype(np.float64) + ah[:, s] @ bh[:, s].T).astype(np.float32)
        acc_lo = (acc_lo.astype(np.float64) + al[:, s] @ bh[:, s].T).astype(np.float32)
    r = (acc_lo.astype(np.float64) / 2048.0 + acc_hi.astype(np.float64)).astype(np.float32)   # the fma: one rounding
    return np.maximum(r + b[None], np.float32(0.0)).reshape(B, Ho, Wo, Cout)


def conv_ratio(got, ref, S) -> float:
    """max over the elements of |got - ref| / (EPS32 S)."""
    got, ref, S = (np.asarray(t, dtype=np.float64) for t in (got, ref, S))
    return float((np.abs(got - ref) / (EPS32 * S)).max())


def prepare_reference(img):
    """[H,W,3] uint8 or fp32 -> iron_lpips_prepare's fp32 arithmetic, one rounding per operation: v = float32(k) / 255 for uint8,
    then ((2 v - 1) - shift) / scale (2 v is exact)."""
    img = np.asarray(img)
    v = img.astype(np.float32) / np.float32(255.0) if img.dtype == np.uint8 else img.astype(np.float32)
    return ((v * np.float32(2.0) - np.float32(1.0)) - np.array(SHIFT, np.float32)) / np.array(SCALE, np.float32)


def ssim_map_direct(x, y):
    """S of one channel pair [H, W] in fp64 from the definition: every 11 x 11 window summed on its own (no running sum, unlike
    uniform_filter, so independent of ssim_map), [H - 10, W - 10]."""
    from numpy.lib.stride_tricks import sliding_window_view
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    wx, wy = sliding_window_view(x, (11, 11)), sliding_window_view(y, (11, 11))
    ux, uy = wx.sum(axis=(2, 3)) / 121., wy.sum(axis=(2, 3)) / 121.
    vx = (wx * wx).sum(axis=(2, 3)) / 121. - ux * ux
    vy = (wy * wy).sum(axis=(2, 3)) / 121. - uy * uy
    vxy = (wx * wy).sum(axis=(2, 3)) / 121. - ux * uy
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))


TAP_PARTIALS = 1024   # k_lpips_tap: 256 workgroups of four waves, one partial per wave


def tap_reference(feat, lin):
    """feat [2, HW, C], lin [C] -> (d [HW], partials [1024], Sd [1024]), fp64: d[p] = sum_c lin[c] (f0 / (|f0| + 1e-10) -
    f1 / (|f1| + 1e-10))^2 at pixel p, partials[w] = d[w] + d[w + 1024] + ... in that order (wave w's pixels), and Sd the same
    sums with |lin|: the scale of a partial's rounding error when lin is signed."""
    f = np.asarray(feat, np.float64)
    lin = np.asarray(lin, np.float64)
    n = f / (np.sqrt((f * f).sum(axis=2, keepdims=True)) + 1e-10)
    t = (n[0] - n[1]) ** 2
    d, da = (t * lin).sum(axis=1), (t * np.abs(lin)).sum(axis=1)
    partials, Sd = np.zeros(TAP_PARTIALS), np.zeros(TAP_PARTIALS)
    for p in range(len(d)):
        partials[p % TAP_PARTIALS] += d[p]
        Sd[p % TAP_PARTIALS] += da[p]
    return d, partials, Sd
