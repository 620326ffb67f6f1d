"""The stage-2 image losses (models/image_losses.py) on the GPU: pyramid L2 and (masked) SSIM, forward and closed-form
backward in HIP (csrc/losses.hip, include/iron_train.h), differentiable through iron_amd.autograd.PyramidL2Fn / SSIMFn.

Same public names and signatures as the reference module, so `from models.image_losses import PyramidL2Loss, ssim_loss_fn`
(render_surface.py:24, after iron_amd.install_as_models()) resolves here.  Neither scipy (the pyramid filter) nor kornia (the
erosion of the SSIM mask) is needed: the filter taps are computed in closed form below, the erosion runs in the SSIM kernel.
Inputs are float32 CUDA tensors; there is no CPU path.

`surface_regularisers` is the rest of the stage-2 loss (render_surface.py:580-613, 639: the eikonal and roughness-range terms), which
the reference writes inline; csrc/optim.hip (iron_surface_reg), differentiable through iron_amd.autograd.SurfaceRegFn.

`volume_losses` is the loss of the stage-1 step (render_volume.py:458-496), which the reference writes inline as well;
csrc/volume_loss.hip (iron_volume_loss), differentiable through iron_amd.autograd.VolumeLossFn.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .autograd import PyramidL2Fn, SSIMFn, refuse_grad


def pyramid_taps() -> np.ndarray:
    """The reference's 7x7 pyramid filter, scipy.ndimage.gaussian_filter(dirac7x7, 1.0) in float32, without scipy: the radius-4
    Gaussian of sigma 1 normalised in float64, its tails reflect-folded into the 7 taps (p < 0 -> -p-1, p > 6 -> 13-p), then
    f[i, j] = f32(g[j] * f32(g[i])) -- the two separable passes of scipy, each rounding to float32."""
    x = np.arange(-4, 5, dtype=np.float64)
    phi = np.exp(-0.5 / 1.0 * x ** 2)
    phi = phi / phi.sum()
    g = np.zeros(7, dtype=np.float64)
    for p, v in zip(range(-1, 8), phi):
        g[-p - 1 if p < 0 else (13 - p if p > 6 else p)] += v
    gi = g.astype(np.float32).astype(np.float64)
    return (g[None, :] * gi[:, None]).astype(np.float32)


class PyramidL2Loss(nn.Module):
    """sum_k |d_k|^2 / ((h/2^k)(w/2^k)), d_0 = pred - trgt, d_{k+1} = avgpool2(conv7x7(d_k)), k = 0..4."""

    def __init__(self, use_cuda=True):
        super().__init__()
        gf = pyramid_taps()
        f = np.zeros([3, 3, 7, 7], dtype=np.float32)
        for c in range(3):
            f[c, c] = gf
        self.f = torch.from_numpy(f)  # kept for parity with the reference; the kernels take the taps from the host
        self.use_cuda = use_cuda  # accepted, no effect: the loss always runs on the GPU
        self._taps = (C.c_float * 49)(*gf.reshape(-1).tolist())

    def forward(self, pred_img, trgt_img):
        """pred_img, trgt_img: [B, 3, H, W], H, W >= 16."""
        if pred_img.shape != trgt_img.shape or pred_img.dim() != 4:
            raise _lib.IronError("PyramidL2Loss: pred_img and trgt_img must both be [B, 3, H, W], got %s and %s"
                                 % (tuple(pred_img.shape), tuple(trgt_img.shape)))
        b, c, h, w = pred_img.shape
        if c != 3:
            raise _lib.IronError("PyramidL2Loss: the filter is [3, 3, 7, 7], so C must be 3 (got %d)" % c)
        if h < 16 or w < 16:
            raise _lib.IronError("PyramidL2Loss: H and W must be >= 16 (the fourth 2x2 pooling would be empty), got %dx%d" % (h, w))
        _lib.require_cuda_f32(pred_img, "pred_img")
        _lib.require_cuda_f32(trgt_img, "trgt_img")
        return PyramidL2Fn.apply(pred_img, trgt_img, self._taps)


def _fspecial_gauss_1d(size, sigma):
    r"""1-D Gaussian kernel [1, 1, size], built in float32 on the host exactly as the reference builds it."""
    coords = torch.arange(size, dtype=torch.float)
    coords -= size // 2

    g = torch.exp(-(coords**2) / (2 * sigma**2))
    g /= g.sum()

    return g.unsqueeze(0).unsqueeze(0)


def _host_window(win: torch.Tensor, channels: int):
    """The 1-D taps of a [C, 1, 1, ws] (or [1, 1, ws]) window as a ctypes float array; every channel must use the same taps."""
    w = win.detach().to("cpu", torch.float32).reshape(-1, win.shape[-1])
    if w.shape[0] not in (1, channels) or not bool((w == w[:1]).all()):
        raise _lib.IronError("gaussian_filter: the window must be one 1-D kernel shared by all %d channels, got %s"
                             % (channels, tuple(win.shape)))
    taps = w[0].tolist()
    return (C.c_float * len(taps))(*taps), len(taps)


def _warn_short_axes(shape, ws: int) -> bool:
    short = False
    for i, s in enumerate(shape[2:]):
        if s < ws:
            short = True
            warnings.warn(f"Skipping Gaussian Smoothing at dimension 2+{i} for input: {shape} and win size: {ws}")
    return short


def gaussian_filter(input, win):
    r"""Valid separable blur of a [B, C, H, W] batch with the 1-D kernel `win` ([C, 1, 1, ws]); an axis shorter than the window is
    not smoothed (with the reference's warning).  Inference only: there is no backward through this entry."""
    refuse_grad("gaussian_filter", input, win)
    assert all([ws == 1 for ws in win.shape[1:-1]]), win.shape
    if input.dim() == 5:
        raise _lib.IronError("gaussian_filter: 5-D (conv3d) input is not supported by iron_amd")
    if input.dim() != 4:
        raise NotImplementedError(input.shape)
    b, c, h, w = input.shape
    taps, ws = _host_window(win, c)
    x = _lib.require_cuda_f32(input, "input")
    _warn_short_axes(input.shape, ws)
    ho = h - ws + 1 if h >= ws else h
    wo = w - ws + 1 if w >= ws else w
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=x.device)
    lib = _lib.load_train()
    with torch.cuda.device(x.device):
        _lib.check_train(lib.iron_gaussian_filter(x.data_ptr(), b * c, h, w, taps, ws, out.data_ptr(), _lib.stream_ptr(x.device)))
    return out


def ssim_loss_fn(X, Y, mask=None, data_range=1.0, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    r"""1 - mean SSIM of X and Y ([B, C, H, W]); with `mask` ([B, 1, H, W], bool / uint8 / float) the valid SSIM map is padded by
    win_size // 2 with 1.0 and averaged over the pixels kept by the win_size x win_size erosion of the mask."""
    if not X.shape == Y.shape:
        raise ValueError("Input images should have the same dimensions.")

    if not X.type() == Y.type():
        raise ValueError("Input images should have the same dtype.")

    if len(X.shape) != 4:
        raise ValueError(f"Input images should be 4-d tensors, but got {X.shape}")

    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")

    _lib.require_cuda_f32(X, "X")
    _lib.require_cuda_f32(Y, "Y")
    win = _fspecial_gauss_1d(win_size, win_sigma).reshape(-1).tolist()
    K1, K2 = K
    C1 = (K1 * data_range) ** 2
    C2 = (K2 * data_range) ** 2
    b, c, h, w = X.shape
    short = _warn_short_axes(X.shape, win_size)
    m = None
    if mask is not None:
        if short:
            raise _lib.IronError("ssim_loss_fn: a mask needs both image axes >= win_size (%d), got %dx%d (the reference fails "
                                 "there with a shape mismatch)" % (win_size, h, w))
        if tuple(mask.shape) != (b, 1, h, w):
            raise _lib.IronError("ssim_loss_fn: mask must be [B, 1, H, W] = %s, got %s" % ((b, 1, h, w), tuple(mask.shape)))
        if not mask.is_cuda or mask.device != X.device:
            raise _lib.IronError("ssim_loss_fn: mask must be a CUDA tensor on %s" % X.device)
        m = mask.detach()
        if m.dtype not in (torch.bool, torch.uint8):
            m = m.float()
        m = m.contiguous()
    return SSIMFn.apply(X, Y, m, (C.c_float * win_size)(*win), win_size, float(C1), float(C2))


def surface_regularisers(eik_grad, normal, mask, specular_roughness, edge_pos_neg_normal=None, eik_weight=0.1, roughrange_weight=0.1,
                         return_counts=False):
    r"""The regularisers of the stage-2 step (render_surface.py:580-613, 639) in one forward and one backward launch chain:

        eik_loss        = eik_weight * (sum_uniform + sum_masked + sum_edge of (|g| - 1)^2) / (M + n_mask + E)
        roughrange_loss = roughrange_weight * mean(r - 0.5 over masked r > 0.5), or 0 when no masked value exceeds 0.5

    eik_grad [M, 3]: SDFNetwork.gradient at the uniform points; normal [H, W, 3], mask [H, W] (bool / uint8) and
    specular_roughness ([H, W] from the ggx render_fn, [H, W, 1] from the comp one): the frame; edge_pos_neg_normal [E, 3] or None.
    With an all-false mask only the uniform set counts, as in the reference.  Returns two device scalars attached to eik_grad,
    normal, specular_roughness and edge_pos_neg_normal; return_counts=True adds the device int64 [3] (M + n_mask + E, n_mask,
    number of selected roughness values)."""
    from .autograd import SurfaceRegFn
    if eik_grad.dim() != 2 or eik_grad.shape[-1] != 3:
        raise _lib.IronError("surface_regularisers: eik_grad must be [M, 3], got %s" % (tuple(eik_grad.shape),))
    if normal.dim() < 2 or normal.shape[-1] != 3:
        raise _lib.IronError("surface_regularisers: normal must be [..., 3], got %s" % (tuple(normal.shape),))
    lead = tuple(normal.shape[:-1])
    if tuple(mask.shape) != lead:
        raise _lib.IronError("surface_regularisers: mask must be %s, got %s" % (lead, tuple(mask.shape)))
    if tuple(specular_roughness.shape) not in (lead, lead + (1,)):
        raise _lib.IronError("surface_regularisers: specular_roughness must be %s or %s, got %s"
                             % (lead, lead + (1,), tuple(specular_roughness.shape)))
    if edge_pos_neg_normal is not None and (edge_pos_neg_normal.dim() != 2 or edge_pos_neg_normal.shape[-1] != 3):
        raise _lib.IronError("surface_regularisers: edge_pos_neg_normal must be [E, 3], got %s" % (tuple(edge_pos_neg_normal.shape),))
    if not mask.is_cuda or mask.device != eik_grad.device or mask.dtype not in (torch.bool, torch.uint8):
        raise _lib.IronError("surface_regularisers: mask must be a bool / uint8 CUDA tensor on %s" % eik_grad.device)
    g = _lib.require_cuda_f32(eik_grad, "eik_grad")
    n = _lib.require_cuda_f32(normal, "normal").reshape(-1, 3)
    r = _lib.require_cuda_f32(specular_roughness, "specular_roughness").reshape(-1)
    e = None if edge_pos_neg_normal is None else _lib.require_cuda_f32(edge_pos_neg_normal, "edge_pos_neg_normal")
    for t, name in ((n, "normal"), (r, "specular_roughness"), (e, "edge_pos_neg_normal")):
        if t is not None and t.device != g.device:
            raise _lib.IronError("surface_regularisers: %s must be on %s" % (name, g.device))
    m = mask.detach().contiguous().reshape(-1)
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    eik, rr, counts = SurfaceRegFn.apply(g, n, m, r, e, float(eik_weight), float(roughrange_weight))
    return (eik, rr, counts) if return_counts else (eik, rr)


def volume_losses(color_fine, true_rgb, mask, weight_sum, weight_max, cdf_fine, gradient_error, igr_weight=0.1, mask_weight=0.0):
    r"""The loss of the stage-1 step (render_volume.py:458-496) and the statistics it logs (:507-510) in one forward and one backward
    launch chain (csrc/volume_loss.hip):

        mask  = (raw mask > 0.5) when mask_weight > 0, else 1;   mask_sum = sum mask + 1e-5
        color_fine_loss = sum |(color_fine - true_rgb) mask| / mask_sum
        mask_loss       = binary_cross_entropy(weight_sum.clip(1e-3, 1 - 1e-3), mask)
        loss            = color_fine_loss + igr_weight * gradient_error + mask_weight * mask_loss

    color_fine [B, 3]; true_rgb [B, 3] and the raw mask [B, 1] (or [B]; None with mask_weight = 0) may be slices of the [B, 10] batch
    (only their last dimension must be dense); weight_sum and weight_max [B, 1] or [B]; cdf_fine [B, M] (its first column is
    used); gradient_error: the renderer's 0-d eikonal statistic.  Returns a dictionary of 0-d device tensors: "loss" (the only one
    attached to the graph: gradients go to color_fine, weight_sum and gradient_error), "color_fine_loss", "eikonal_loss",
    "mask_loss", "psnr" (+inf when prediction equals target), "cdf", "weight_max", "mask_sum".  Nothing waits for the host."""
    from .autograd import VolumeLossFn
    if color_fine.dim() != 2 or color_fine.shape[1] != 3 or color_fine.shape[0] < 1:
        raise _lib.IronError("volume_losses: color_fine must be [B >= 1, 3], got %s" % (tuple(color_fine.shape),))
    b = color_fine.shape[0]
    c = _lib.require_cuda_f32(color_fine, "color_fine")
    dev = c.device

    def rows(t, name, width):
        """[B, >= width] float32 on `dev` whose rows are dense (a slice of a wider batch stays where it is)."""
        if not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dtype != torch.float32:
            raise _lib.IronError("volume_losses: %s must be a float32 CUDA tensor on %s" % (name, dev))
        t = t.detach()
        if t.dim() == 1:
            t = t.unsqueeze(-1)
        if t.dim() != 2 or t.shape[0] != b or t.shape[1] < width:
            raise _lib.IronError("volume_losses: %s must be [%d, >= %d], got %s" % (name, b, width, tuple(t.shape)))
        if t.stride(1) != 1 or (b > 1 and t.stride(0) < t.shape[1]):
            t = t.contiguous()
        return t

    def column(t, name):
        if not torch.is_tensor(t) or t.device != dev or t.numel() != b:
            raise _lib.IronError("volume_losses: %s must hold %d values on %s" % (name, b, dev))
        return _lib.require_cuda_f32(t, name).reshape(-1)

    if true_rgb.dim() != 2 or true_rgb.shape[1] != 3:
        raise _lib.IronError("volume_losses: true_rgb must be [B, 3], got %s" % (tuple(true_rgb.shape),))
    t = rows(true_rgb, "true_rgb", 3)
    if mask is None:
        if mask_weight > 0:
            raise _lib.IronError("volume_losses: mask_weight > 0 needs a mask")
        m = None
    else:
        if mask.numel() != b:
            raise _lib.IronError("volume_losses: mask must be [B, 1], got %s" % (tuple(mask.shape),))
        m = rows(mask, "mask", 1)
    cdf = rows(cdf_fine, "cdf_fine", 1)
    if not torch.is_tensor(gradient_error) or gradient_error.numel() != 1 or gradient_error.device != dev:
        raise _lib.IronError("volume_losses: gradient_error must be a device scalar on %s" % dev)
    ge = _lib.require_cuda_f32(gradient_error, "gradient_error").reshape(())
    loss, record = VolumeLossFn.apply(c, t, m, column(weight_sum, "weight_sum"), column(weight_max.detach(), "weight_max"), cdf, ge,
                                      float(igr_weight), float(mask_weight))
    out = {k: record[i] for i, k in enumerate(_lib.VOLUME_LOSS_RECORD)}
    out["loss"] = loss
    return out
