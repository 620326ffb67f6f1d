"""PSNR, skimage's uniform-window SSIM and LPIPS-AlexNet on the HIP kernels (csrc/imgmetrics.hip): the three numbers of
evaluation/eval_image_folder.py without skimage, imageio, lpips or torchvision.

Conventions (include/iron_hip.h, iron_img_* / iron_lpips_* block): images are [H, W, 3] CUDA tensors, a pair is both uint8 (what the
command reads from disk; means k / 255) or both float32 in [0, 1].  `skimage_ssim` is the SSIM of the evaluation script -- a uniform
11 x 11 window, population covariance, a border of 5 pixels cropped -- and NOT the training loss's Gaussian-window SSIM
(iron_amd.image_losses.ssim_loss_fn).  LPIPS takes its weights from the caller (`LPIPS.from_files`, `LPIPS.from_state`): nothing is
downloaded and nothing is guessed.  There is no CPU path: CPU tensors are refused.  Every result is bitwise reproducible.

Each metric comes as a function returning a Python float (one host wait) and a `*_device` variant returning a device scalar.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _args, _lib

# AlexNet's feature stack as LPIPS (net='alex', v0.1) taps it: (Cin, Cout, kernel, stride, padding), the index of the convolution in
# torchvision's `features` Sequential, and whether a 3x3/2 max-pool follows the tap
ALEX_LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
ALEX_FEATURE_INDEX = (0, 3, 6, 8, 10)
ALEX_POOL_AFTER = (True, True, False, False, False)
MIN_LPIPS_SIDE = 31  # 31 -> conv1 7 -> pool 3 -> pool 1


def _pair(pred, trgt, what: str):
    for name, x in (("pred", pred), ("trgt", trgt)):
        if not isinstance(x, torch.Tensor):
            raise _lib.IronError("%s: %s must be a CUDA tensor, got %s" % (what, name, type(x).__name__))
        if not x.is_cuda:
            raise _lib.IronError("%s: CPU tensors are not accepted (iron_amd has no CPU path); %s is on the CPU" % (what, name))
    if pred.dim() != 3 or pred.shape[2] != 3 or pred.shape != trgt.shape:
        raise _lib.IronError("%s: images must be two [H, W, 3] tensors of one size, got %s and %s" % (what, tuple(pred.shape), tuple(trgt.shape)))
    if pred.dtype != trgt.dtype or pred.dtype not in (torch.uint8, torch.float32):
        raise _lib.IronError("%s: images must be both uint8 or both float32, got %s and %s" % (what, pred.dtype, trgt.dtype))
    if pred.device != trgt.device:
        raise _lib.IronError("%s: images are on different devices" % what)
    return pred.detach().contiguous(), trgt.detach().contiguous(), int(pred.dtype == torch.float32)


# ---- squared error / PSNR -------------------------------------------------------------------------------------------------------
def squared_error_device(pred, trgt) -> torch.Tensor:
    """fp64 device tensor [2]: the sum of (pred - trgt)^2 over all pixels and channels (in the units of images in [0, 1]) and the
    element count."""
    a, b, is_f32 = _pair(pred, trgt, "psnr")
    lib = _lib.load()
    n = a.numel()
    with torch.cuda.device(a.device):
        ws = _args.sized_workspace(lib.iron_img_sqerr_workspace_bytes, n, device=a.device, tag="img_sqerr")
        out = torch.empty(2, dtype=torch.float64, device=a.device)
        _lib.check(lib.iron_img_sqerr(a.data_ptr(), b.data_ptr(), n, is_f32, ws.data_ptr(), out.data_ptr(), _lib.stream_ptr(a.device)))
    return out


def mse2psnr(mse: float) -> float:
    """evaluation/eval_image_folder.py:22."""
    return -10.0 * math.log(mse + 1e-10) / math.log(10.0)


def psnr_device(pred, trgt) -> torch.Tensor:
    s = squared_error_device(pred, trgt)
    return -10.0 * torch.log(s[0] / s[1] + 1e-10) / math.log(10.0)


def psnr(pred, trgt) -> float:
    """-10 log10(mean((pred - trgt)^2) + 1e-10) of two [H, W, 3] images."""
    s = squared_error_device(pred, trgt).cpu()
    return mse2psnr(float(s[0]) / float(s[1]))


# ---- SSIM -----------------------------------------------------------------------------------------------------------------------
def _ssim_sums(pred, trgt, want_map: bool):
    a, b, is_f32 = _pair(pred, trgt, "skimage_ssim")
    H, W = int(a.shape[0]), int(a.shape[1])
    if H < 11 or W < 11:
        raise _lib.IronError("skimage_ssim: win_size 11 exceeds the image extent %d x %d" % (H, W))
    lib = _lib.load()
    with torch.cuda.device(a.device):
        ws = _args.sized_workspace(lib.iron_img_ssim_workspace_bytes, H, W, device=a.device, tag="img_ssim")
        sums = torch.empty(3, dtype=torch.float64, device=a.device)
        smap = torch.empty((3, H - 10, W - 10), dtype=torch.float64, device=a.device) if want_map else None
        # skimage_ssim(pred, trgt) calls structural_similarity(trgt, pred); S is symmetric in its arguments term by term
        _lib.check(lib.iron_img_ssim(b.data_ptr(), a.data_ptr(), H, W, is_f32, ws.data_ptr(), sums.data_ptr(), _lib.ptr(smap),
                                     _lib.stream_ptr(a.device)))
    return sums, smap, (H - 10) * (W - 10)


def skimage_ssim_device(pred, trgt) -> torch.Tensor:
    sums, _, n = _ssim_sums(pred, trgt, False)
    return (sums / n).sum() / 3.0


def skimage_ssim(pred, trgt) -> float:
    """skimage_ssim of evaluation/eval_image_folder.py:10-17: the mean over the three channels of skimage's structural_similarity
    with data_range=1, win_size=11, use_sample_covariance=False (uniform window; the script's sigma / k1 / k2 are inert)."""
    sums, _, n = _ssim_sums(pred, trgt, False)
    s = sums.cpu()
    return (float(s[0]) / n + float(s[1]) / n + float(s[2]) / n) / 3.0


def skimage_ssim_map(pred, trgt) -> torch.Tensor:
    """The S map, fp64 [3, H - 10, W - 10] (skimage's full=True map with its border of 5 pixels cropped)."""
    return _ssim_sums(pred, trgt, True)[1]


# ---- LPIPS ----------------------------------------------------------------------------------------------------------------------
def _need(sd, key, shape, src):
    if not isinstance(sd, dict):
        raise _lib.IronError("%s does not hold a state dict (got %s)" % (src, type(sd).__name__))
    if key not in sd:
        raise _lib.IronError("%s: key '%s' is missing; keys found: %s" % (src, key, sorted(str(k) for k in sd.keys())))
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise _lib.IronError("%s: key '%s' must have shape %s, got %s" % (src, key, tuple(shape), got))
    if not t.is_floating_point() or not bool(torch.isfinite(t).all()):
        raise _lib.IronError("%s: key '%s' must hold finite floating-point values" % (src, key))
    return t.detach().to("cpu", torch.float32)


def load_lpips_state(alexnet_pth, lin_pth):
    """Read torchvision's AlexNet checkpoint (`features.{0,3,6,8,10}.{weight,bias}`) and the lpips package's weights/v0.1/alex.pth
    (`lin{0..4}.model.1.weight`, [1, C, 1, 1]) -> (conv_w, conv_b, lin_w), lists of five CPU fp32 tensors.  A missing or misshaped
    key raises IronError naming it and the keys that were found; nothing is guessed."""
    alex = torch.load(alexnet_pth, map_location="cpu", weights_only=True)
    lin = torch.load(lin_pth, map_location="cpu", weights_only=True)
    conv_w, conv_b, lin_w = [], [], []
    for l, ((cin, cout, k, _, _), idx) in enumerate(zip(ALEX_LAYERS, ALEX_FEATURE_INDEX)):
        conv_w.append(_need(alex, "features.%d.weight" % idx, (cout, cin, k, k), str(alexnet_pth)))
        conv_b.append(_need(alex, "features.%d.bias" % idx, (cout,), str(alexnet_pth)))
        lin_w.append(_need(lin, "lin%d.model.1.weight" % l, (1, cout, 1, 1), str(lin_pth)))
    return conv_w, conv_b, lin_w


class LPIPS:
    """lpips.LPIPS(net='alex') (version 0.1, lpips=True, spatial=False, eval mode), forward only.  `lp(pred, trgt)` takes [H, W, 3]
    images in [0, 1] (uint8 or fp32 CUDA tensors; the 2 x - 1 and the scaling layer are inside) and returns a Python float."""

    def __init__(self, conv_w, conv_b, lin_w, device=None):
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.IronError("LPIPS needs a GPU (iron_amd has no CPU path)")
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.IronError("LPIPS: the device must be a GPU, got %s" % device)
        if len(conv_w) != 5 or len(conv_b) != 5 or len(lin_w) != 5:
            raise _lib.IronError("LPIPS: five convolution weights, five biases and five lin weights are needed")
        self.device = device
        self.conv_w, self.conv_b, self.lin_w = [], [], []
        for l, (cin, cout, k, _, _) in enumerate(ALEX_LAYERS):
            sd = {"conv_w[%d]" % l: conv_w[l], "conv_b[%d]" % l: conv_b[l], "lin_w[%d]" % l: lin_w[l]}
            lin = sd["lin_w[%d]" % l]
            if isinstance(lin, torch.Tensor) and lin.dim() == 4:
                sd["lin_w[%d]" % l] = lin.reshape(-1) if tuple(lin.shape) == (1, cout, 1, 1) else lin
            w = _need(sd, "conv_w[%d]" % l, (cout, cin, k, k), "LPIPS.from_state")
            b = _need(sd, "conv_b[%d]" % l, (cout,), "LPIPS.from_state")
            v = _need(sd, "lin_w[%d]" % l, (cout,), "LPIPS.from_state")
            # the kernels' weight layout: [Cout, ky, kx, Cin], the k order of an NHWC patch
            self.conv_w.append(w.permute(0, 2, 3, 1).contiguous().to(device))
            self.conv_b.append(b.contiguous().to(device))
            self.lin_w.append(v.contiguous().to(device))
        self._weights = _lib.iron_lpips_weights()
        for l in range(5):
            self._weights.conv_weight[l] = self.conv_w[l].data_ptr()
            self._weights.conv_bias[l] = self.conv_b[l].data_ptr()
            self._weights.lin[l] = self.lin_w[l].data_ptr()

    @classmethod
    def from_state(cls, conv_w, conv_b, lin_w, device=None):
        """conv_w[l] [Cout, Cin, k, k], conv_b[l] [Cout], lin_w[l] [Cout] or [1, Cout, 1, 1] (any device; copied to `device`)."""
        return cls(conv_w, conv_b, lin_w, device=device)

    @classmethod
    def from_files(cls, alexnet_pth, lin_pth, device=None):
        return cls(*load_lpips_state(alexnet_pth, lin_pth), device=device)

    def _images(self, pred, trgt):
        a, b, is_f32 = _pair(pred, trgt, "LPIPS")
        if a.device != self.device:
            raise _lib.IronError("LPIPS: the images are on %s, the weights on %s" % (a.device, self.device))
        H, W = int(a.shape[0]), int(a.shape[1])
        if H < MIN_LPIPS_SIDE or W < MIN_LPIPS_SIDE:
            raise _lib.IronError("LPIPS: the AlexNet stack needs images of at least %d x %d, got %d x %d" % (MIN_LPIPS_SIDE, MIN_LPIPS_SIDE, H, W))
        return a, b, is_f32, H, W

    def lpips_device(self, pred, trgt) -> torch.Tensor:
        """fp64 device tensor [2]: the LPIPS distance and a flag (1.0 if an operand left fp16 range; the distance is then NaN)."""
        a, b, is_f32, H, W = self._images(pred, trgt)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            ws = _args.sized_workspace(lib.iron_lpips_workspace_bytes, H, W, device=self.device, tag="lpips")
            out = torch.empty(2, dtype=torch.float64, device=self.device)
            _lib.check(lib.iron_lpips_forward(a.data_ptr(), b.data_ptr(), H, W, is_f32, C.byref(self._weights), ws.data_ptr(), out.data_ptr(),
                                              _lib.stream_ptr(self.device)))
        return out

    def __call__(self, pred, trgt) -> float:
        return lpips_value(self.lpips_device(pred, trgt).cpu())

    def run_staged(self, pred, trgt, stage=None):
        """The forward pass one library call at a time (what lpips_device enqueues in one): returns (taps, out) with taps[l] the
        l-th tap map [2, Hl, Wl, Cl] (image 0 = pred) and out as lpips_device.  `stage(name, fn)` wraps every call
        (tools/bench_imgmetrics.py times them); by default it just calls fn."""
        a, b, is_f32, H, W = self._images(pred, trgt)
        lib = _lib.load()
        run = stage if stage is not None else (lambda name, fn: fn())
        dev = self.device
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            x = torch.empty((2, H, W, 3), dtype=torch.float32, device=dev)
            run("prepare", lambda: _lib.check(lib.iron_lpips_prepare(a.data_ptr(), b.data_ptr(), H, W, is_f32, x.data_ptr(), st)))
            partials = torch.empty((5, 1024), dtype=torch.float64, device=dev)
            taps = []
            for l, (cin, cout, k, s, p) in enumerate(ALEX_LAYERS):
                h, w = int(x.shape[1]), int(x.shape[2])
                ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
                y = torch.empty((2, ho, wo, cout), dtype=torch.float32, device=dev)
                run("conv%d" % (l + 1), lambda x=x, y=y, h=h, w=w: _lib.check(lib.iron_conv2d_relu(
                    x.data_ptr(), 2, h, w, cin, self.conv_w[l].data_ptr(), self.conv_b[l].data_ptr(), cout, k, s, p, y.data_ptr(),
                    flag.data_ptr(), st)))
                run("tap%d" % (l + 1), lambda y=y: _lib.check(lib.iron_lpips_tap(y.data_ptr(), ho, wo, cout, self.lin_w[l].data_ptr(),
                                                                                  partials[l].data_ptr(), st)))
                taps.append(y)
                x = y
                if ALEX_POOL_AFTER[l]:
                    z = torch.empty((2, (ho - 3) // 2 + 1, (wo - 3) // 2 + 1, cout), dtype=torch.float32, device=dev)
                    run("pool%d" % (l + 1), lambda y=y, z=z: _lib.check(lib.iron_maxpool3s2(y.data_ptr(), 2, ho, wo, cout, z.data_ptr(), st)))
                    x = z
            inv_hw = torch.tensor([1.0 / (t.shape[1] * t.shape[2]) for t in taps], dtype=torch.float64, device=dev)
            bad = (flag[0] != 0)
            value = (partials.sum(dim=1) * inv_hw).sum()
            out = torch.stack([torch.where(bad, torch.full_like(value, float("nan")), value), bad.double()])
        return taps, out

    def features(self, img):
        """The five tap maps (after the ReLU) of one [H, W, 3] image, fp32 device tensors [C, Hl, Wl]."""
        taps, out = self.run_staged(img, img)
        lpips_value(out.cpu())  # raises on a range violation
        return [t[0].permute(2, 0, 1).contiguous() for t in taps]


def lpips_value(out_cpu) -> float:
    """The Python float of an LPIPS device result [value, flag] already copied to the host; raises the range error if flagged."""
    if float(out_cpu[1]) != 0.0:
        raise _lib.IronError("libiron_hip: range error (IRON_ERR_RANGE): an LPIPS convolution operand (weight or activation) left "
                             "fp16's range (|x| > 65504 or non-finite); the split-fp16 product has no value for it")
    return float(out_cpu[0])


# ---- the pair and the table of evaluation/eval_image_folder.py -----------------------------------------------------------------
def _upload_u8(x, name):
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise _lib.IronError("evaluate_pair: CPU tensors are not accepted (iron_amd has no CPU path); pass numpy arrays or CUDA tensors")
        t = x
    else:
        x = np.ascontiguousarray(x)
        if x.dtype != np.uint8:
            raise _lib.IronError("evaluate_pair: %s must be uint8, got %s" % (name, x.dtype))
        if not torch.cuda.is_available():
            raise _lib.IronError("evaluate_pair needs a GPU (iron_amd has no CPU path)")
        t = torch.from_numpy(x).cuda()
    if t.dtype != torch.uint8:
        raise _lib.IronError("evaluate_pair: %s must be uint8, got %s" % (name, t.dtype))
    return t


def evaluate_pair(pred_u8, trgt_u8, lpips=None):
    """(psnr, ssim, lpips) of one 8-bit [H, W, 3] pair (numpy arrays or CUDA tensors) as the evaluation script computes them; the
    LPIPS entry is NaN when no `lpips` object is given.  One host wait."""
    a, b = _upload_u8(pred_u8, "pred"), _upload_u8(trgt_u8, "trgt")
    sq = squared_error_device(a, b)
    sums, _, n = _ssim_sums(a, b, False)
    # the script scores loss_fn_alex(trgt, pred); the distance is symmetric, the argument order is kept anyway
    lp = lpips.lpips_device(b, a) if lpips is not None else torch.tensor([float("nan"), 0.0], dtype=torch.float64, device=a.device)
    host = torch.cat([sq, sums, lp]).cpu()
    d = lpips_value(host[5:7])
    ssim = (float(host[2]) / n + float(host[3]) / n + float(host[4]) / n) / 3.0
    return mse2psnr(float(host[0]) / float(host[1])), ssim, d


def format_metrics(rows) -> str:
    """The text of metrics.txt (evaluation/eval_image_folder.py:36-63) for rows of (img_name, psnr, ssim, lpips)."""
    rows = list(rows)
    text = 'img_name\tpsnr\tssim\tlpips\n'
    for name, p, s, d in rows:
        text += '{}\t{:.3f}\t{:.3f}\t{:.4f}\n'.format(name, p, s, d)
    mean = [float(np.mean([r[i] for r in rows])) if rows else float("nan") for i in (1, 2, 3)]
    text += '\nAverage\t{:.3f}\t{:.3f}\t{:.4f}\n'.format(*mean)
    return text
