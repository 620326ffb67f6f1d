"""The stage-2 image losses pixel by pixel (csrc/losses.hip): every gradient pixel, pooled border, SSIM tile seam, window size and
mask threshold against the fp64 torch restatement (tests/_loss_oracle.py), bounded by the restatement's own fp32 run on the same
inputs: |got - ref64| <= 4 max(F, 2 ulp32 |ref64|) with F = max over pixels |oracle32 - oracle64| (the CPU side
of the bound is tests/test_image_losses_oracle.py).  The C entries are also called directly, with exactly sized, 0xFF-filled
workspaces in front of a guard pattern.  Every case prints its worst error over F ("ratio" lines, pytest -s)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import _loss_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PYR_SEED, SSIM_SEED = 31, 41
IRON_ERR_WORKSPACE = -5   # include/iron_hip.h: workspace too small
SSIM_DENSE = [(1, 3) + s for s in O.SSIM_SHAPES] + [(1, 1, 27, 43, 11), (1, 4, 27, 43, 11), (2, 3, 27, 43, 11)]
SSIM_UNMASKED = SSIM_DENSE + [(1, 3) + s for s in O.SSIM_PASS_THROUGH]


# ---- running the native losses ------------------------------------------------------------------------------------------------
def _native(kind, x, y, mask=None, win=11, scale=1.0, need=(True, True)):
    from iron_amd.image_losses import PyramidL2Loss, ssim_loss_fn
    x = x.detach().to(DEV).clone().requires_grad_(need[0])
    y = y.detach().to(DEV).clone().requires_grad_(need[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = PyramidL2Loss()(x, y) if kind == "pyr" else ssim_loss_fn(x, y, None if mask is None else mask.to(DEV), win_size=win)
    (scale * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), None if x.grad is None else x.grad.cpu(), None if y.grad is None else y.grad.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _dense(kind, b, c, h, w, win=11, masked=False, scale=1.0):
    """(case, ref64, ref32, F) of a dense pair; computed once per case and shared."""
    x, y = O.case_images(PYR_SEED if kind == "pyr" else SSIM_SEED, b, c, h, w)
    case = dict(kind=kind, x=x, y=y, win=win, scale=scale, mask=O.det_mask(b, h, w) if masked else None)
    return (case,) + O.floors(case)


def _check_loss(name, got, r64, r32):
    """The rule of test_gpu_image_losses.py: 1e-6 relative, or 1.5 x the restatement's own fp32 gap."""
    ref, gap = float(r64["loss"]), abs(float(r32["loss"]) - float(r64["loss"]))
    err, tol = abs(float(got) - ref), max(1e-6 * abs(ref), 1.5 * gap)
    print("ratio %-44s loss  err %.2e tol %.2e (fp32 gap %.2e)" % (name, err, tol, gap))
    assert err <= tol, (name, float(got), ref, tol)


def _check(name, out, got, ref64, F, tile, origin=(0, 0)):
    v = O.judge(got.double().numpy(), ref64, F, O.MARGIN, tile, origin)
    print("ratio %-44s %-5s %.3f of F (F %.2e, %.1e of max|ref|) at %s" % (name, out, v.ratio, F, F / max(float(np.abs(ref64).max()), 1e-300),
                                                                          v.index))
    assert v.ok, (name, out, v)
    return v


# ---- pyramid L2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", O.PYR_SIZES)
def test_pyramid_dense_pair(h, w):
    """Loss, dX and dY at every pixel; dY is -dX bit for bit; an image's dX does not depend on its neighbour in the batch."""
    case, r64, r32, F = _dense("pyr", 2, 3, h, w)
    name = "pyr dense %dx%d" % (h, w)
    loss, dx, dy = _native("pyr", case["x"], case["y"])
    _check_loss(name, loss, r64, r32)
    _check(name, "dx", dx, r64["dx"], F["dx"], O.PYR_TILE)
    _check(name, "dy", dy, r64["dy"], F["dy"], O.PYR_TILE)
    assert _same_bits(dy, -dx)
    for b in range(2):
        _, alone, _ = _native("pyr", case["x"][b:b + 1], case["y"][b:b + 1])
        assert _same_bits(alone[0], dx[b]), b


@pytest.mark.parametrize("h,w", O.PYR_SIZES)
def test_pyramid_impulse_probes(h, w):
    """One impulse at a time on both sides of every tile seam, at the borders and on the rows / columns the floor pooling drops:
    the loss (it moves by 3 - 8 % with the position) and the whole dX, which is exactly zero wherever the restatement's is."""
    pts = O.impulse_points(h, w)
    X = torch.cat([O.impulse(h, w, p)[0] for p in pts])
    Z = torch.zeros_like(X)
    ref = {}
    for dt in (torch.float64, torch.float32):
        xx = X.to(dt).requires_grad_(True)
        per = O.pyramid_l2(xx, Z.to(dt), per_image=True)
        ref[dt] = (per.detach().double().numpy(), torch.autograd.grad(per.sum(), xx)[0].double().numpy())
    worst, worst_loss = None, 0.0
    for i, p in enumerate(pts):
        loss, dx, _ = _native("pyr", X[i:i + 1], Z[i:i + 1], need=(True, False))
        l64, l32 = ref[torch.float64][0][i], ref[torch.float32][0][i]
        err, tol = abs(float(loss) - l64), max(1e-6 * l64, 1.5 * abs(l32 - l64))
        assert err <= tol, (h, w, p, float(loss), l64, tol)
        worst_loss = max(worst_loss, err / tol)
        g64, g32 = ref[torch.float64][1][i], ref[torch.float32][1][i]
        Fp = float(np.abs(g32 - g64).max())
        v = O.judge(dx[0].double().numpy(), g64, Fp, O.MARGIN, O.PYR_TILE)
        assert v.ok, (h, w, p, v)
        assert not bool(dx[0][torch.from_numpy(g64 == 0)].any()), (h, w, p)
        if worst is None or v.ratio > worst[0]:
            worst = (v.ratio, p, v.index)
    print("ratio %-44s dx    %.3f of F, impulse at %s, pixel %s; loss %.3f of its tolerance (%d probes)"
          % ("pyr impulse %dx%d" % (h, w), worst[0], worst[1], worst[2], worst_loss, len(pts)))


@pytest.mark.parametrize("h,w", O.PYR_SIZES)
def test_pyramid_options(h, w):
    """An upstream gradient of -2.5; only X, and only Y, requiring a gradient."""
    case, r64, r32, F = _dense("pyr", 2, 3, h, w, scale=-2.5)
    name = "pyr scale -2.5 %dx%d" % (h, w)
    loss, dx, dy = _native("pyr", case["x"], case["y"], scale=-2.5)
    _check_loss(name, loss, r64, r32)
    _check(name, "dx", dx, r64["dx"], F["dx"], O.PYR_TILE)
    _check(name, "dy", dy, r64["dy"], F["dy"], O.PYR_TILE)
    case, r64, r32, F = _dense("pyr", 2, 3, h, w)
    _, dx, none = _native("pyr", case["x"], case["y"], need=(True, False))
    assert none is None
    _check("pyr only X %dx%d" % (h, w), "dx", dx, r64["dx"], F["dx"], O.PYR_TILE)
    _, none, dy = _native("pyr", case["x"], case["y"], need=(False, True))
    assert none is None
    _check("pyr only Y %dx%d" % (h, w), "dy", dy, r64["dy"], F["dy"], O.PYR_TILE)


# ---- SSIM ---------------------------------------------------------------------------------------------------------------------
def _ssim_name(tag, b, c, h, w, win):
    return "ssim %s %dx%dx%dx%d win %d" % (tag, b, c, h, w, win)


@pytest.mark.parametrize("b,c,h,w,win", SSIM_UNMASKED)
def test_ssim_dense_pair_unmasked(b, c, h, w, win):
    case, r64, r32, F = _dense("ssim", b, c, h, w, win)
    name = _ssim_name("dense", b, c, h, w, win)
    loss, dx, dy = _native("ssim", case["x"], case["y"], None, win)
    _check_loss(name, loss, r64, r32)
    _check(name, "dx", dx, r64["dx"], F["dx"], O.SSIM_TILE)
    _check(name, "dy", dy, r64["dy"], F["dy"], O.SSIM_TILE)


def _reach(mask, win):
    """bool [B, 1, H, W]: the pixels some kept pixel of the valid map has in its window; every other pixel has gradient exactly 0."""
    h, w = mask.shape[-2:]
    kept = (O.keep_map(mask, win) & O.valid_box(h, w, win)).float()
    return torch.nn.functional.max_pool2d(kept, win, stride=1, padding=win // 2) > 0.5


def _check_support(name, grads, ref64, floors, mask, win):
    reach = _reach(mask, win)
    assert bool((~reach).any()) and bool(reach.any()), name
    for g, r, F in zip(grads, ref64, floors):
        out = (~reach).expand_as(g)
        assert not bool(torch.from_numpy(r)[out].any()), name           # the restatement agrees that these are exact zeros
        assert bool((_bits(g)[out] == 0).all()), name                   # +0, not -0 and not a leftover
        # inside the reach the per-pixel bound decides: where x == y under a one-tap window the gradient is a rounding residue
        # (1e-20 in the restatement, 0 or 1e-12 on the device), so zero-ness itself is not comparable there
        big = torch.from_numpy(np.abs(r) > 8.0 * O.MARGIN * F) & reach.expand_as(g)
        assert bool(big.any()) and bool((g[big] != 0).all()), name


@pytest.mark.parametrize("b,c,h,w,win", SSIM_DENSE)
def test_ssim_dense_pair_masked(b, c, h, w, win):
    """All ones with a hole at the centre and the bottom row zero, as bool, as uint8 holding 1, 2 and 255, and as float: the same
    bits; the gradient is exactly +0 outside the reach of the kept valid pixels."""
    case, r64, r32, F = _dense("ssim", b, c, h, w, win, masked=True)
    name = _ssim_name("masked", b, c, h, w, win)
    m = case["mask"]
    u8 = m.to(torch.uint8) * torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.arange(m.numel()) % 3].reshape(m.shape)
    assert set(u8.unique().tolist()) == {0, 1, 2, 255}
    runs = [_native("ssim", case["x"], case["y"], mm, win) for mm in (m, u8, m.float())]
    for other in runs[1:]:
        for a, bb in zip(runs[0], other):
            assert _same_bits(a, bb), name
    loss, dx, dy = runs[0]
    _check_loss(name, loss, r64, r32)
    _check(name, "dx", dx, r64["dx"], F["dx"], O.SSIM_TILE)
    _check(name, "dy", dy, r64["dy"], F["dy"], O.SSIM_TILE)
    _check_support(name, (dx, dy), (r64["dx"], r64["dy"]), (F["dx"], F["dy"]), m, win)


def test_ssim_float_mask_thresholds():
    """0.5, the next float above it, 2.0, -1.0 and NaN in an all-ones float mask: only 0.5, -1.0 and NaN drop their neighbourhood.
    The loss gives the kept count and sum, the gradient's support gives the kept set."""
    h, w, win = 27, 43, 11
    x, y = O.case_images(SSIM_SEED, 1, 3, h, w)
    m = torch.ones(1, 1, h, w)
    for (py, px), v in O.THRESHOLD_PIXELS.items():
        m[0, 0, py, px] = v
    case = dict(kind="ssim", x=x, y=y, win=win, mask=m)
    r64, r32, F = O.floors(case)
    loss, dx, dy = _native("ssim", x, y, m, win)
    _check_loss("ssim float thresholds", loss, r64, r32)
    _check("ssim float thresholds", "dx", dx, r64["dx"], F["dx"], O.SSIM_TILE)
    _check("ssim float thresholds", "dy", dy, r64["dy"], F["dy"], O.SSIM_TILE)
    _check_support("ssim float thresholds", (dx, dy), (r64["dx"], r64["dy"]), (F["dx"], F["dy"]), m, win)
    # each value alone against the all-ones mask: a kept value changes no bit, a dropped one changes the loss
    ones = _native("ssim", x, y, torch.ones(1, 1, h, w), win)
    for (py, px), v in O.THRESHOLD_PIXELS.items():
        one = torch.ones(1, 1, h, w)
        one[0, 0, py, px] = v
        got = _native("ssim", x, y, one, win)
        if v > 0.5:
            assert all(_same_bits(a, b) for a, b in zip(got, ones)), (py, px, v)
        else:
            assert not _same_bits(got[0], ones[0]) and not bool(got[1][0, :, py, px].any()), (py, px, v)


@pytest.mark.parametrize("h,w,win", O.SSIM_SHAPES)
def test_ssim_single_pixel_probes(h, w, win):
    """A mask whose erosion keeps one pixel q of the valid map (and, at the border, band pixels that count 1.0): the loss is
    1 - (n_band + S(q)) / n_kept with S the fp64 SSIM map, dX lives on q's window alone.  q: the corners of the valid map, both
    sides of the 16-row / 32-column tile seams and of the erosion's 32-px seams, one interior pixel."""
    x, y = O.case_images(SSIM_SEED, 1, 3, h, w)
    smap = O.ssim_map(x.double(), y.double(), win)[0, 0]
    rows, worst = [], 0.0
    for q in O.ssim_probe_points(h, w, win):
        m, keep, n_band = O.probe_mask(h, w, win, q)
        r64, r32, F = O.floors(dict(kind="ssim", x=x, y=y, win=win, mask=m))
        want = 1.0 - (n_band + float(smap[q])) / int(keep.sum())
        assert abs(want - float(r64["loss"])) <= 1e-13
        loss, dx, _ = _native("ssim", x, y, m, win, need=(True, False))
        rows.append((q, float(loss), want, abs(float(r32["loss"]) - want)))
        block = torch.zeros(1, 3, h, w, dtype=torch.bool)
        block[:, :, q[0]:q[0] + win, q[1]:q[1] + win] = True
        assert bool((_bits(dx)[~block] == 0).all()), (h, w, win, q)
        sl = (slice(None), slice(None), slice(q[0], q[0] + win), slice(q[1], q[1] + win))
        v = O.judge(dx[sl].double().numpy(), r64["dx"][sl], F["dx"], O.MARGIN, O.SSIM_TILE, origin=(-q[0], -q[1]))
        assert v.ok, (h, w, win, q, v)
        worst = max(worst, v.ratio)
    F_loss = max(r[3] for r in rows)
    worst_loss = 0.0
    for q, got, want, _ in rows:
        v = O.judge(np.float64(got), np.float64(want), F_loss, O.MARGIN)
        assert v.ok, (h, w, win, q, got, want, v)
        worst_loss = max(worst_loss, v.ratio)
    print("ratio %-44s loss  %.3f of its bound (F %.2e), dx %.3f of F (%d probes)" % ("ssim probes %dx%d win %d" % (h, w, win), worst_loss, F_loss,
                                                                                      worst, len(rows)))


def test_ssim_all_false_mask():
    x, y = O.case_images(SSIM_SEED, 1, 3, 26, 42)
    for m in (torch.zeros(1, 1, 26, 42, dtype=torch.bool), torch.zeros(1, 1, 26, 42)):
        loss, dx, dy = _native("ssim", x, y, m, 11)
        assert bool(torch.isnan(loss))
        assert not bool(dx.any()) and not bool(dy.any())


@pytest.mark.parametrize("b,c,h,w,win", SSIM_UNMASKED)
def test_gaussian_filter_per_pixel(b, c, h, w, win):
    from iron_amd.image_losses import _fspecial_gauss_1d, gaussian_filter
    x, _ = O.case_images(SSIM_SEED, b, c, h, w)
    r64, _, F = O.floors(dict(kind="blur", x=x, win=win))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = gaussian_filter(x.to(DEV), _fspecial_gauss_1d(win, 1.5).repeat(c, 1, 1, 1)).cpu()
    assert tuple(got.shape) == r64["out"].shape
    _check("blur %dx%dx%dx%d win %d" % (b, c, h, w, win), "out", got, r64["out"], F["out"], O.SSIM_TILE)


# ---- the C entries, called directly ---------------------------------------------------------------------------------------------
GUARD = 4096


class _Guarded:
    """`nbytes` of 0xFF directly in front of a 4 KiB pattern."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.empty(self.n + GUARD, dtype=torch.uint8, device=DEV)
        self.buf[:self.n] = 0xFF
        self.pattern = (torch.arange(GUARD, device=DEV) % 251).to(torch.uint8)
        self.buf[self.n:] = self.pattern

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return torch.equal(self.buf[self.n:], self.pattern)

    def floats(self, shape):
        return self.buf[:self.n].view(torch.float32).reshape(shape).clone().cpu()


def _entries():
    from iron_amd import _lib
    return _lib, _lib.load_train(), _lib.stream_ptr(DEV)


def _win_taps(win):
    from iron_amd.image_losses import _fspecial_gauss_1d
    return (C.c_float * win)(*_fspecial_gauss_1d(win, 1.5).reshape(-1).tolist())


@pytest.mark.parametrize("h,w", [(17, 31), (66, 130)])
def test_pyramid_entries_with_an_exact_poisoned_workspace(h, w):
    from iron_amd.image_losses import PyramidL2Loss
    _lib, lib, stream = _entries()
    case = _dense("pyr", 2, 3, h, w)[0]
    want = _native("pyr", case["x"], case["y"])
    x, y = case["x"].to(DEV), case["y"].to(DEV)
    taps = PyramidL2Loss()._taps
    nbytes = lib.iron_pyramid_l2_workspace_bytes(6, h, w)
    assert nbytes > 0 and nbytes % 256 == 0
    one = torch.ones(1, device=DEV)
    runs = []
    for _ in range(2):
        ws, loss, dx, dy = _Guarded(nbytes), _Guarded(4), _Guarded(4 * x.numel()), _Guarded(4 * x.numel())
        assert lib.iron_pyramid_l2_forward(x.data_ptr(), y.data_ptr(), 6, h, w, taps, loss.ptr(), ws.ptr(), nbytes, stream) == 0
        assert lib.iron_pyramid_l2_backward(x.data_ptr(), y.data_ptr(), 6, h, w, taps, one.data_ptr(), ws.ptr(), nbytes, dx.ptr(), dy.ptr(),
                                            stream) == 0
        torch.cuda.synchronize()
        assert all(g.intact() for g in (ws, loss, dx, dy))
        runs.append((loss.floats(()), dx.floats(x.shape), dy.floats(x.shape)))
    for got in runs:
        for a, b in zip(got, want):
            assert _same_bits(a, b)      # nothing was read before it was written, and two runs agree
    ws, loss = _Guarded(nbytes), _Guarded(4)
    assert lib.iron_pyramid_l2_forward(x.data_ptr(), y.data_ptr(), 6, h, w, taps, loss.ptr(), ws.ptr(), nbytes - 1, stream) == IRON_ERR_WORKSPACE
    assert lib.iron_pyramid_l2_backward(x.data_ptr(), y.data_ptr(), 6, h, w, taps, one.data_ptr(), ws.ptr(), nbytes - 1, loss.ptr(), None,
                                        stream) == IRON_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws.buf[:nbytes] == 0xFF).all()) and bool((loss.buf[:4] == 0xFF).all())   # nothing was enqueued
    assert lib.iron_pyramid_l2_workspace_bytes(6, 15, 16) == 0
    assert lib.iron_pyramid_l2_forward(x.data_ptr(), y.data_ptr(), 6, 15, 16, taps, loss.ptr(), ws.ptr(), nbytes, stream) == _lib.IRON_ERR_UNSUPPORTED


@pytest.mark.parametrize("b,c,h,w,win,masked", [(1, 3, 27, 43, 11, True), (2, 3, 27, 43, 11, False), (1, 3, 37, 53, 21, True),
                                                (1, 3, 17, 33, 1, True), (1, 3, 8, 45, 11, False)])
def test_ssim_entries_with_exact_poisoned_buffers(b, c, h, w, win, masked):
    _lib, lib, stream = _entries()
    case = _dense("ssim", b, c, h, w, win, masked)[0]
    m = case["mask"]
    want = _native("ssim", case["x"], case["y"], m, win)
    x, y = case["x"].to(DEV), case["y"].to(DEV)
    m8 = None if m is None else m.to(DEV).view(torch.uint8).contiguous()
    taps = _win_taps(win)
    c1, c2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
    state_b, scratch_b = C.c_size_t(0), C.c_size_t(0)
    assert lib.iron_ssim_workspace_bytes(b, c, h, w, win, int(masked), C.byref(state_b), C.byref(scratch_b)) == 0
    state_b, scratch_b = state_b.value, scratch_b.value
    hv, wv = (h - win + 1 if h >= win else h), (w - win + 1 if w >= win else w)
    assert scratch_b == 16 * b * c * hv * wv
    one = torch.ones(1, device=DEV)

    def forward(state, loss, nbytes):
        return lib.iron_ssim_forward(x.data_ptr(), y.data_ptr(), b, c, h, w, taps, win, c1, c2, _lib.ptr(m8), 1 if masked else 0, loss.ptr(),
                                     state.ptr(), nbytes, stream)

    def backward(state, scratch, dx, dy, state_n, scratch_n):
        return lib.iron_ssim_backward(x.data_ptr(), y.data_ptr(), b, c, h, w, taps, win, c1, c2, int(masked), one.data_ptr(), state.ptr(),
                                      state_n, scratch.ptr(), scratch_n, dx.ptr(), dy.ptr(), stream)

    for _ in range(2):
        state, scratch, loss = _Guarded(state_b), _Guarded(scratch_b), _Guarded(4)
        dx, dy = _Guarded(4 * x.numel()), _Guarded(4 * x.numel())
        assert forward(state, loss, state_b) == 0
        assert backward(state, scratch, dx, dy, state_b, scratch_b) == 0
        torch.cuda.synchronize()
        assert all(g.intact() for g in (state, scratch, loss, dx, dy))
        for a, bb in zip((loss.floats(()), dx.floats(x.shape), dy.floats(x.shape)), want):
            assert _same_bits(a, bb)
    fresh, loss = _Guarded(state_b), _Guarded(4)
    assert forward(fresh, loss, state_b - 1) == IRON_ERR_WORKSPACE
    assert backward(state, scratch, dx, dy, state_b - 1, scratch_b) == IRON_ERR_WORKSPACE
    assert backward(state, scratch, dx, dy, state_b, scratch_b - 1) == IRON_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((fresh.buf[:state_b] == 0xFF).all()) and bool((loss.buf[:4] == 0xFF).all())


def test_ssim_entries_refuse_what_they_cannot_run():
    _lib, lib, stream = _entries()
    x = torch.rand(1, 3, 27, 43, device=DEV)
    buf, loss = _Guarded(1 << 16), _Guarded(4)
    sb, tb = C.c_size_t(0), C.c_size_t(0)
    assert lib.iron_ssim_workspace_bytes(1, 3, 27, 43, 23, 0, C.byref(sb), C.byref(tb)) == _lib.IRON_ERR_UNSUPPORTED   # above kMaxWin = 21
    assert lib.iron_ssim_workspace_bytes(1, 3, 27, 43, 10, 0, C.byref(sb), C.byref(tb)) == _lib.IRON_ERR_BAD_ARG
    assert lib.iron_ssim_workspace_bytes(1, 3, 27, 43, 21, 0, C.byref(sb), C.byref(tb)) == 0
    mask = torch.ones(1, 1, 27, 43, dtype=torch.uint8, device=DEV)
    for win, rc in ((23, _lib.IRON_ERR_UNSUPPORTED), (10, _lib.IRON_ERR_BAD_ARG), (0, _lib.IRON_ERR_BAD_ARG), (-3, _lib.IRON_ERR_BAD_ARG)):
        taps = _win_taps(max(win, 1))
        assert lib.iron_ssim_forward(x.data_ptr(), x.data_ptr(), 1, 3, 27, 43, taps, win, 1e-4, 9e-4, None, 0, loss.ptr(), buf.ptr(), buf.n,
                                     stream) == rc, win
        assert lib.iron_gaussian_filter(x.data_ptr(), 3, 27, 43, taps, win, buf.ptr(), stream) == rc, win
    # a mask with an axis shorter than the window: the reference fails there, so do the entries and the Python surface
    taps = _win_taps(11)
    for h, w in ((8, 45), (45, 8)):
        assert lib.iron_ssim_workspace_bytes(1, 3, h, w, 11, 1, C.byref(sb), C.byref(tb)) == _lib.IRON_ERR_UNSUPPORTED
        assert lib.iron_ssim_forward(x.data_ptr(), x.data_ptr(), 1, 3, h, w, taps, 11, 1e-4, 9e-4, mask.data_ptr(), 1, loss.ptr(), buf.ptr(),
                                     buf.n, stream) == _lib.IRON_ERR_UNSUPPORTED
    assert lib.iron_ssim_forward(x.data_ptr(), x.data_ptr(), 1, 3, 27, 43, taps, 11, 1e-4, 9e-4, mask.data_ptr(), 3, loss.ptr(), buf.ptr(),
                                 buf.n, stream) == _lib.IRON_ERR_BAD_ARG          # mask kind: 1 = uint8, 2 = float
    torch.cuda.synchronize()
    assert bool((buf.buf[:buf.n] == 0xFF).all()) and bool((loss.buf[:4] == 0xFF).all()) and buf.intact()
    from iron_amd.image_losses import ssim_loss_fn
    short = torch.rand(1, 3, 45, 8, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(_lib.IronError):
            ssim_loss_fn(short, short, torch.ones(1, 1, 45, 8, dtype=torch.bool, device=DEV))
        with pytest.raises(ValueError):
            ssim_loss_fn(short, short, win_size=10)


@pytest.mark.parametrize("c,h,w,win", [(3, 27, 43, 11), (3, 37, 53, 21), (4, 45, 8, 11)])
def test_gaussian_filter_entry_writes_its_output_and_nothing_else(c, h, w, win):
    from iron_amd.image_losses import _fspecial_gauss_1d, gaussian_filter
    _lib, lib, stream = _entries()
    x = O.case_images(SSIM_SEED, 1, c, h, w)[0].to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = gaussian_filter(x, _fspecial_gauss_1d(win, 1.5).repeat(c, 1, 1, 1)).cpu()
    out = _Guarded(4 * want.numel())
    assert lib.iron_gaussian_filter(x.data_ptr(), c, h, w, _win_taps(win), win, out.ptr(), stream) == 0
    torch.cuda.synchronize()
    assert out.intact() and _same_bits(out.floats(want.shape), want)
