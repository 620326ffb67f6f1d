"""GPU: csrc/imgmetrics.hip kernel by kernel, through the C entries, against the fp64 references of tests/_imgmetrics_oracle.py
("Operator by operator").  tests/test_gpu_imgmetrics.py pins the metrics end to end; this file pins each operator at
the shapes where a tile edge, a guard or a second code path decides the result.

  iron_conv2d_relu    per output element |got - ref| <= C_CONV * EPS32 * S, S = conv(|x|, |w|) + |b| (C_CONV: twice the numpy
                      emulation's worst ratio, see the oracle); the range flag; refusals; rows independent of the batch
  iron_maxpool3s2     equal to torch's CPU max_pool2d, and blind to the row / column no window reaches
  iron_lpips_tap      all 1024 per-wave partials within 1e-12 * Sd of the fp64 sums in the kernel's pixel order (fp64 with at most
                      ~400 additions per partial is 4e-14 Sd: a margin of 25)
  iron_lpips_prepare  bitwise equal to numpy's fp32 ((2 v - 1) - shift) / scale: every operation is one fp32 rounding
  iron_img_ssim       the S map per pixel within 1e-11 of direct fp64 window sums (the bound of test_ssim_map_uint8) with H - 10 and
                      W - 10 on, one short of and one past the 16 x 32 tile; sums against the map's own total

Every output buffer has 64 elements of NaN behind it (and is NaN before the call): nothing may be written past the end, and every
element must be written.  Every figure is printed before it is asserted."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import _imgmetrics_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 64
IRON_OK, IRON_ERR_BAD_ARG = 0, -1


def lib():
    from iron_amd import _lib
    return _lib.load()


def stream():
    from iron_amd import _lib
    return _lib.stream_ptr(DEV)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype=torch.float32):
    """(buffer, view): a NaN-filled torch buffer of prod(shape) + GUARD elements and its leading part as `shape`."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[:n].view(*shape)


def guard_intact(buf):
    return bool(torch.isnan(buf[-GUARD:]).all())


def same_bits(a, b):
    view = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@functools.lru_cache(maxsize=None)
def photo():
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, "g22_eval_photo.png")).convert("RGB"), dtype=np.uint8)


# ---- iron_conv2d_relu -------------------------------------------------------------------------------------------------------------
def out_hw(H, W, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def run_conv(x, w, b, ks, stride, pad, flag0=0, finite=True):
    """-> (out [B,Ho,Wo,Cout] on the CPU, the range flag after the call)."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    tx, tw, tb = up(x), up(w), up(b)
    buf, out = guarded((B, Ho, Wo, Cout))
    flag = torch.full((1,), flag0, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib().iron_conv2d_relu(tx.data_ptr(), B, H, W, Cin, tw.data_ptr(), tb.data_ptr(), Cout, ks, stride, pad, out.data_ptr(),
                                    flag.data_ptr(), stream())
    assert rc == IRON_OK, rc
    torch.cuda.synchronize(DEV)
    assert guard_intact(buf), "written past the end of the output"
    got = out.cpu()
    if finite:
        assert not bool(torch.isnan(got).any()), "an output element was not written"
    return got, int(flag.item())


@functools.lru_cache(maxsize=None)
def conv_ref(i):
    """(x, w, b, want, S) of CONV_CASES[i]: computed once, shared, never modified (callers copy before they edit)."""
    x, w, b = O.conv_case(i)
    want, S = O.conv_reference(x, w, b, *O.CONV_CASES[i][5:])
    return x, w, b, want, S


@pytest.mark.parametrize("idx", range(len(O.CONV_CASES)), ids=["x".join(str(v) for v in c) for c in O.CONV_CASES])
def test_conv_per_element(idx):
    case = O.CONV_CASES[idx]
    x, w, b, want, S = conv_ref(idx)
    got, flag = run_conv(x, w, b, *case[5:])
    assert tuple(got.shape) == tuple(want.shape)
    ratio = O.conv_ratio(got, want, S)
    at = np.unravel_index(int(np.argmax(np.abs(got.double().numpy() - want.numpy()) / S.numpy())), tuple(want.shape))
    print("conv %s K %d: worst |got - ref| / (eps32 S) = %.3f at %s (C_CONV %.2f), flag %d" % (case, case[3] * case[5] ** 2, ratio, at, O.C_CONV, flag))
    assert ratio <= O.C_CONV
    assert flag == 0
    again, _ = run_conv(x, w, b, *case[5:])
    assert same_bits(got, again)


def test_conv_rows_do_not_depend_on_the_batch():
    """An output pixel's bits depend on its patch alone, not on where its row falls in a 128-row tile: each image of the B = 3 case
    alone (M = 182, other tile boundaries) gives that image's slice of the batched run."""
    idx = 4
    case = O.CONV_CASES[idx]
    assert case[0] == 3
    x, w, b, _, _ = conv_ref(idx)
    full, _ = run_conv(x, w, b, *case[5:])
    for i in range(3):
        one, flag = run_conv(x[i:i + 1], w, b, *case[5:])
        assert flag == 0 and same_bits(one[0], full[i]), i


def test_conv_range_flag():
    idx = 1
    case = O.CONV_CASES[idx]
    x0, w0, b, _, _ = conv_ref(idx)
    x = x0.copy()
    x[1, 3, 4, 2] = 65504.0          # fp16's largest finite value: still has a split
    want, S = O.conv_reference(x, w0, b, *case[5:])
    got, flag = run_conv(x, w0, b, *case[5:])
    ratio = O.conv_ratio(got, want, S)
    print("conv with one input element at 65504: worst ratio %.3f, flag %d" % (ratio, flag))
    assert flag == 0 and ratio <= O.C_CONV
    for bad in (65536.0, float("inf"), float("-inf"), float("nan")):
        x = x0.copy()
        x[1, 3, 4, 2] = bad
        _, flag = run_conv(x, w0, b, *case[5:], finite=False)
        assert flag == 1, bad
    w = w0.copy()
    w[63, 2, 2, 3] = 1e6
    _, flag = run_conv(x0, w, b, *case[5:], finite=False)
    assert flag == 1
    _, flag = run_conv(x0, w0, b, *case[5:], flag0=1)   # the kernel only ever ORs into the word
    assert flag == 1


# (B, H, W, Cin, Cout, ksize, stride, pad, offset of `in` in floats); the first is accepted, every other differs from it in one respect
CONV_OK = (1, 8, 8, 4, 8, 3, 1, 1, 0)
CONV_REFUSED = {
    "pad == ksize": (1, 8, 8, 4, 8, 3, 1, 3, 0),
    "H + 2 pad < ksize": (1, 2, 8, 4, 8, 5, 1, 1, 0),
    "stride 0": (1, 8, 8, 4, 8, 3, 0, 1, 0),
    "ksize 32": (1, 32, 32, 4, 8, 32, 1, 0, 0),
    "Cin 4097": (1, 4, 4, 4097, 8, 1, 1, 0, 0),
    "in misaligned": (1, 8, 8, 4, 8, 3, 1, 1, 1),
    "B 0": (0, 8, 8, 4, 8, 3, 1, 1, 0),
}


def test_conv_refusals():
    """Every buffer holds 2^20 floats, far more than any of these shapes would touch if it were wrongly accepted."""
    n = 1 << 20
    tx, tw, tb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    out = torch.full((n,), float("nan"), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(B, H, W, Cin, Cout, ks, stride, pad, off):
        with torch.cuda.device(DEV):
            rc = lib().iron_conv2d_relu(tx.data_ptr() + 4 * off, B, H, W, Cin, tw.data_ptr(), tb.data_ptr(), Cout, ks, stride, pad,
                                        out.data_ptr(), flag.data_ptr(), stream())
        torch.cuda.synchronize(DEV)
        return rc

    for name, args in CONV_REFUSED.items():
        assert call(*args) == IRON_ERR_BAD_ARG, name
        assert bool(torch.isnan(out).all()) and int(flag.item()) == 0, name
    assert call(*CONV_OK) == IRON_OK                       # the shape they all start from is accepted
    assert int(torch.isnan(out).logical_not().sum()) == 8 * 8 * 8


# ---- iron_maxpool3s2 --------------------------------------------------------------------------------------------------------------
POOL_SHAPES = ((1, 3, 3, 1), (2, 4, 5, 3), (1, 7, 8, 64), (3, 15, 15, 65), (1, 3, 40, 7), (2, 6, 6, 256))


def run_pool(x):
    B, H, W, C = x.shape
    tx = up(x)
    buf, out = guarded((B, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C))
    with torch.cuda.device(DEV):
        rc = lib().iron_maxpool3s2(tx.data_ptr(), B, H, W, C, out.data_ptr(), stream())
    assert rc == IRON_OK, rc
    torch.cuda.synchronize(DEV)
    assert guard_intact(buf), "written past the end of the output"
    return out.cpu()


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["x".join(str(v) for v in s) for s in POOL_SHAPES])
def test_maxpool(shape):
    B, H, W, C = shape
    x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)   # signed: a maximum seeded with 0 would show
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous()
    got = run_pool(x)
    assert torch.equal(got, want)
    # the last row / column belongs to no window when (H - 3) or (W - 3) is odd: NaN there must not reach the output
    y = x.copy()
    if (H - 3) % 2 == 1:
        y[:, H - 1] = np.nan
    if (W - 3) % 2 == 1:
        y[:, :, W - 1] = np.nan
    if np.isnan(y).any():
        assert torch.equal(run_pool(y), want)


# ---- iron_lpips_tap ---------------------------------------------------------------------------------------------------------------
TAP_SHAPES = ((1, 1, 64), (3, 5, 128), (6, 6, 192), (13, 13, 256), (7, 9, 320), (33, 32, 384))


def run_tap(feat, lin, H, W):
    C = feat.shape[2]
    tf, tl = up(feat), up(lin)
    buf, part = guarded((O.TAP_PARTIALS,), torch.float64)
    with torch.cuda.device(DEV):
        rc = lib().iron_lpips_tap(tf.data_ptr(), H, W, C, tl.data_ptr(), part.data_ptr(), stream())
    assert rc == IRON_OK, rc
    torch.cuda.synchronize(DEV)
    assert guard_intact(buf), "written past the end of the partials"
    return part.cpu().numpy()


@pytest.mark.parametrize("signed", (False, True), ids=("lin>=0", "lin signed"))
@pytest.mark.parametrize("shape", TAP_SHAPES, ids=["x".join(str(v) for v in s) for s in TAP_SHAPES])
def test_tap_partials(shape, signed):
    H, W, C = shape
    hw = H * W
    rng = np.random.default_rng(1000 + C + int(signed))
    feat = np.maximum(rng.standard_normal((2, hw, C)), 0.0).astype(np.float32)   # after a ReLU: about half zeros
    lin = (rng.standard_normal(C) if signed else rng.uniform(0.0, 2.0, C)).astype(np.float32)
    zeroed = feat.copy()
    zeroed[:, 0] = 0.0               # 0 / (0 + 1e-10) in both images
    if hw > 1:
        zeroed[0, 1] = 0.0           # and in one image only
    # the single-pixel map is run both ways: zeroing its only pixel would leave nothing to compare
    for f in ((feat, zeroed) if hw == 1 else (zeroed,)):
        d, want, Sd = O.tap_reference(f, lin)
        got = run_tap(f, lin, H, W)
        assert not np.isnan(got).any(), "a partial was not written"
        err = np.abs(got - want)
        worst = float((err[Sd > 0] / Sd[Sd > 0]).max()) if (Sd > 0).any() else 0.0
        print("tap %s %s: worst |got - want| / Sd = %.3e over %d waves with pixels" % (shape, "signed" if signed else "lin>=0", worst, min(hw, O.TAP_PARTIALS)))
        assert np.all(err <= 1e-12 * Sd)
        assert np.all(got[hw:] == 0.0)
        if f is zeroed:
            assert d[0] == 0.0
            if hw <= O.TAP_PARTIALS:     # wave 0's only pixel: 0 / 1e-10 - 0 / 1e-10, exactly zero and no NaN
                assert got[0] == 0.0


@pytest.mark.parametrize("C", (96, 448))
def test_tap_refusals(C):
    tf, tl = torch.zeros(2 * 4 * 512, device=DEV), torch.zeros(512, device=DEV)
    part = torch.full((O.TAP_PARTIALS,), float("nan"), dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        rc = lib().iron_lpips_tap(tf.data_ptr(), 2, 2, C, tl.data_ptr(), part.data_ptr(), stream())
    torch.cuda.synchronize(DEV)
    assert rc == IRON_ERR_BAD_ARG
    assert bool(torch.isnan(part).all())


# ---- iron_lpips_prepare -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("uint8", "float32"))
def test_prepare_bitwise(dtype):
    H, W = 5, 7
    rng = np.random.default_rng(5)
    if dtype == "uint8":
        a, b = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
        a[0, 0], a[0, 1] = 0, 255
    else:
        a, b = (rng.random((H, W, 3)).astype(np.float32) for _ in range(2))
        a[0, 0], a[0, 1] = 0.0, 1.0
    ta, tb = up(a), up(b)
    buf, out = guarded((2, H, W, 3))
    with torch.cuda.device(DEV):
        rc = lib().iron_lpips_prepare(ta.data_ptr(), tb.data_ptr(), H, W, int(dtype == "float32"), out.data_ptr(), stream())
    assert rc == IRON_OK, rc
    torch.cuda.synchronize(DEV)
    assert guard_intact(buf)
    got = out.cpu().numpy()
    want = np.stack([O.prepare_reference(a), O.prepare_reference(b)])
    assert want.dtype == np.float32 and want.shape == got.shape
    differ = np.flatnonzero(got.view(np.int32).ravel() != want.view(np.int32).ravel())
    print("prepare %s: %d of %d elements differ in their bits" % (dtype, differ.size, got.size))
    assert differ.size == 0, (differ[:8], got.ravel()[differ[:8]], want.ravel()[differ[:8]])


# ---- iron_img_ssim ----------------------------------------------------------------------------------------------------------------
SSIM_OH, SSIM_OW = (1, 15, 16, 17, 33), (1, 31, 32, 33, 65)      # H - 10, W - 10 around the 16 x 32 tile of S
SSIM_U8 = [(oh + 10, ow + 10) for oh in SSIM_OH for ow in SSIM_OW]
SSIM_F32 = [(11, 11), (11, 75), (43, 11), (43, 75), (26, 42)]     # the four corners and the centre


def run_ssim(x, y):
    """x, y [H, W, 3], both uint8 or both fp32 -> (S map [3, H - 10, W - 10], sums [3]) as numpy fp64."""
    from iron_amd import _args
    H, W = x.shape[:2]
    tx, ty = up(x), up(y)
    ws = _args.sized_workspace(lib().iron_img_ssim_workspace_bytes, H, W, device=DEV)
    sbuf, sums = guarded((3,), torch.float64)
    mbuf, smap = guarded((3, H - 10, W - 10), torch.float64)
    with torch.cuda.device(DEV):
        rc = lib().iron_img_ssim(tx.data_ptr(), ty.data_ptr(), H, W, int(x.dtype == np.float32), ws.data_ptr(), sums.data_ptr(),
                                 smap.data_ptr(), stream())
    assert rc == IRON_OK, rc
    torch.cuda.synchronize(DEV)
    assert guard_intact(sbuf) and guard_intact(mbuf), "written past the end of an output"
    S, s = smap.cpu().numpy(), sums.cpu().numpy()
    assert not np.isnan(S).any() and not np.isnan(s).any(), "an output element was not written"
    return S, s


def as_f64(img):
    return img.astype(np.float64) / 255. if img.dtype == np.uint8 else img.astype(np.float64)


def check_ssim(x, y, what):
    S, sums = run_ssim(x, y)
    H, W = x.shape[:2]
    n = (H - 10) * (W - 10)
    xd, yd = as_f64(x), as_f64(y)
    worst = 0.0
    for ch in range(3):
        want = O.ssim_map_direct(xd[:, :, ch], yd[:, :, ch])
        worst = max(worst, float(np.abs(S[ch] - want).max()))
    gap = max(abs(float(sums[ch]) - math.fsum(S[ch].ravel())) for ch in range(3))
    print("ssim %s %d x %d: worst |S - direct| %.3e, sums - total of the map %.3e (allowed %.3e)" % (what, H, W, worst, gap, 1e-12 * n))
    assert worst <= 1e-11
    assert gap <= 1e-12 * n
    return S


def ssim_pair(H, W, fp32, seed):
    """A crop of the photo and its noisy partner; fp32: off the k / 255 grid, as a render scored before quantisation."""
    trgt = np.ascontiguousarray(photo()[190:190 + H, 220:220 + W])
    pred = O.partners(trgt, seed=seed)["noise"]
    if not fp32:
        return pred, trgt
    rng = np.random.default_rng(seed)
    y = trgt.astype(np.float32) / np.float32(255.)
    x = np.clip(pred.astype(np.float32) / np.float32(255.) + rng.normal(0.0, 0.002, pred.shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return x, y


@pytest.mark.parametrize("H,W", SSIM_U8, ids=["%dx%d" % s for s in SSIM_U8])
def test_ssim_map_uint8_tile_edges(H, W):
    check_ssim(*ssim_pair(H, W, False, 40), "uint8")


@pytest.mark.parametrize("H,W", SSIM_F32, ids=["%dx%d" % s for s in SSIM_F32])
def test_ssim_map_fp32_tile_edges(H, W):
    check_ssim(*ssim_pair(H, W, True, 41), "fp32")


@pytest.mark.parametrize("fp32", (False, True), ids=("uint8", "fp32"))
def test_ssim_constant_and_identical_images(fp32):
    H, W = 27, 43                                                 # 17 x 33 outputs: two tiles along either axis
    x, _ = ssim_pair(H, W, fp32, 42)
    for k in (0, 37, 255):
        c = np.full((H, W, 3), k, dtype=np.uint8)
        if fp32:
            c = c.astype(np.float32) / np.float32(255.)
        S, sums = run_ssim(c, c.copy())
        print("ssim of two constant images k = %d (%s): max |S - 1| %.3e" % (k, c.dtype, np.abs(S - 1.0).max()))
        assert np.abs(S - 1.0).max() <= 1e-12 and np.abs(sums - 17 * 33).max() <= 1e-12 * 17 * 33
        check_ssim(c, x, "constant %d against the photo" % k)    # vx = 0 exactly on one side
        check_ssim(x, c, "the photo against constant %d" % k)
    S = check_ssim(x, x.copy(), "an image against itself")
    assert np.abs(S - 1.0).max() <= 1e-12
