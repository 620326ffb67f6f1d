"""GPU: PSNR, uniform-window SSIM and LPIPS (csrc/imgmetrics.hip, iron_amd.image_metrics) against the fp64 restatement of
evaluation/eval_image_folder.py (tests/_imgmetrics_oracle.py): the precision contract of DESIGN.md §14, determinism, errors and the
`python -m iron_amd.eval_image_folder` command.

Where the bounds come from.  uint8 path: the window sums are exact integers, so only the fp64 evaluation of S and a fixed-order fp64
mean separate the kernel from the oracle fed the same integers: 1e-12 on SSIM, 1e-9 dB on PSNR.  Against the oracle fed the
reference's float32(k / 255) the allowance is twice that oracle's own distance from the integer-fed one (plus the 1e-12 above),
computed here.  fp32 path: twice the distance between a float32 and a float64 run of the oracle on the same input, floor 1e-6.
LPIPS per layer: rel-L2 5e-7, the contract tests/test_gpu_gemm.py holds the split-fp16 product to, and on the two small images
the per-element C_CONV eps32 S of tests/test_gpu_imgmetrics_kernels.py (the constant comes from the oracle's emulation).  LPIPS end to end:
max(4 e32, 1e-6) relative, e32 the error of the oracle's own float32 CPU run against its float64 run (4 = the ratio between the
split's 22-bit operands and fp32's 24 bits); every figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _imgmetrics_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def dev():
    return torch.device("cuda", 0)


def photo():
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, "g22_eval_photo.png")).convert("RGB"), dtype=np.uint8)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def u8_cases():
    """(name, pred, trgt) uint8 pairs: the fixture against its four partners, then the sizes of the contract."""
    p = photo()
    cases = [("fixture/" + k, v, p) for k, v in O.partners(p, seed=0).items()]
    for i, (H, W) in enumerate(((11, 11), (11, 64), (37, 53), (800, 800), (1600, 1200))):
        t = O.sized_image(p, H, W)
        cases.append(("%dx%d" % (H, W), O.partners(t, seed=10 + i)["noise"], t))
    return cases


def f64(x):
    return x.astype(np.float64) / 255.


def f32(x):
    return x.astype(np.float32) / np.float32(255.)   # the reference's reader: imread(...).astype(np.float32) / 255.


# ---- PSNR / SSIM ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(9))
def test_psnr_ssim_uint8(idx):
    from iron_amd import image_metrics as M
    name, pred, trgt = u8_cases()[idx]
    a, b = cu(pred), cu(trgt)
    got_p, got_s = M.psnr(a, b), M.skimage_ssim(a, b)
    want_p, want_s = O.psnr(f64(pred), f64(trgt)), O.skimage_ssim(f64(pred), f64(trgt))
    ref_p, ref_s = O.psnr(f32(pred), f32(trgt)), O.skimage_ssim(f32(pred), f32(trgt))
    tol_p, tol_s = 2.0 * abs(ref_p - want_p) + 1e-9, 2.0 * abs(ref_s - want_s) + 1e-12
    print("%s: psnr %.12f (oracle %+.3e, fp32-fed oracle %+.3e, allowed %.3e)  ssim %.15f (oracle %+.3e, fp32-fed oracle %+.3e, allowed %.3e)"
          % (name, got_p, got_p - want_p, got_p - ref_p, tol_p, got_s, got_s - want_s, got_s - ref_s, tol_s))
    assert abs(got_p - want_p) <= 1e-9
    assert abs(got_s - want_s) <= 1e-12
    assert abs(got_p - ref_p) <= tol_p
    assert abs(got_s - ref_s) <= tol_s
    # the device variants hold the same numbers
    assert abs(float(M.psnr_device(a, b)) - got_p) <= 1e-12
    assert abs(float(M.skimage_ssim_device(a, b)) - got_s) <= 1e-15


def test_ssim_map_uint8():
    from iron_amd import image_metrics as M
    p = photo()
    q = O.partners(p, seed=0)["jpeg"]
    S = M.skimage_ssim_map(cu(q), cu(p)).cpu().numpy()
    assert S.shape == (3, 502, 502)
    for ch in range(3):
        want = O.ssim_map(f64(p)[:, :, ch].copy(), f64(q)[:, :, ch].copy())
        assert np.abs(S[ch] - want).max() <= 1e-11   # per pixel: the cancellation in vx + vy + C2 >= 9e-4 amplifies 1e-16 by <= 1e3


@pytest.mark.parametrize("idx", range(9))
def test_psnr_ssim_fp32(idx):
    from iron_amd import image_metrics as M
    name, pred, trgt = u8_cases()[idx]
    rng = np.random.default_rng(100 + idx)
    # a render scored before quantisation: float32 values off the k / 255 grid
    x = np.clip(f32(pred) + rng.normal(0.0, 0.002, pred.shape).astype(np.float32), 0.0, 1.0).astype(np.float32)
    y = f32(trgt)
    got_p, got_s = M.psnr(cu(x), cu(y)), M.skimage_ssim(cu(x), cu(y))
    s32, s64 = O.skimage_ssim(x, y), O.skimage_ssim(x.astype(np.float64), y.astype(np.float64))
    p32, p64 = O.psnr(x, y), O.psnr(x.astype(np.float64), y.astype(np.float64))
    tol_s, tol_p = max(2.0 * abs(s32 - s64), 1e-6), max(2.0 * abs(p32 - p64), 1e-6)
    print("%s fp32: ssim %.9f - oracle64 %+.3e (oracle32 - oracle64 %+.3e, allowed %.3e); psnr - oracle64 %+.3e (oracle32 %+.3e, allowed %.3e)"
          % (name, got_s, got_s - s64, s32 - s64, tol_s, got_p - p64, p32 - p64, tol_p))
    assert abs(got_s - s64) <= tol_s
    assert abs(got_p - p64) <= tol_p


def test_small_and_mismatched_images_are_errors():
    from iron_amd import image_metrics as M
    from iron_amd._lib import IronError
    a = torch.zeros((10, 64, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(IronError, match="win_size"):
        M.skimage_ssim(a, a)
    b = torch.zeros((16, 16, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(IronError):
        M.psnr(b, b.float())
    with pytest.raises(IronError):
        M.skimage_ssim(b, b[:, :15])
    with pytest.raises(IronError, match="CPU"):
        M.psnr(b.cpu(), b.cpu())
    assert M.skimage_ssim(b, b) == 1.0 and M.psnr(b, b) == pytest.approx(100.0, abs=1e-9)


# ---- LPIPS ----------------------------------------------------------------------------------------------------------------------
def lpips_cases():
    p = photo()
    cases = [("fixture/" + k, v, p) for k, v in O.partners(p, seed=0).items()]
    for i, (H, W) in enumerate(((31, 31), (64, 48), (800, 800))):
        t = O.sized_image(p[64:], H, W)
        cases.append(("%dx%d" % (H, W), O.partners(t, seed=20 + i)["noise"], t))
    return cases


_W = {}


def weights():
    if not _W:
        from iron_amd.image_metrics import LPIPS
        _W["cpu"] = O.seeded_lpips_weights(7)
        _W["gpu"] = LPIPS.from_state(*_W["cpu"], device=dev())
    return _W["cpu"], _W["gpu"]


@pytest.mark.parametrize("idx", range(7))
def test_lpips_per_layer(idx):
    """Each convolution, fed what the device computed before it, against the fp64 oracle on that same input.  On the two small
    images every output element is also held to the per-element contract C_CONV eps32 S of tests/test_gpu_imgmetrics_kernels.py,
    where a few wrong border outputs cannot hide in the norm; conv1's input there is the device's own fp32 prepare
    (O.prepare_reference, which test_prepare_bitwise pins bit for bit)."""
    name, pred, _ = lpips_cases()[idx]
    (cw, cb, _), lp = weights()
    taps = [t.cpu().double()[None] for t in lp.features(cu(pred))]
    x = O.lpips_input(f32(pred), torch.float64)   # the device forms float(k) / 255, 2 x - 1 and the scaling layer in fp32
    per_element = name in ("31x31", "64x48")
    x_dev = torch.from_numpy(O.prepare_reference(pred)).double().permute(2, 0, 1)[None]
    for l in range(5):
        want = O.conv_relu(x, l, cw, cb)
        assert taps[l].shape == want.shape, (taps[l].shape, want.shape)
        rel = float(torch.linalg.norm(taps[l] - want) / torch.linalg.norm(want))
        print("%s conv%d %s: rel-L2 %.3e" % (name, l + 1, tuple(want.shape[1:]), rel))
        assert rel <= 5e-7, (name, l, rel)
        if per_element:
            _, _, k, s, p = O.ALEX_LAYERS[l]
            ref, S = O.conv_reference(x_dev.permute(0, 2, 3, 1), cw[l].permute(0, 2, 3, 1), cb[l], k, s, p)
            ratio = O.conv_ratio(taps[l].permute(0, 2, 3, 1), ref, S)
            print("%s conv%d: worst |got - ref| / (eps32 S) = %.3f (C_CONV %.2f)" % (name, l + 1, ratio, O.C_CONV))
            assert ratio <= O.C_CONV, (name, l, ratio)
        x = taps[l]
        if O.POOL_AFTER[l]:
            x = torch.nn.functional.max_pool2d(x, 3, 2)
        x_dev = x


@pytest.mark.parametrize("idx", range(7))
def test_lpips_end_to_end(idx):
    name, pred, trgt = lpips_cases()[idx]
    w, lp = weights()
    got = lp(cu(pred), cu(trgt))
    d64 = O.lpips(f64(pred), f64(trgt), *w, dtype=torch.float64)
    d32 = O.lpips(f32(pred), f32(trgt), *w, dtype=torch.float32)
    e32 = abs(d32 - d64) / d64
    ours = abs(got - d64) / d64
    tol = max(4.0 * e32, 1e-6)
    print("%s: lpips %.10f  oracle64 %.10f  ours rel %.3e  e32 rel %.3e  ours / e32 %.2f  allowed %.3e" % (name, got, d64, ours, e32, ours / max(e32, 1e-300), tol))
    assert d64 > 0.0
    assert ours <= tol
    # fp32 images holding the same values score the same bits, and the metric is symmetric
    assert lp(cu(f32(pred)), cu(f32(trgt))) == got
    assert lp(cu(trgt), cu(pred)) == got


def test_lpips_identical_inputs_and_errors():
    from iron_amd.image_metrics import LPIPS
    from iron_amd._lib import IronError
    (cw, cb, lw), lp = weights()
    p = photo()
    assert lp(cu(p), cu(p.copy())) == 0.0
    assert lp(cu(p[:31, :31]), cu(p[:31, :31])) == 0.0
    with pytest.raises(IronError, match="at least 31"):
        lp(cu(p[:30, :30]), cu(p[:30, :30]))
    with pytest.raises(IronError, match="at least 31"):
        lp(cu(p[:64, :30]), cu(p[:64, :30]))
    with pytest.raises(IronError, match="CPU"):
        lp(torch.from_numpy(p), torch.from_numpy(p))
    # operands beyond fp16 range: the range error, not inf
    big = LPIPS.from_state([cw[0] * 1e6] + list(cw[1:]), cb, lw, device=dev())
    with pytest.raises(IronError, match="range"):
        big(cu(p[:64, :64]), cu(p[64:128, :64]))
    with pytest.raises(IronError, match="range"):
        big.features(cu(p[:64, :64]))
    with pytest.raises(IronError, match="finite"):
        LPIPS.from_state([cw[0] * float("inf")] + list(cw[1:]), cb, lw, device=dev())
    with pytest.raises(IronError, match="shape"):
        LPIPS.from_state([cw[0][:, :, :10]] + list(cw[1:]), cb, lw, device=dev())


def test_lpips_from_files(tmp_path):
    from iron_amd.image_metrics import LPIPS
    w, lp = weights()
    pa, pl = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex_lin.pth")
    O.write_checkpoints(pa, pl, *w)
    lp2 = LPIPS.from_files(pa, pl, device=dev())
    p = photo()[:96, :128]
    q = O.partners(p, seed=3)["blur"]
    assert lp2(cu(q), cu(p)) == lp(cu(q), cu(p))


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_bitwise_determinism():
    from iron_amd import image_metrics as M
    _, lp = weights()
    p = photo()
    q = O.partners(p, seed=0)["noise"]
    a, b = cu(q), cu(p)
    x, y = cu(f32(q)), cu(f32(p))
    for u, v in ((a, b), (x, y)):
        r1 = (M.squared_error_device(u, v).cpu(), M._ssim_sums(u, v, False)[0].cpu(), M.skimage_ssim_map(u, v).cpu(), lp.lpips_device(u, v).cpu())
        # other work in between, so that a second run does not simply find the first one's buffers untouched
        M.skimage_ssim(cu(O.sized_image(p, 300, 200)), cu(O.sized_image(p[8:], 300, 200)))
        lp(cu(p[:200, :300]), cu(q[:200, :300]))
        r2 = (M.squared_error_device(u, v).cpu(), M._ssim_sums(u, v, False)[0].cpu(), M.skimage_ssim_map(u, v).cpu(), lp.lpips_device(u, v).cpu())
        for t1, t2 in zip(r1, r2):
            assert torch.equal(t1, t2)
    t1 = [t.cpu() for t in lp.features(a)]
    t2 = [t.cpu() for t in lp.features(a)]
    assert all(torch.equal(u, v) for u, v in zip(t1, t2))
    # the one-call forward and the staged forward are the same kernels in the same order
    taps, out = lp.run_staged(a, b)
    assert float(out[0]) == pytest.approx(float(lp.lpips_device(a, b)[0]), rel=1e-14)


# ---- the command ----------------------------------------------------------------------------------------------------------------
def _folders(tmp_path):
    from PIL import Image
    p = photo()
    f1, f2 = tmp_path / "out" / "render_all", tmp_path / "gt"
    f1.mkdir(parents=True)
    f2.mkdir()
    parts = O.partners(p[:256, :320], seed=5)
    names = []
    for i, kind in enumerate(("noise", "blur", "mask")):
        name = "%d_%s" % (i, kind)
        Image.fromarray(parts[kind]).save(str(f1 / (name + ".jpg")), quality=92)
        Image.fromarray(np.ascontiguousarray(p[:256, :320])).save(str(f2 / (name + ".png")))
        names.append(name + ".jpg")
    return f1, f2, names


def _run(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "iron_amd.eval_image_folder"] + args, cwd=str(cwd), env=env, capture_output=True, text=True,
                          timeout=600)


def _parse(text, names):
    lines = text.split("\n")
    assert lines[0] == "img_name\tpsnr\tssim\tlpips"
    assert [l.split("\t")[0] for l in lines[1:1 + len(names)]] == sorted(names)
    assert lines[1 + len(names)] == "" and lines[2 + len(names)].startswith("Average\t") and lines[3 + len(names):] == [""]
    rows = [l.split("\t") for l in lines[1:1 + len(names)]] + [lines[2 + len(names)].split("\t")]
    for r in rows:
        assert len(r) == 4
        assert len(r[1].split(".")[1]) == 3 and len(r[2].split(".")[1]) == 3 and (r[3] == "nan" or len(r[3].split(".")[1]) == 4)
    return rows


def test_command(tmp_path):
    from iron_amd import eval_image_folder as E
    from iron_amd.image_metrics import evaluate_pair
    w, lp = weights()
    f1, f2, names = _folders(tmp_path)
    pa, pl = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex_lin.pth")
    O.write_checkpoints(pa, pl, *w)
    want = []
    for name in sorted(names):
        a, b = E.read_image_u8(str(f1 / name)), E.read_image_u8(str(f2 / (name.split('.')[0] + '.png')))
        o = (O.psnr(f64(a), f64(b)), O.skimage_ssim(f64(a), f64(b)), O.lpips(f64(b), f64(a), *w))
        got = evaluate_pair(a, b, lpips=lp)       # the unrounded values meet the bounds of the tests above
        e32 = abs(O.lpips(f32(b), f32(a), *w, dtype=torch.float32) - o[2]) / o[2]
        print("%s: psnr %+.3e ssim %+.3e lpips rel %.3e (e32 %.3e)" % (name, got[0] - o[0], got[1] - o[1], abs(got[2] - o[2]) / o[2], e32))
        assert abs(got[0] - o[0]) <= 1e-9 and abs(got[1] - o[1]) <= 1e-12 and abs(got[2] - o[2]) / o[2] <= max(4.0 * e32, 1e-6)
        got_no = evaluate_pair(a, b)
        assert got_no[:2] == got[:2] and np.isnan(got_no[2])
        want.append(o)
    want.append(tuple(float(np.mean([o[i] for o in want])) for i in range(3)))

    r = _run([str(f1), str(f2), "--alexnet", pa, "--lpips-lin", pl], tmp_path)
    assert r.returncode == 0, r.stderr
    mpath = tmp_path / "out" / "metrics.txt"            # FOLDER1/../metrics.txt
    rows = _parse(mpath.read_text(), names)
    for row, o in zip(rows, want):
        # within one unit of the last printed digit: a value may sit on a rounding boundary
        assert abs(float(row[1]) - o[0]) <= 1.0e-3 + 1e-12 and abs(float(row[2]) - o[1]) <= 1.0e-3 + 1e-12 and abs(float(row[3]) - o[2]) <= 1.0e-4 + 1e-12, (row, o)
    with_weights = mpath.read_text()

    mpath.unlink()
    r = _run([str(f1), str(f2)], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "lpips" in r.stderr.lower() and "nan" in r.stderr
    rows_no = _parse(mpath.read_text(), names)
    assert all(row[3] == "nan" for row in rows_no)
    assert [row[:3] for row in rows_no] == [row[:3] for row in _parse(with_weights, names)]


def test_command_errors(tmp_path):
    from PIL import Image
    f1, f2, names = _folders(tmp_path)
    # a grayscale partner
    Image.fromarray(photo()[:256, :320, 0]).save(str(f2 / "1_blur.png"))
    r = _run([str(f1), str(f2)], tmp_path)
    assert r.returncode != 0 and "1_blur.png" in r.stderr, (r.returncode, r.stderr)
    # a missing partner
    (f2 / "1_blur.png").unlink()
    r = _run([str(f1), str(f2)], tmp_path)
    assert r.returncode != 0 and "1_blur" in r.stderr, (r.returncode, r.stderr)
    # a size mismatch
    Image.fromarray(np.ascontiguousarray(photo()[:200, :320])).save(str(f2 / "1_blur.png"))
    r = _run([str(f1), str(f2)], tmp_path)
    assert r.returncode != 0 and "1_blur" in r.stderr, (r.returncode, r.stderr)
    # one weight file without the other
    r = _run([str(f1), str(f2), "--alexnet", "x.pth"], tmp_path)
    assert r.returncode != 0
