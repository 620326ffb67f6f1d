"""CPU: the image-metric oracle (tests/_imgmetrics_oracle.py) against closed-form answers and independent restatements, and the host
side of iron_amd.image_metrics / iron_amd.eval_image_folder (the table's text, the checkpoint loader, no CPU path)."""
import os

import numpy as np
import pytest
import torch

import _imgmetrics_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def photo():
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, "g22_eval_photo.png")).convert("RGB"), dtype=np.uint8)


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------------
def test_oracle_identical_images():
    x = photo()[:96, :80].astype(np.float64) / 255.
    assert O.skimage_ssim(x, x.copy()) == pytest.approx(1.0, abs=1e-15)
    w = O.seeded_lpips_weights(1)
    assert O.lpips(x, x.copy(), *w) == 0.0


def test_oracle_psnr_of_a_constant_offset():
    rng = np.random.default_rng(0)
    x = rng.uniform(0.0, 0.8, (40, 50, 3))
    # mse = 0.01: 20 dB, less the 4.3e-8 dB that the reference's own `+ 1e-10` inside the logarithm takes off (so "20 dB to 1e-9"
    # can only be asked of the closed form with that term in it; without the term the same 1e-9 holds against 20 exactly)
    assert abs(O.psnr(x + 0.1, x) - (-10.0 * np.log10(0.01 + 1e-10))) <= 1e-9
    mse = np.mean(((x + 0.1) - x) ** 2)
    assert abs(-10.0 * np.log10(mse) - 20.0) <= 1e-9
    assert abs(O.psnr(x + 0.1, x) - 20.0) <= 5e-8


def test_oracle_uniform_filter_is_the_11x11_mean():
    x = photo()[:128, :160, 1].astype(np.float64) / 255.
    from scipy.ndimage import uniform_filter
    u = uniform_filter(x, size=11)
    rng = np.random.default_rng(1)
    for _ in range(200):
        i, j = int(rng.integers(5, x.shape[0] - 5)), int(rng.integers(5, x.shape[1] - 5))
        assert abs(u[i, j] - x[i - 5:i + 6, j - 5:j + 6].mean()) <= 1e-14
    # and S at one pixel from its definition
    y = np.clip(x + rng.normal(0, 0.05, x.shape), 0, 1)
    S = O.ssim_map(x, y)
    i, j = 40, 77
    a, b = x[i - 5:i + 6, j - 5:j + 6], y[i - 5:i + 6, j - 5:j + 6]
    ua, ub = a.mean(), b.mean()
    va, vb, vab = (a * a).mean() - ua * ua, (b * b).mean() - ub * ub, (a * b).mean() - ua * ub
    want = ((2 * ua * ub + 1e-4) * (2 * vab + 9e-4)) / ((ua * ua + ub * ub + 1e-4) * (va + vb + 9e-4))
    assert abs(S[i - 5, j - 5] - want) <= 1e-12
    assert S.shape == (x.shape[0] - 10, x.shape[1] - 10)


def test_oracle_fixture_numbers():
    """The figures the fixture was chosen by: sigma 0.05 noise gives a well-conditioned SSIM and a PSNR near 28 dB."""
    p = photo()
    assert p.shape == (512, 512, 3)
    q = O.partners(p, seed=0)["noise"]
    s = O.skimage_ssim(q.astype(np.float64) / 255., p.astype(np.float64) / 255.)
    assert 0.15 < s < 0.3
    assert 27.0 < O.psnr(q.astype(np.float64) / 255., p.astype(np.float64) / 255.) < 29.0


def test_oracle_lpips_symmetric_and_naive_convolution():
    p = photo()
    a = p[100:131, 200:231].astype(np.float64) / 255.          # 31 x 31: the smallest size the stack accepts
    b = O.partners(np.ascontiguousarray(p[100:131, 200:231]), seed=2)["noise"].astype(np.float64) / 255.
    w = O.seeded_lpips_weights(3)
    d_ab, d_ba = O.lpips(a, b, *w), O.lpips(b, a, *w)
    assert d_ab > 0.0 and abs(d_ab - d_ba) <= 1e-15
    taps = O.lpips_features(a, w[0], w[1])
    assert [tuple(t.shape[1:]) for t in taps] == [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    naive = O.lpips_from_features(O.naive_features(a, w[0], w[1]), O.naive_features(b, w[0], w[1]), w[2])
    assert abs(naive - d_ab) <= 1e-12, (naive, d_ab)
    with pytest.raises(RuntimeError):
        O.lpips_features(a[:30, :30], w[0], w[1])             # 30 x 30: the second pool has nothing to pool


# ---- the per-operator references (tests/test_gpu_imgmetrics_kernels.py) ----------------------------------------------------------
def test_conv_emulation_sets_c_conv():
    """C_CONV is twice what the numpy model of the kernel's split-fp16 arithmetic leaves against the fp64 reference on CONV_CASES:
    a constant that went stale (new cases, a changed model) fails here, on the CPU, before any kernel is asked."""
    worst = 0.0
    for i, case in enumerate(O.CONV_CASES):
        x, w, b = O.conv_case(i)
        want, S = O.conv_reference(x, w, b, *case[5:])
        got = O.conv_split_emulation(x, w, b, *case[5:])
        assert got.dtype == np.float32 and got.shape == tuple(want.shape)
        r = O.conv_ratio(got, want, S)
        y32 = torch.relu(torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(0, 3, 1, 2),
                                                    torch.from_numpy(b), stride=case[6], padding=case[7])).permute(0, 2, 3, 1)
        print("%s K %d: emulation %.3f eps S, torch fp32 %.3f eps S, zeros %.2f" % (case, case[3] * case[5] ** 2, r, O.conv_ratio(y32, want, S),
                                                                               float((want == 0).double().mean())))
        worst = max(worst, r)
    print("emulation's worst ratio %.3f, C_CONV %.3f" % (worst, O.C_CONV))
    assert worst <= O.C_CONV / 2
    assert worst >= O.C_CONV / 4


@pytest.mark.parametrize("idx", [0, len(O.CONV_CASES) - 1])
def test_conv_reference_against_loops(idx):
    """conv_reference's layout conventions (NHWC, [Cout, ky, kx, Cin], zero padding, stride) from the definition, by explicit loops
    with exact sums, on the first three outputs along every axis."""
    import math
    B, H, W, Cin, Cout, ks, stride, pad = O.CONV_CASES[idx]
    x, w, b = O.conv_case(idx)
    want, S = O.conv_reference(x, w, b, ks, stride, pad)
    assert tuple(want.shape) == (B, (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1, Cout)
    xd, wd = x.astype(np.float64), w.astype(np.float64)
    for oy in range(min(3, want.shape[1])):
        for ox in range(min(3, want.shape[2])):
            for o in range(min(3, Cout)):
                terms, mags = [float(b[o])], [abs(float(b[o]))]
                for ky in range(ks):
                    for kx in range(ks):
                        iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
                        if 0 <= iy < H and 0 <= ix < W:
                            for c in range(Cin):
                                terms.append(xd[0, iy, ix, c] * wd[o, ky, kx, c])   # exact: two fp32 factors
                                mags.append(abs(terms[-1]))
                assert abs(float(want[0, oy, ox, o]) - max(math.fsum(terms), 0.0)) <= 1e-13, (oy, ox, o)
                assert abs(float(S[0, oy, ox, o]) - math.fsum(mags)) <= 1e-13 * math.fsum(mags), (oy, ox, o)


def test_ssim_map_direct_agrees_with_ssim_map():
    p = photo()[200:248, 100:164].astype(np.float64) / 255.           # 64 wide, 48 high
    q = O.partners(np.ascontiguousarray(photo()[200:248, 100:164]), seed=4)["noise"].astype(np.float64) / 255.
    for ch in range(3):
        a, b = np.ascontiguousarray(p[:, :, ch]), np.ascontiguousarray(q[:, :, ch])
        direct = O.ssim_map_direct(a, b)
        assert direct.shape == (38, 54)
        assert np.abs(direct - O.ssim_map(a, b)).max() <= 1e-12


def test_tap_reference_is_the_layer_term():
    rng = np.random.default_rng(6)
    for (h, w, c), signed in (((3, 5, 128), False), ((33, 32, 64), False), ((7, 9, 320), True)):
        feat = np.maximum(rng.standard_normal((2, h * w, c)), 0.0).astype(np.float32)
        feat[:, 0] = 0.0
        feat[0, 1] = 0.0
        lin = (rng.standard_normal(c) if signed else rng.uniform(0.0, 2.0, c)).astype(np.float32)
        d, partials, Sd = O.tap_reference(feat, lin)
        assert d.shape == (h * w,) and partials.shape == (1024,) and Sd.shape == (1024,)
        assert d[0] == 0.0 and np.all(partials[h * w:] == 0.0) and np.all(Sd >= np.abs(partials))
        maps = [torch.from_numpy(feat[i].astype(np.float64)).reshape(1, h, w, c).permute(0, 3, 1, 2) for i in range(2)]
        want = float(O.lpips_layer_term(maps[0], maps[1], torch.from_numpy(lin)).item())
        assert abs(partials.sum() / (h * w) - want) <= 1e-13, (h, w, c)
        if h * w > 1024:   # wave 5 takes pixels 5 and 1029, in that order
            assert partials[5] == d[5] + d[1029] and partials[32] == d[32]


# ---- host side of the modules -----------------------------------------------------------------------------------------------------
def test_format_metrics_is_the_references_text():
    from iron_amd.eval_image_folder import format_metrics
    rows = [("0.jpg", 27.96449, 0.20563, 0.123449), ("12.jpg", 31.0005, 0.9, 0.05), ("7_a.jpg", 8.25, 0.0004, 1.23456)]
    want = ("img_name\tpsnr\tssim\tlpips\n"
            "0.jpg\t27.964\t0.206\t0.1234\n"
            "12.jpg\t31.000\t0.900\t0.0500\n"
            "7_a.jpg\t8.250\t0.000\t1.2346\n"
            "\nAverage\t22.405\t0.369\t0.4693\n")
    assert format_metrics(rows) == want
    # the reference's own statements on the same rows
    ref = 'img_name\tpsnr\tssim\tlpips\n'
    for name, psnr, ssim, d in rows:
        ref += '{}\t{:.3f}\t{:.3f}\t{:.4f}\n'.format(name, psnr, ssim, d)
    ref += '\nAverage\t{:.3f}\t{:.3f}\t{:.4f}\n'.format(np.mean([r[1] for r in rows]), np.mean([r[2] for r in rows]), np.mean([r[3] for r in rows]))
    assert format_metrics(rows) == ref
    nan_rows = [("a.jpg", 20.0, 0.5, float("nan"))]
    assert format_metrics(nan_rows) == "img_name\tpsnr\tssim\tlpips\na.jpg\t20.000\t0.500\tnan\n\nAverage\t20.000\t0.500\tnan\n"


def test_pairing_rule_and_reader(tmp_path):
    from PIL import Image
    from iron_amd import eval_image_folder as E
    from iron_amd._lib import IronError
    f1, f2 = tmp_path / "run" / "render", tmp_path / "gt"
    f1.mkdir(parents=True)
    f2.mkdir()
    img = photo()[:40, :48]
    for name in ("b.jpg", "a.x.jpg", "10.jpg"):
        Image.fromarray(img).save(str(f1 / name), quality=95)
    Image.fromarray(img).save(str(f1 / "ignored.png"))
    pairs = E.image_pairs(str(f1), str(f2))
    assert [p[0] for p in pairs] == ["10.jpg", "a.x.jpg", "b.jpg"]                      # sorted
    assert [os.path.basename(p[2]) for p in pairs] == ["10.png", "a.png", "b.png"]      # name.split('.')[0] + '.png'
    a = E.read_image_u8(str(f1 / "b.jpg"))
    assert a.dtype == np.uint8 and a.shape == (40, 48, 3)
    Image.fromarray(img[:, :, 0]).save(str(f2 / "gray.png"))
    with pytest.raises(IronError, match="gray.png"):
        E.read_image_u8(str(f2 / "gray.png"))
    with pytest.raises(IronError, match="absent.png"):
        E.read_image_u8(str(f2 / "absent.png"))


def test_checkpoint_loader(tmp_path):
    from iron_amd.image_metrics import load_lpips_state
    from iron_amd._lib import IronError
    w = O.seeded_lpips_weights(4)
    pa, pl = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex_lin.pth")
    O.write_checkpoints(pa, pl, *w)
    cw, cb, lw = load_lpips_state(pa, pl)
    for l in range(5):
        assert torch.equal(cw[l], w[0][l]) and torch.equal(cb[l], w[1][l])
        assert tuple(lw[l].shape) == (1, O.ALEX_LAYERS[l][1], 1, 1) and torch.equal(lw[l].reshape(-1), w[2][l])
    alex, lin = torch.load(pa), torch.load(pl)
    for key in list(alex.keys()):
        if not key.startswith("features."):
            continue
        broken = {k: v for k, v in alex.items() if k != key}
        torch.save(broken, str(tmp_path / "m.pth"))
        with pytest.raises(IronError, match="'%s' is missing" % key.replace(".", r"\.")) as e:
            load_lpips_state(str(tmp_path / "m.pth"), pl)
        assert "features." in str(e.value).split("keys found")[1]                      # it lists what it did find
        broken = dict(alex)
        broken[key] = alex[key][..., :-1].contiguous() if alex[key].dim() > 1 else alex[key][:-1].contiguous()
        torch.save(broken, str(tmp_path / "m.pth"))
        with pytest.raises(IronError, match="'%s' must have shape" % key.replace(".", r"\.")):
            load_lpips_state(str(tmp_path / "m.pth"), pl)
    for key in list(lin.keys()):
        torch.save({k: v for k, v in lin.items() if k != key}, str(tmp_path / "m.pth"))
        with pytest.raises(IronError, match="'%s' is missing" % key.replace(".", r"\.")):
            load_lpips_state(pa, str(tmp_path / "m.pth"))
        broken = dict(lin)
        broken[key] = lin[key].reshape(-1)                                              # [C] where the package has [1, C, 1, 1]
        torch.save(broken, str(tmp_path / "m.pth"))
        with pytest.raises(IronError, match="'%s' must have shape" % key.replace(".", r"\.")):
            load_lpips_state(pa, str(tmp_path / "m.pth"))
    torch.save([1, 2, 3], str(tmp_path / "m.pth"))
    with pytest.raises(IronError, match="state dict"):
        load_lpips_state(str(tmp_path / "m.pth"), pl)


def test_cpu_tensors_are_refused():
    from iron_amd import image_metrics as M
    from iron_amd._lib import IronError
    a = torch.zeros((16, 16, 3), dtype=torch.uint8)
    for fn in (M.psnr, M.skimage_ssim, M.psnr_device, M.skimage_ssim_device, M.skimage_ssim_map):
        with pytest.raises(IronError, match="CPU"):
            fn(a, a)
    with pytest.raises(IronError, match="CPU"):
        M.evaluate_pair(a, a)
    w = O.seeded_lpips_weights(5)
    if not torch.cuda.is_available():
        with pytest.raises(IronError, match="GPU"):
            M.LPIPS.from_state(*w)
    with pytest.raises(IronError, match="GPU"):
        M.LPIPS.from_state(*w, device="cpu")


def test_library_validates_image_arguments_on_the_host():
    """Shape checks come before any device work: callable without a GPU."""
    import ctypes
    from iron_amd import _lib
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    assert lib.iron_img_ssim_workspace_bytes(10, 64, ctypes.byref(n)) == -1            # H < 11: an error, as in skimage
    assert lib.iron_img_ssim_workspace_bytes(11, 11, ctypes.byref(n)) == 0 and n.value == 3 * 8
    assert lib.iron_lpips_workspace_bytes(30, 64, ctypes.byref(n)) == -1
    assert lib.iron_lpips_workspace_bytes(31, 31, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.iron_img_sqerr(None, None, 16, 0, None, None, None) == -1
    assert lib.iron_conv2d_relu(None, 2, 31, 31, 3, None, None, 64, 11, 4, 2, None, None, None) == -1
    assert lib.iron_lpips_forward(None, None, 64, 64, 0, None, None, None, None) == -1
