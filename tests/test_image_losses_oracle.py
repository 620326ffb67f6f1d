"""CPU: the torch restatement of the stage-2 image losses (tests/_loss_oracle.py) against G20, the reference's own
models/image_losses.py (tests/golden/make_golden_losses.py), and the drop-in surface of iron_amd.image_losses."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

import _loss_oracle as O
from _util import golden
from test_surface_signatures import _compatible


@pytest.fixture(scope="module")
def g20():
    return golden("g20_image_losses.npz")


def _cases(g):
    return json.loads(str(g["meta_json"]))["cases"]


def _inputs(g, case, dtype):
    meta = _cases(g)[case]
    xu, yu = O.g20_images(meta["image"])
    x = torch.from_numpy(xu).float() / 255.0
    y = torch.from_numpy(yu).float() / 255.0
    m = None if meta["mask"] is None else torch.from_numpy(O.g20_mask(meta["mask"])).bool()
    return x.to(dtype), y.to(dtype), m


def test_g20_inputs_rebuild_bit_for_bit(g20):
    """The images and masks G20 was recorded on are rebuilt from tests/_loss_oracle.py's integer recipe, not stored."""
    for name in list(O.G20_IMAGES) + ["near96"]:
        x, y = O.g20_images(name)
        assert O.sha256(x) == str(g20["sha256__img__%s__x" % name]), name
        assert O.sha256(y) == str(g20["sha256__img__%s__y" % name]), name
    for name in O.G20_MASKS:
        assert O.sha256(O.g20_mask(name)) == str(g20["sha256__mask__%s" % name]), name


def test_closed_form_taps_are_bit_equal_to_the_recorded_filter_and_window(g20):
    from iron_amd.image_losses import PyramidL2Loss, _fspecial_gauss_1d, pyramid_taps
    f = g20["pyramid_f"]
    assert f.dtype == np.float32 and f.shape == (3, 3, 7, 7)
    for taps in (pyramid_taps(), O.pyramid_taps()):
        for c in range(3):
            assert np.array_equal(f[c, c].view(np.uint32), taps.view(np.uint32))
    assert np.array_equal(PyramidL2Loss().f.numpy().view(np.uint32), f.view(np.uint32))
    assert not f[0, 1].any() and not f[2, 0].any()
    win = g20["ssim_win"]
    assert np.array_equal(_fspecial_gauss_1d(11, 1.5).numpy().view(np.uint32), win.view(np.uint32))
    assert np.array_equal(O.gauss_1d(11, 1.5).numpy().view(np.uint32), win.view(np.uint32))
    # the backward's conv^T is the same correlation: the taps are point symmetric bit for bit
    t = pyramid_taps()
    assert np.array_equal(t, t[::-1, ::-1])


def _oracle(kind, x, y, m):
    x = x.clone().requires_grad_(True)
    y = y.clone().requires_grad_(True)
    loss = O.pyramid_l2(x, y) if kind == "pyr" else O.ssim(x, y, m)
    dx, dy = torch.autograd.grad(loss, (x, y))
    return float(loss.detach()), dx.reshape(-1).numpy(), dy.reshape(-1).numpy()


def test_oracle_matches_g20_in_fp64(g20):
    import warnings
    n = 0
    for case, meta in _cases(g20).items():
        x, y, m = _inputs(g20, case, torch.float64)
        idx = g20["case__%s__idx" % case]
        for kind in meta["losses"]:
            p = "case__%s__%s__" % (case, kind)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                loss, dx, dy = _oracle(kind, x, y, m)
            ref = float(g20[p + "loss64"])
            assert abs(loss - ref) <= 1e-12 * max(abs(ref), 1e-30) + 1e-15, (case, kind, loss, ref)
            for name, got in (("dx", dx), ("dy", dy)):
                want = g20[p + name + "64"]
                scale = float(g20[p + name + "max64"])
                assert np.abs(got[idx] - want).max() <= 1e-12 * scale, (case, kind, name)
            n += 1
    assert n == 15


def test_erosion_restatement_properties():
    gen = torch.Generator().manual_seed(3)
    k = torch.ones(11, 11)
    full = torch.ones(2, 1, 40, 57)
    assert bool((O.erosion(full, k) > 0.5).all())  # the border never wins
    for p in (0.002, 0.02, 0.2):
        m = (torch.rand(2, 1, 40, 57, generator=gen) > p).float()
        m[:, :, 10:20, 30:45] = 0
        e = O.erosion(m, k)
        assert torch.equal(e, O.min_filter(m, 11))
        keep = e > 0.5
        assert bool((m[keep] > 0.5).all())  # inside the mask
        assert not bool(keep[:, :, 5:25, 25:50].any())  # the hole grown by 5 px


def test_image_losses_signatures_are_compatible_with_the_reference(g20):
    import iron_amd.image_losses as IL
    sigs = json.loads(str(g20["signatures_json"]))
    assert set(sigs) == {"PyramidL2Loss", "_fspecial_gauss_1d", "gaussian_filter", "ssim_loss_fn"}
    for name, entry in sigs.items():
        obj = getattr(IL, name)
        if entry["type"] == "function":
            assert _compatible(entry["params"], obj) is None, (name, _compatible(entry["params"], obj))
        else:
            for mname, params in entry["methods"].items():
                assert _compatible(params, getattr(obj, mname)) is None, (name, mname)


def test_install_as_models_resolves_the_drivers_import_line():
    import iron_amd
    import iron_amd.image_losses
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    try:
        for k in saved:
            del sys.modules[k]
        iron_amd.install_as_models()
        ns = {}
        exec("from models.image_losses import PyramidL2Loss, ssim_loss_fn", ns)  # render_surface.py / render_nir.py line 24
        assert ns["PyramidL2Loss"] is iron_amd.image_losses.PyramidL2Loss
        assert ns["ssim_loss_fn"] is iron_amd.image_losses.ssim_loss_fn
        assert importlib.import_module("models.image_losses") is iron_amd.image_losses
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---- the per-pixel bound of tests/test_gpu_image_loss_pixels.py, checked on the CPU ------------------------------------------------
def _dense_cases():
    """Every dense case the GPU file judges per pixel: (name, case, tile)."""
    out = []
    for h, w in O.PYR_SIZES:
        x, y = O.case_images(31, 2, 3, h, w)
        out.append(("pyr %dx%d" % (h, w), dict(kind="pyr", x=x, y=y), O.PYR_TILE))
    for h, w, win in O.SSIM_SHAPES + O.SSIM_PASS_THROUGH:
        x, y = O.case_images(41, 1, 3, h, w)
        out.append(("ssim %dx%d win %d" % (h, w, win), dict(kind="ssim", x=x, y=y, win=win), O.SSIM_TILE))
        if (h, w, win) in O.SSIM_SHAPES:
            out.append(("ssim %dx%d win %d masked" % (h, w, win), dict(kind="ssim", x=x, y=y, win=win, mask=O.det_mask(1, h, w)), O.SSIM_TILE))
    return out


def _grad64(fn, x, y):
    x = x.double().requires_grad_(True)
    y = y.double().requires_grad_(True)
    loss = fn(x, y)
    dx, dy = torch.autograd.grad(loss, (x, y))
    return loss.detach().numpy(), dx.numpy(), dy.numpy()


def test_fp32_oracle_meets_the_per_pixel_bound_at_margin_1_and_not_at_099():
    """F is the fp32 restatement's own worst pixel: judged against itself it passes at margin 1 with its worst pixel exactly on
    the bound, and fails at 0.99 -- the bound is one floor wide, not a figure with slack in it."""
    n = 0
    for name, case, tile in _dense_cases():
        r64, r32, F = O.floors(case)
        for k in ("dx", "dy"):
            assert F[k] > 0, (name, k)
            v = O.judge(r32[k], r64[k], F[k], 1.0, tile)
            assert v.ok and v.ratio == 1.0, (name, k, v)
            assert not O.judge(r32[k], r64[k], F[k], 0.99, tile).ok, (name, k)
            assert O.judge(r64[k], r64[k], F[k], 0.0).ok
            n += 1
    assert n == 2 * (5 + 12 + 10)
    # a non-finite value fails whatever the margin, and the report names the pixel and its seam
    x, y = O.case_images(41, 1, 3, 43, 75)
    r64, _, F = O.floors(dict(kind="ssim", x=x, y=y))
    got = r64["dx"].copy()
    got[0, 1, 16, 32] = np.nan
    v = O.judge(got, r64["dx"], F["dx"], 1e30, O.SSIM_TILE)
    assert not v.ok and v.index == (0, 1, 16, 32) and "row 0 of its 16-row tile, column 0 of its 32-column tile" in v.where, v


def test_manual_pyramid_adjoint_is_the_autograd_gradient():
    for h, w in O.PYR_SIZES:
        x, y = O.case_images(31, 2, 3, h, w)
        for scale in (1.0, -2.5):
            _, dx, _ = _grad64(lambda a, b: scale * O.pyramid_l2(a, b), x, y)
            g = O.pyramid_l2_grad(x.double(), y.double(), scale=scale).numpy()
            assert np.abs(g - dx).max() <= 1e-13 * np.abs(dx).max(), (h, w)
        per = O.pyramid_l2(x.double(), y.double(), per_image=True)
        assert abs(float(per.sum()) - float(O.pyramid_l2(x.double(), y.double()))) <= 1e-15
        assert abs(float(per[1]) - float(O.pyramid_l2(x[1:].double(), y[1:].double()))) <= 1e-15


def test_wrong_pyramid_restatements_fail_the_bound_at_margin_4():
    """Level divisors from the floor-pooled sizes, and a pooling adjoint that also feeds the dropped last row / column: each is
    the restatement itself wherever no level is odd (16x16, 64x64) and fails margin 4 by orders of magnitude wherever one is."""
    for h, w in O.PYR_SIZES:
        x, y = O.case_images(31, 2, 3, h, w)
        r64, _, F = O.floors(dict(kind="pyr", x=x, y=y))
        _, dx, _ = _grad64(lambda a, b: O.pyramid_l2(a, b, divisors="floor"), x, y)
        floor_div = O.judge(dx, r64["dx"], F["dx"], O.MARGIN, O.PYR_TILE)
        clamp = O.judge(O.pyramid_l2_grad(x.double(), y.double(), adjoint="clamp").numpy(), r64["dx"], F["dx"], O.MARGIN, O.PYR_TILE)
        odd = (h, w) not in ((16, 16), (64, 64))
        assert floor_div.ok != odd and clamp.ok != odd, (h, w, floor_div, clamp)
        if odd:
            assert floor_div.ratio > 1e3 and clamp.ratio > 1e3, (h, w, floor_div, clamp)


def test_wrong_mask_restatements_fail_the_bound_at_margin_4():
    """An erosion that counts out-of-image pixels as zero loses the kept pixels near the border (loss and gradient fail); a border
    band that counts 0 changes the loss alone.  win 1 has neither a band nor a window that leaves the image: both are exact there."""
    for h, w, win in O.SSIM_SHAPES:
        x, y = O.case_images(41, 1, 3, h, w)
        m = O.det_mask(1, h, w)
        r64, _, F = O.floors(dict(kind="ssim", x=x, y=y, win=win, mask=m))
        for kw, grad_fails in ((dict(erode_pad=0.0), True), (dict(band_value=0.0), False)):
            loss, dx, _ = _grad64(lambda a, b: O.ssim(a, b, m, win_size=win, **kw), x, y)
            vl = O.judge(loss, r64["loss"], F["loss"], O.MARGIN)
            vg = O.judge(dx, r64["dx"], F["dx"], O.MARGIN, O.SSIM_TILE)
            if win == 1:
                assert vl.ratio == 0.0 and vg.ratio == 0.0, (h, w, win, kw)
                continue
            assert not vl.ok and vl.ratio > 1e3, (h, w, win, kw, vl)
            assert abs(float(loss) - float(r64["loss"])) > max(1e-6 * float(r64["loss"]), 1.5 * F["loss"])  # the GPU file's loss rule
            assert vg.ok != grad_fails, (h, w, win, kw, vg)


def _threshold_mask(h, w):
    m = torch.ones(1, 1, h, w)
    for (py, px), v in O.THRESHOLD_PIXELS.items():
        m[0, 0, py, px] = v
    return m


def test_masked_cases_keep_and_drop_enough():
    """Every masked case keeps at least a quarter of its valid map, at least one pixel of the border band (win 1 has no band)
    and drops at least one pixel; a speckle mask under the largest window keeps nothing of the valid map, hence det_mask."""
    for h, w, win in O.SSIM_SHAPES:
        for m in [O.det_mask(1, h, w)] + ([_threshold_mask(h, w)] if (h, w, win) == (27, 43, 11) else []):
            s = O.mask_stats(m, win)
            assert s["valid_kept"] >= 0.25 and s["dropped"] >= 1, (h, w, win, s)
            assert (s["band_kept"] >= 1) if win >= 3 else (s["band_kept"] == 0), (h, w, win, s)
    speckle = torch.from_numpy((O._hash(36 * 52, 99) % np.uint64(25) != 0).reshape(1, 1, 36, 52))
    assert O.mask_stats(speckle, 21)["valid_kept"] == 0.0
    # only 0.5 and below, and NaN, are dropped: the oracle's kept set under the threshold mask
    keep = O.keep_map(_threshold_mask(27, 43), 11)[0, 0]
    gone = torch.zeros(27, 43, dtype=torch.bool)
    for (py, px), v in O.THRESHOLD_PIXELS.items():
        if not (v > 0.5):
            gone[max(py - 5, 0):py + 6, max(px - 5, 0):px + 6] = True
        else:
            assert bool(keep[py, px]), (py, px, v)
    assert torch.equal(~keep, gone) and int(gone.sum()) == 3 * 9 * 11


def test_probe_masks_keep_exactly_one_valid_pixel():
    n = 0
    for h, w, win in O.SSIM_SHAPES:
        pts = O.ssim_probe_points(h, w, win)
        assert 8 <= len(pts) <= 15, (h, w, win, len(pts))
        for q in pts:
            m, keep, n_band = O.probe_mask(h, w, win, q)   # asserts the property
            assert int(m.sum()) == win * win and int(keep.sum()) == n_band + 1
            n += 1
    _, keep, n_band = O.probe_mask(26, 42, 11, (0, 0))
    assert int(keep.sum()) == 36 and n_band == 35 and bool(keep[:6, :6].all())   # the 6x6 corner
    _, keep, n_band = O.probe_mask(43, 75, 11, (16, 32))
    assert int(keep.sum()) == 1 and n_band == 0
    assert n > 100


def test_ssim_map_is_what_ssim_averages_and_probes_read_one_pixel_of_it():
    x, y = O.case_images(41, 1, 3, 27, 43)
    x, y = x.double(), y.double()
    smap = O.ssim_map(x, y, 11)
    assert smap.shape == (1, 1, 17, 33)
    assert abs(float(1.0 - smap.mean()) - float(O.ssim(x, y))) <= 1e-15
    for q in O.ssim_probe_points(27, 43, 11):
        m, keep, n_band = O.probe_mask(27, 43, 11, q)
        want = 1.0 - (n_band + float(smap[0, 0, q[0], q[1]])) / int(keep.sum())
        assert abs(float(O.ssim(x, y, m)) - want) <= 1e-14, q


def test_impulse_loss_depends_on_where_the_impulse_sits():
    """The pyramid loss of one impulse varies with its position (zero padding and floor-dropped rows differ per level), so it is a
    forward probe of the per-level border handling; the fp32 restatement stays within 1.5e-7 relative of the fp64 one."""
    for h, w in O.PYR_SIZES:
        pts = O.impulse_points(h, w)
        assert 25 <= len(pts) <= 72
        X = torch.cat([O.impulse(h, w, p)[0] for p in pts])
        l64 = O.pyramid_l2(X.double(), torch.zeros_like(X).double(), per_image=True).numpy()
        l32 = O.pyramid_l2(X, torch.zeros_like(X), per_image=True).double().numpy()
        assert (l64.max() - l64.min()) / l64.min() > 0.02, (h, w)
        assert (np.abs(l32 - l64) / l64).max() < 1.5e-7, (h, w)
