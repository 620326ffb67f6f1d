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
