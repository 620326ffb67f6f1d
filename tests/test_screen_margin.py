"""CPU: the dense sampler's screen margin (csrc/trace.hip: delta = max(12 x max|f_screen - f| on a fixed calibration set, 1e-3))
against the CPU emulation of the screen (tools/screen_margin.py: fp16 weights and activations, fp32 accumulation) on the samples
the sampler evaluates.  The margin is empirical; this pins that on S0 / S1 / S3 at 200 x 200 and on a generalised 8 x 256 net it
covers the largest emulated error over the sampler's points at least 4x -- the samples the screen decides without an exact value."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import screen_margin as SM  # noqa: E402


@pytest.mark.parametrize("scene", ["S0", "S1", "S3"])
def test_margin_covers_the_emulated_error_on_the_scenes(scene):
    r = SM.margin_report(*SM.scene_net(scene), 200)
    print(scene, r)
    assert r["samples"] > 100000
    assert r["delta"] >= 4.0 * r["max_err"], r


def test_margin_covers_the_emulated_error_on_a_generalised_net():
    r = SM.margin_report(*SM.generalised_net(0), 100)
    print("gen0", r)
    assert r["samples"] > 10000
    assert r["delta"] >= 4.0 * r["max_err"], r


def test_emulation_rounds_like_the_screen():
    """The emulated screen differs from fp32 by fp16-sized amounts, and its calibration set is the kernel's (unit ball, fixed)."""
    import torch
    sd, spec = SM.scene_net("S1")
    x = SM.calibration_points()
    assert x.shape == (SM.CALIB_POINTS, 3) and float(x.norm(dim=1).max()) <= 1.0
    from oracle import iron_ref as R
    err = (SM.screen_forward(sd, spec, x) - R.sdf_forward(sd, spec, x)[:, 0]).abs()
    assert 1e-5 < float(err.max()) < 2e-3
    assert torch.equal(SM.calibration_points(), x)
