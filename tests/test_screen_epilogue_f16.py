"""CPU: a packed-fp16 epilogue for the screen (softplus_100 on fp16 halves of the rounded accumulator), through its emulation
(tools/screen_margin_f16.py).  It was built for csrc/mlp_h2.h, measured slower, and not adopted.

  * the emulated activation is softplus_100 to within fp16 rounding of its intermediate terms;
  * the margin a screen with that epilogue would calibrate still covers its own emulated error on the sampler's points >= 4x;
  * but it moves the screen's values off the fp32-epilogue emulation by more than a third of the median tolerance of
    tests/test_gpu_screen_stream.py on the points that test uses: rounding the accumulator to fp16 before softplus re-rounds every
    activation, and the screen's output is as sensitive to that as to its own fp16 error.  That is the other reason the kernel keeps
    the fp32 epilogue."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import screen_margin as SM  # noqa: E402
import screen_margin_f16 as S16  # noqa: E402


def test_emulated_activation_is_softplus_to_fp16_rounding():
    from oracle import iron_ref as R
    z = torch.linspace(-0.2, 2.0, 200001)
    got = S16.softplus100_f16(z).double()
    want = R.softplus100(z.double())
    assert torch.isfinite(got).all()
    # |z| rounding (2^-12 relative) and a few fp16 roundings of terms <= ln2 / 100
    assert float(((got - want).abs() - want.abs() * 2.0 ** -11).max()) <= 2.0e-5
    assert float(S16.softplus100_f16(torch.tensor([float("nan")]))[0]) != float(S16.softplus100_f16(torch.tensor([0.0]))[0])


def test_fp16_epilogue_margin_covers_its_emulated_error():
    r = S16.margin_report(*SM.scene_net("S0"), 100)
    print("S0", r)
    assert r["samples"] > 10000
    assert r["delta"] >= 4.0 * r["max_err"], r


def test_fp16_epilogue_departs_from_the_screen_emulation():
    sd, spec = SM.scene_net("S0")
    g = S16.gate(sd, spec, S16.gate_points(n=30_000))
    print("S0", g)
    assert g["finite"]
    assert g["median"] > 1e-4 / 3, g
