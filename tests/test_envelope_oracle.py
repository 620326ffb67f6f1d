"""CPU: the envelope cases of tests/_envelope_cases.py are what they claim to be, and the reference's own fp32 run passes every
comparison tests/test_gpu_envelope_entries.py makes of a kernel (so a failure there is the kernel's, not the yardstick's).

Conditions on every builder: the reference's fp32 arithmetic is finite on all rows (values of 6e4 .. 1e5 are ordinary numbers to it);
every folded weight stays below 65 504 (the h2 stream is built); the band 65 504 .. 65 520 holds at most 1 % of the rows; each stratum
the case is built to populate holds at least 5 %; no row lies within 0.05 of a stratum cut (the h2 split moves z_j by 0.016 there)."""
import numpy as np
import pytest
import torch

import _envelope_cases as E


@pytest.mark.parametrize("key", E.ALL_KEYS)
def test_builder_conditions(key):
    c = E.get_case(key)
    for k, v in c.ref32.items():
        assert bool(torch.isfinite(v).all()), (key, k)
        assert bool(torch.isfinite(c.ref64[k]).all()), (key, k)
    wmax = E.max_folded_weight(c.net)
    frac = {s: float((c.stratum == s).mean()) for s in E.STRATA}
    print("envelope case %-22s strata %s  fp32 floor %s  split floor (max) %s  max |w| %.3g" % (
        key, " ".join("%s %.3f" % (s, frac[s]) for s in E.STRATA), " ".join("%s %.1e" % kv for kv in c.floor.items()),
        " ".join("%s %.1e" % (k, float(v.max())) for k, v in c.split.items()), wmax))
    assert wmax < E.F16_MAX, wmax
    assert frac["band"] <= 0.01
    for s in c.uses:
        assert frac[s] >= 0.05, (key, s, frac)
    if key.split("/")[-1] not in ("f", "g", "w"):
        assert E.near_a_cut(c.z) == 0
    if key.split("/")[-1] == "h":
        assert frac["dirty"] == 0.0 and frac["band"] == 0.0


@pytest.mark.parametrize("key", E.ALL_KEYS)
def test_the_reference_fp32_run_meets_every_comparison(key):
    c = E.get_case(key)
    for name, idx in E.arrangements(c).items():
        got = {k: v[idx] for k, v in c.ref32.items()}
        for exact in (False, True):
            problems, any_bad, worst, _ = E.judge(c, idx, got, exact=exact)
            assert not problems and not any_bad, (key, name, exact, problems)


def test_the_probe_is_an_ordinary_neuron_to_the_reference():
    """The issue's figures for S1's SDF net, p = -0.3: the probe moves the SDF by an ordinary amount, the fp32 floor is ~1e-6, and
    the split floor (what 22 bits of a 6e4 activation and the subnormal quantum of 1e-6 weights cost, by the oracle) is of that order."""
    c = E.get_case("sdf/a")
    from iron_amd import scenes
    from oracle import iron_ref as R
    base = scenes.build_networks("S1")["sdf_network"]
    plain = R.sdf_forward({k: v.detach().double() for k, v in base.state_dict().items()}, R.SDFSpec(), c.inputs[0].double())[:, :1]
    moved = float((plain - c.ref64["sdf"]).abs().max())
    print("sdf/a: the probe moves the SDF by up to %.3f; fp32 floor %.2e; split floor up to %.2e" % (moved, c.floor["sdf"],
                                                                                                  float(c.split["sdf"].max())))
    assert 0.01 <= moved <= 2.0
    assert c.floor["sdf"] <= 1e-5
    assert float(c.split["sdf"][c.rows("quiet")].max()) <= 1e-12      # a quiet neuron has nothing to perturb
    assert 1e-8 <= float(c.split["sdf"][c.rows("large")].max()) <= 1e-4
