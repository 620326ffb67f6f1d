"""CPU: the slope bound of the screen's adaptive march (csrc/trace.hip k_sampler_screen: a sample with f1 > delta + L * dz * m proves
the skipped samples up to m positions away positive, L = 2 x max |grad f| over the calibration set) against the CPU emulation of the
march (tools/sampler_stride_margin.py) on S0 / S1 / S3 at 200 x 200 and on two generalised 8 x 256 nets.  L is empirical; this pins
that no skipped sample is non-positive, that the smallest exact value of a skipped sample keeps half the margin, that the slope guard
stays below its threshold (and rises above it with a tenth of L), and what the march saves."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sampler_stride_margin as ST  # noqa: E402
import screen_margin as SM  # noqa: E402

NETS = ["S0", "S1", "S3", "gen0", "gen1"]


@functools.lru_cache(maxsize=None)
def _net(name):
    sd, spec = SM.generalised_net(int(name[3:])) if name.startswith("gen") else SM.scene_net(name)
    return sd, spec, ST.ray_samples(sd, spec, 200)


@functools.lru_cache(maxsize=None)
def _report(name, l_scale=1.0):
    sd, spec, samples = _net(name)
    r = ST.stride_report(sd, spec, 200, l_scale=l_scale, samples=samples)
    print(name, l_scale, r)
    return r


@pytest.mark.parametrize("name", NETS)
def test_no_skipped_sample_is_non_positive(name):
    r = _report(name)
    assert r["strided_passes"] > 0, r
    assert r["skipped_nonpositive"] == 0, r


@pytest.mark.parametrize("name", NETS)
def test_skipped_samples_keep_half_the_margin(name):
    """The rule gives delta minus the screen's error (held under delta / 4 by tests/test_screen_margin.py) when the slope stays under L."""
    r = _report(name)
    assert r["min_exact_skipped"] >= 0.5 * r["delta"], r


@pytest.mark.parametrize("name", NETS)
def test_slope_guard_stays_below_its_threshold(name):
    r = _report(name)
    assert 0.0 < r["guard"] < ST.GUARD, r


@pytest.mark.parametrize("name", NETS)
def test_slope_guard_rises_with_a_tenth_of_the_bound(name):
    r = _report(name, 0.1)
    assert r["guard"] > ST.GUARD, r


@pytest.mark.parametrize("name", NETS)
def test_lane_evaluations(name):
    """Passes x 8 against the stride-1 march's: at most half on the scenes (most of their sampled rays have no root); not more on the
    generalised nets (nearly all their rays have one)."""
    r = _report(name)
    assert r["lane_evals"] <= (0.5 if name.startswith("S") else 1.0) * r["baseline_lane_evals"], r


def test_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iron_amd", "csrc", "trace.hip")).read()
    assert "constexpr float kStrideK = %.1ff;" % ST.K_STRIDE in src
    assert "constexpr float kStrideGuard = %.2ff;" % ST.GUARD in src
    assert "constexpr float kStrideCalibH = 1.0f / %.1ff;" % (1.0 / ST.CALIB_H) in src
    assert "#define IRON_SAMPLER_STRIDE_MAX %d " % ST.STRIDE_MAX in src
