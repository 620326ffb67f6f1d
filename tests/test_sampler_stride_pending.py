"""CPU: pending rays stride too (csrc/trace.hip k_sampler_screen) -- the emulation of the whole march, to each ray's first
certainly-negative screened sample (tools/sampler_stride_margin.py march_rays), on S0 / S1 / S3 at 200 x 200 and two generalised
8 x 256 nets.  With pending rays striding, the samples the stride-1 code classifies as uncertain (listed for the resolve) or
certainly negative (the ray's end) are exactly those of the all-stride-1 march, ray by ray; the march saves passes over the one
that kept pending rays on stride 1; and the slope guard's two resolve-side sources make observations that do not depend on the
march, stay below kStrideGuard on the scenes and rise above it with a tenth of L.

The exact-pair source has no allowance for the evaluation's own rounding.  On gen0 the emulation reads 1.82 from it: two rays
whose whole range is 2.5e-6 wide (samples 2e-8 apart, L * dz = 9e-7), where the fp32 rounding of the exact value (1.7e-6) is all
the difference there is.  That is noise, not slope, and a raised guard costs speed, never a result; the generalised nets are
therefore held to the classification and the counts only, as is the kernel on the GPU (tests/test_gpu_sampler_stride_pending.py,
where the same nets read 0.26 at 256 x 256)."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sampler_stride_margin as ST  # noqa: E402
import screen_margin as SM  # noqa: E402

SCENES = ["S0", "S1", "S3"]
NETS = SCENES + ["gen0", "gen1"]


from test_sampler_stride_margin import _net  # noqa: E402  (the same nets and samples, evaluated once per session)


@functools.lru_cache(maxsize=None)
def _report(name, l_scale=1.0):
    sd, spec, samples = _net(name)
    r = ST.pending_report(sd, spec, 200, l_scale=l_scale, samples=samples)
    print(name, l_scale, r)
    return r


@pytest.mark.parametrize("name", NETS)
def test_stride_1_classification_is_the_all_stride_1_marchs(name):
    r = _report(name)
    assert r["pending_rays"] > 0 and r["listed_samples"] > 0, r
    assert r["class_mismatch_rays"] == 0 and r["class_mismatch_rays_before"] == 0, r


@pytest.mark.parametrize("name", NETS)
def test_pending_rays_save_passes(name):
    r = _report(name)
    assert r["passes_after"] < r["passes_before"] < r["passes_stride1"], r
    assert r["stride1_behind_after"] < r["stride1_behind_before"], r
    assert r["stride1_fresh_after"] == r["stride1_fresh_before"], r   # rays that have listed nothing march as before
    if name in SCENES:   # most of their pending rays graze the surface: at least a tenth of all passes goes
        assert r["passes_after"] <= 0.9 * r["passes_before"], r


@pytest.mark.parametrize("name", NETS)
def test_resolve_side_sources_do_not_depend_on_the_march(name):
    r = _report(name)
    assert r["obs_resolve_after"] == r["obs_resolve_before"] > 0, r
    assert r["guard_resolve_after"] == r["guard_resolve_before"], r
    # (a pass lists its uncertain samples in order: a pair straddling two passes is not adjacent on the list, so the pair count
    # moves by the few pairs whose halves a restart puts into different passes)
    assert abs(r["obs_pair_after"] - r["obs_pair_before"]) <= 0.001 * r["obs_pair_before"], r
    # the guard keeps observations in numbers comparable to those the stride-1 passes lose
    assert r["obs_resolve_after"] + r["obs_pair_after"] + r["obs_march_after"] >= 0.5 * r["obs_march_before"], r


@pytest.mark.parametrize("name", SCENES)
def test_every_source_stays_below_the_threshold_on_the_scenes(name):
    r = _report(name)
    for k in ("guard_march_after", "guard_resolve_after", "guard_pair_after"):
        assert 0.0 < r[k] < ST.GUARD, (k, r)


@pytest.mark.parametrize("name", SCENES)
def test_resolve_side_sources_rise_with_a_tenth_of_the_bound(name):
    r = _report(name, 0.1)
    assert max(r["guard_resolve_after"], r["guard_pair_after"]) > ST.GUARD, r
