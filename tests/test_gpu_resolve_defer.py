"""GPU: the resolve's two rounds (csrc/trace.hip k_resolve_list / k_screen_resolve) change nothing.

The samples a ray lists behind its first listed one with f1 < 0 are deferred; round 1 evaluates the others, round 2 the deferred
ones that still lie in front of the ray's first negative sample.  With the deferral on and off (iron_set_resolve_defer) conv,
points, sdf, distance and depth are bit-equal, iron_trace_stats and the `resolved` count are equal -- on S0, S1 and the hard fields
bumpy(0.03, 1) and gen0 (multi-root rays, reversed ranges) at 64 x 64 in chunks of 1000 rays.  A call that collects statistics
evaluates every listed sample (round 2 takes all deferred ones: the counts and guard maxima the suite pins are those of the whole
list), so the comparison is made a second time with statistics off: that is the path a render takes, and the only one on which
round 2 runs on demand.  On that path round 1 evaluates at most 0.65 of the listed samples on S0 and S1 and round 2 next to none; a
forced margin below the screen's error makes round 2 run, with the outputs of the one-round resolve under the same margin; and a
list forced to overflow leaves every ray, overflowed or not, with the outputs of the unforced run.

Every run takes a fresh network handle (own calibration, no guard raised), so that a guard one run raises cannot turn the next
run's screen off.

Measured on one MI355X, statistics off (listed / round 1 / round 2): S0 5 847 / 2 716 (0.465) / 190 (0.032); S1 2 506 / 1 306 (0.521)
/ 27 (0.011); bumpy(0.03, 1) 3 060 / 2 287 / 31; gen0 (its list overflows: 8 192 entries, ~645 rays marched again) 8 192 / 4 858 / 74;
forced margin 2e-4 on S1 at 400 x 400: 4 603 / 4 497 / 27, screen guard ratio 1.20; forced overflow: 64 listed, ~365 rays overflow."""
import ctypes as C
import functools

import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, raytrace_camera

pytestmark = pytest.mark.gpu
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")
RES = 64
CHUNK = 1000
FIELDS = ("S0", "S1", "bumpy03_s1", "gen0")
# Round 2 on the scenes: a ray's deferred samples come back only when the exact value of its first listed sample with f1 < 0 is not
# negative.  The CPU emulation of the screen (tools/screen_margin.py screen_forward, the stride-1 march of
# tools/sampler_stride_margin.py, 200 x 200, calibrated margin) sends p = 2.7 % of S0's listed samples to round 2 (1 543 of 57 708,
# from 230 rays) and 1.4 % of S1's (328 of 24 051, 73 rays): whole rays of m = 7 / 5 samples.  The kernel's rounding is not the
# emulation's, so twice p is allowed, and a 64 x 64 view lists few samples: three standard deviations of a share of n samples that
# come m at a time, 3 sqrt(p m / n), on top.
ROUND2_EMULATED = {"S0": (0.027, 7.0), "S1": (0.014, 5.0)}


@functools.lru_cache(maxsize=None)
def _field(name):
    if name in ("S0", "S1"):
        return scenes.build_networks(name)["sdf_network"].cuda(), 0.0
    import _hard_fields as HF
    return HF.build(name).cuda(), HF.yaw_of(name)


def _counts():
    lib, dev = _lib.load(), torch.device("cuda", 0)
    ws = _lib.current_workspace(dev, "trace")
    assert ws is not None
    a, b = (C.c_double * 5)(), (C.c_double * 4)()
    _lib.check(lib.iron_trace_screen_counts(ws.data_ptr(), a, _lib.stream_ptr(dev)))
    _lib.check(lib.iron_trace_resolve_counts(ws.data_ptr(), b, _lib.stream_ptr(dev)))
    return {"screened": a[0], "resolved": a[1], "overflow": a[2], "ratio": a[3], "pending": a[4],
            "round1": b[0], "round2": b[1], "list1": b[2], "list2": b[3]}


def _trace(name, defer, stats, res=RES):
    import iron_amd.raytracer as RT
    lib = _lib.load()
    net, yaw = _field(name)
    net.invalidate()
    K, W2C = scenes.fixture_camera_matrices(res, res, yaw)
    cam = Camera(res, res, K.cuda(), W2C.cuda())
    prev = lib.iron_set_resolve_defer(1 if defer else 0)
    old = RT.VERBOSE_MODE
    try:
        RT.VERBOSE_MODE = stats
        tr = RayTracer()
        tr.last_stats = None
        out = raytrace_camera(cam, net, tr, max_num_rays=CHUNK)
        torch.cuda.synchronize()
        cnt = _counts()
    finally:
        RT.VERBOSE_MODE = old
        lib.iron_set_resolve_defer(prev)
    assert (tr.last_stats is not None) == stats
    return {k: out[k].clone() for k in KEYS}, (dict(tr.last_stats) if stats else None), cnt


def _check_counts(cnt, defer, stats):
    assert cnt["screened"] > 0, cnt                       # the screen ran
    assert cnt["round1"] + cnt["round2"] <= cnt["resolved"], cnt
    assert cnt["round1"] == cnt["list1"] or not defer, cnt
    assert cnt["round2"] == cnt["list2"], cnt
    if not defer:
        assert cnt["round1"] == cnt["resolved"] and cnt["round2"] == 0 and cnt["list1"] == 0, cnt
    elif stats:                                            # the audit: every listed sample is evaluated
        assert cnt["round1"] + cnt["round2"] == cnt["resolved"], cnt


@functools.lru_cache(maxsize=None)
def _runs(name):
    """The four runs of a field: (deferral, statistics) -> (outputs, iron_trace_stats, counts)."""
    runs = {(d, s): _trace(name, d, s) for s in (True, False) for d in (False, True)}
    for (d, s), (_, _, cnt) in runs.items():
        print("resolve defer %-10s defer %d stats %d" % (name, d, s), cnt)
    return runs


@torch.no_grad()
@pytest.mark.parametrize("name", FIELDS)
def test_outputs_stats_and_resolved_are_equal_with_statistics(name):
    runs = _runs(name)
    (want, ws, c0), (got, gs, c1) = runs[(False, True)], runs[(True, True)]
    _check_counts(c0, False, True)
    _check_counts(c1, True, True)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws, (gs, ws)
    assert c1["pending"] > 0 and c0["pending"] > 0, (c0, c1)
    if c0["overflow"] == 0 and c1["overflow"] == 0:   # (which rays overflow a full list depends on the order of the waves: gen0's does)
        assert c1["pending"] == c0["pending"], (c0, c1)
        assert c1["resolved"] == c0["resolved"] > 0, (c0, c1)
        assert c1["ratio"] == c0["ratio"], (c0, c1)   # the audit sees every listed sample


@torch.no_grad()
@pytest.mark.parametrize("name", FIELDS)
def test_outputs_and_resolved_are_equal_without_statistics(name):
    """The product path: round 2 on demand."""
    runs = _runs(name)
    (want, _, c0), (got, _, c1) = runs[(False, False)], runs[(True, False)]
    _check_counts(c0, False, False)
    _check_counts(c1, True, False)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(got[k], runs[(False, True)][0][k]), k   # ... and of the runs with statistics
    assert c1["pending"] > 0 and c0["pending"] > 0, (c0, c1)
    if c0["overflow"] == 0 and c1["overflow"] == 0:
        assert c1["pending"] == c0["pending"], (c0, c1)
        assert c1["resolved"] == c0["resolved"] > 0, (c0, c1)
        assert c1["round1"] < c1["resolved"], c1                   # something was deferred


@torch.no_grad()
@pytest.mark.parametrize("name", ("S0", "S1"))
def test_round_1_share_on_the_scenes(name):
    _, _, cnt = _runs(name)[(True, False)]
    share1, share2 = cnt["round1"] / cnt["resolved"], cnt["round2"] / cnt["resolved"]
    print("resolve defer %s: round 1 %d (%.3f of resolved %d), round 2 %d (%.4f)" % (name, cnt["round1"], share1, cnt["resolved"], cnt["round2"], share2))
    assert cnt["overflow"] == 0, cnt
    assert share1 <= 0.65, cnt
    p, m = ROUND2_EMULATED[name]
    assert share2 <= 2.0 * p + 3.0 * (p * m / cnt["resolved"]) ** 0.5, cnt


@torch.no_grad()
def test_round_2_runs_when_the_screen_calls_signs_wrongly():
    """A forced margin below the screen's error (tests/test_gpu_sampler_screen.py's guard test forces the same way): samples the
    screen calls negative are not, and their rays' deferred samples come back in round 2.  That test's 2e-5 leaves no ray with two
    listed samples, so nothing is ever deferred (the CPU emulation at 200 x 200: 96 listed samples on 96 rays); 2e-4 is still below
    the screen's largest error next to the surface (2.5e-4 in the emulation, median 4e-5) and lists runs of samples on grazing
    rays: 34 deferred there, 7 of them on the 4 rays whose first screened negative is wrong.  400 x 400 has four times the rays."""
    lib = _lib.load()
    _lib.check(lib.iron_sampler_screen_debug(0, FORCED_DELTA))
    try:
        want, _, c0 = _trace("S1", False, False, FORCED_RES)
        got, _, c1 = _trace("S1", True, False, FORCED_RES)
    finally:
        _lib.check(lib.iron_sampler_screen_debug(0, 0.0))
    print("resolve defer forced delta: one round", c0, "two rounds", c1)
    _check_counts(c0, False, False)
    _check_counts(c1, True, False)
    assert c1["round2"] > 0, c1
    assert c1["round1"] + c1["round2"] < c1["resolved"], c1   # ... on demand: other deferred samples stayed unevaluated
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k


FORCED_DELTA = 2e-4
FORCED_RES = 400


@torch.no_grad()
def test_forced_overflow_leaves_every_ray_alone():
    lib = _lib.load()
    want = _runs("S1")[(False, False)][0]
    _lib.check(lib.iron_sampler_screen_debug(1, 64.0))
    try:
        runs = [_trace("S1", d, s) for s in (False, True) for d in (False, True)]
    finally:
        _lib.check(lib.iron_sampler_screen_debug(1, 0.0))
    for (got, _, cnt), (d, s) in zip(runs, [(d, s) for s in (False, True) for d in (False, True)]):
        print("resolve defer forced overflow defer %d stats %d" % (d, s), cnt)
        _check_counts(cnt, d, s)
        assert cnt["overflow"] > 0, cnt
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (d, s, k)
    assert runs[2][1] == runs[3][1], (runs[2][1], runs[3][1])   # iron_trace_stats, one round against two
    assert runs[3][1] == _runs("S1")[(True, True)][1]            # ... and against the list that did not overflow
