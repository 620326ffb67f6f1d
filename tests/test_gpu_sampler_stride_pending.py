"""GPU: pending rays stride too (csrc/trace.hip k_sampler_screen), and the slope guard has two sources in the resolve.

A ray that has listed an uncertain sample used to march the rest of its range at stride 1; it now strides by the rules of the other
rays.  Nothing that is computed may move: conv, points, sdf, dist, depth and iron_trace_stats are bit-equal between the march as it
is, the march with pending rays on stride 1 (iron_sampler_screen_debug(4, 1): what the previous build did) and the stride-1 march
-- on S0 and S1 at two resolutions and on generalised nets.  On the S0 800 x 800 frame of the benchmark the screen's counts are the
previous build's (resolved 920 833, pending 99 738, overflow 0, screen guard ratio 0.0468) and the screened evaluations fall below its
5 419 268.  The slope guard's resolve-side sources (exact value of a listed sample against its screened predecessor; exact values of
adjacent listed samples) stay below kStrideGuard on the stock scenes, make observations in numbers comparable to the stride-1
passes', and raise the guard on their own (iron_sampler_screen_debug(5, 1) mutes the stride-1 passes' source) under a forced
L = 1e-3, after which the network's next call marches at stride 1 with the stride-1 results.

Measured on one MI355X (stride-1 passes / resolve against the screened predecessor / exact pairs; observations, largest ratio to L):
S0 800 x 800 980 920 / 823 179 / 756 589, 0.0102 / 0.0172 / 0.1535 (with pending rays on stride 1: 2 694 114, 0.1785 from the
passes); S1 800 x 800 760 182 / 335 376 / 299 819, 0.170 / 0.112 / 0.192 (before 2 051 507, 0.268); generalised nets 0.32 / 0.29 /
0.26 and 0.33 / 0.33 / 0.30; forced L = 1e-3 with the passes muted: 0 / 32 193 / 29 082 observations, 0 / 614 / 1 026."""
import ctypes as C

import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, raytrace_camera

pytestmark = pytest.mark.gpu
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")
STRIDE_GUARD = 0.75   # kStrideGuard
ON, PARENT, OFF = "on", "parent", "off"


def _dev():
    return _lib.stream_ptr(torch.device("cuda", 0))


def _counts():
    lib = _lib.load()
    ws = [_lib.current_workspace(torch.device("cuda", 0), "trace")]   # this stream's, not a side stream's of an earlier render
    assert ws[0] is not None
    a, b, d = (C.c_double * 5)(), (C.c_double * 4)(), (C.c_double * 9)()
    _lib.check(lib.iron_trace_screen_counts(ws[0].data_ptr(), a, _dev()))
    _lib.check(lib.iron_trace_stride_counts(ws[0].data_ptr(), b, _dev()))
    _lib.check(lib.iron_trace_stride_detail(ws[0].data_ptr(), d, _dev()))
    return {"screened": a[0], "resolved": a[1], "overflow": a[2], "ratio": a[3], "pending": a[4],
            "passes": b[0], "strided": b[1], "slope": b[2], "adaptive": b[3],
            "stride1_behind": d[0], "stride1_fresh": d[1], "restarts": d[2],
            "obs_march": d[3], "obs_resolve": d[4], "obs_pair": d[5], "slope_march": d[6], "slope_resolve": d[7], "slope_pair": d[8]}


def _trace(sdf, res, mode, mute=False):
    import iron_amd.raytracer as RT
    lib = _lib.load()
    K, W2C = scenes.fixture_camera_matrices(res, res)
    cam = Camera(res, res, K.cuda(), W2C.cuda())
    prev = lib.iron_set_sampler_stride(0 if mode == OFF else 1)
    _lib.check(lib.iron_sampler_screen_debug(4, 1.0 if mode == PARENT else 0.0))
    _lib.check(lib.iron_sampler_screen_debug(5, 1.0 if mute else 0.0))
    old = RT.VERBOSE_MODE
    try:
        RT.VERBOSE_MODE = True
        tr = RayTracer()
        out = raytrace_camera(cam, sdf, tr, max_num_rays=res * res)
        torch.cuda.synchronize()
        cnt = _counts()
    finally:
        RT.VERBOSE_MODE = old
        _lib.check(lib.iron_sampler_screen_debug(4, 0.0))
        _lib.check(lib.iron_sampler_screen_debug(5, 0.0))
        lib.iron_set_sampler_stride(prev)
    return out, dict(tr.last_stats), cnt


def _three(sdf, res, tag):
    """The three marches of one frame; asserts what must hold on every net and returns their counts."""
    runs = {m: _trace(sdf, res, m) for m in (OFF, PARENT, ON)}
    for m in (OFF, PARENT, ON):
        print("pending stride", tag, res, m, runs[m][2], "n_evals", runs[m][1]["n_evals"])
    want, ws, c0 = runs[OFF]
    for m in (PARENT, ON):
        got, gs, c = runs[m]
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (m, k)
        assert gs == ws, (m, gs, ws)
        assert c["adaptive"] == 1, (m, c)
        if c["overflow"] == 0 and c0["overflow"] == 0:   # the screen lists and resolves the same samples (which rays overflow a
            for k in ("resolved", "pending", "ratio"):   # full list, and so what is on it, depends on the order of the waves)
                assert c[k] == c0[k], (m, k, c, c0)
        for k in ("slope", "slope_march", "slope_resolve", "slope_pair"):
            assert c[k] < STRIDE_GUARD, (m, k, c)
        assert c["slope"] == max(c["slope_march"], c["slope_resolve"], c["slope_pair"]), (m, c)
        assert c["stride1_behind"] + c["stride1_fresh"] <= c["passes"] - c["strided"], (m, c)
        assert c["restarts"] <= c["strided"], (m, c)
    assert c0["adaptive"] == 0 and c0["strided"] == 0 and c0["obs_march"] == 0 and c0["obs_resolve"] == 0 and c0["obs_pair"] == 0, c0
    cp, c1 = runs[PARENT][2], runs[ON][2]
    assert c1["screened"] <= cp["screened"] <= c0["screened"], (c0, cp, c1)
    assert c1["passes"] <= cp["passes"], (cp, c1)
    # the resolve-side sources do not depend on the march: one observation per listed sample behind a ray's first, in both
    # (which samples of a ray that overflows the list are on it depends on the order of the waves)
    assert 0 < c1["obs_resolve"] <= c1["resolved"] and 0 < cp["obs_resolve"] <= cp["resolved"], (cp, c1)
    if c1["overflow"] == 0:
        assert c1["obs_resolve"] == cp["obs_resolve"] and c1["obs_pair"] == cp["obs_pair"], (cp, c1)
    assert c1["obs_pair"] <= c1["obs_resolve"], c1
    return c0, cp, c1


@torch.no_grad()
def test_c1_frame_counts():
    """The benchmark's frame.  The previous build's figures (profiles/r06_sampler_stride_ab_c1.txt): 5 419 268 screened evaluations,
    702 698 ray-passes of which 151 312 strided, 920 833 resolved, 99 738 pending, 0 overflows, screen guard ratio 0.0468."""
    sdf = scenes.build_networks("S0")["sdf_network"].cuda()
    c0, cp, c1 = _three(sdf, 800, "S0")
    assert (cp["screened"], cp["passes"], cp["strided"]) == (5419268, 702698, 151312), cp   # the hook marches as the previous build
    for c in (cp, c1):
        assert (c["resolved"], c["pending"], c["overflow"]) == (920833, 99738, 0), c
        assert round(c["ratio"], 4) == 0.0468, c
    assert c1["screened"] < 5419268, c1
    assert c1["strided"] > cp["strided"], (cp, c1)
    assert c1["stride1_behind"] < cp["stride1_behind"], (cp, c1)


@torch.no_grad()
@pytest.mark.parametrize("scene,res", [("S0", 400), ("S1", 400), ("S1", 800)])
def test_pending_stride_is_bit_equal(scene, res):
    sdf = scenes.build_networks(scene)["sdf_network"].cuda()
    c0, cp, c1 = _three(sdf, res, scene)
    assert c0["overflow"] == 0 and cp["overflow"] == 0 and c1["overflow"] == 0, (c0, cp, c1)
    assert c1["strided"] > cp["strided"], (cp, c1)


@torch.no_grad()
@pytest.mark.parametrize("seed", [0, 1])
def test_pending_stride_on_generalised_nets(seed):
    import _nets
    from iron_amd.fields import SDFNetwork
    net = _nets.generalise(_nets.build(SDFNetwork, _nets.sdf_kw("prod"), "prod"), 1000 + seed).cuda()
    _three(net, 256, "gen%d" % seed)


def _status(sdf):
    st = C.c_int32(0)
    _lib.check(_lib.load().iron_net_numeric_status(sdf.hip_net().handle, C.byref(st), _dev()))
    return st.value


@torch.no_grad()
def test_resolve_sources_raise_the_guard_alone():
    """The forced slope bound of tests/test_gpu_sampler_stride.py's guard test (L = 1e-3, far below the network's slope) with the
    stride-1 passes' source muted: the resolve's sources raise the guard in the call that uses the bound, and the network's next
    call marches at stride 1 and gives the stride-1 results.  (The calibrated margin only: with that test's second case, a margin
    of 2e-5, a 256 x 256 frame need not list a single sample, and the resolve has nothing to observe.)"""
    lib = _lib.load()
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    want, ws, _ = _trace(sdf, 256, OFF)
    sdf.invalidate()   # a fresh handle: its own calibration and guards
    assert not _status(sdf) & 16
    _lib.check(lib.iron_sampler_screen_debug(3, 1e-3))
    try:
        _, _, cnt = _trace(sdf, 256, ON, mute=True)
    finally:
        _lib.check(lib.iron_sampler_screen_debug(3, 0.0))
    print("resolve-side guard", cnt)
    assert cnt["adaptive"] == 1 and cnt["obs_march"] == 0 and cnt["slope_march"] == 0.0, cnt
    assert cnt["obs_resolve"] > 0 and cnt["slope_resolve"] > STRIDE_GUARD, cnt
    assert cnt["slope"] > STRIDE_GUARD, cnt
    assert _status(sdf) & 16
    got, gs, cnt2 = _trace(sdf, 256, ON)   # the next call: stride 1
    assert cnt2["adaptive"] == 0 and cnt2["strided"] == 0, cnt2
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws
    lib.iron_net_force_exact(sdf.hip_net().handle, 0)   # clears the status
    assert not _status(sdf) & 16
