"""GPU: the dense sampler's screen (csrc/trace.hip k_sampler_screen) changes nothing.  The screened and the unscreened sampler run in
one process through iron_set_sampler_screen; conv, points, sdf, dist and iron_trace_stats must be bit-equal -- at 800x800 (S0, S1),
on S3, on generalised 8 x 256 nets, through iron_trace_stage(1), in the 8-tile sharded form, with silhouette edges, and with the
resolve list forced to overflow.  The guard ratio (largest |f_screen - f_h2| / delta over the resolved samples) is reported and must
stay <= 0.25; a forced tiny delta must raise the guard, after which the network's next call is the unscreened one."""
import ctypes as C
import sys

import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, raytrace_camera

pytestmark = pytest.mark.gpu
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")


def _field(scene):
    if scene in ("S0", "S1", "S3"):
        return scenes.build_networks(scene)["sdf_network"].cuda()
    import _hard_fields   # bumpy03_s1 = bumpy(0.03, 1): overshoot and multi-root rays by the hundred
    return _hard_fields.build(scene).cuda()


def _counts_of(ws):
    out = (C.c_double * 5)()
    _lib.check(_lib.load().iron_trace_screen_counts(ws.data_ptr(), out, _lib.stream_ptr(torch.device("cuda", 0))))
    return {"screened": out[0], "resolved": out[1], "overflow": out[2], "ratio": out[3], "pending": out[4]}


def _counts():
    ws = _lib.current_workspace(torch.device("cuda", 0), "trace")   # this stream's: a process that rendered edges has a side stream's too
    assert ws is not None
    return _counts_of(ws)


def _screened_anywhere(extra=()):
    """Largest screened count over every trace workspace of the process (+ `extra` buffers): did the screen run at all?"""
    return max(_counts_of(b)["screened"] for b in [b for k, b in _lib._workspaces.items() if k[2] == "trace"] + list(extra))


def _trace(sdf, res, screen, max_rays=None):
    import iron_amd.raytracer as RT
    lib = _lib.load()
    K, W2C = scenes.fixture_camera_matrices(res, res)
    cam = Camera(res, res, K.cuda(), W2C.cuda())
    prev = lib.iron_set_sampler_screen(1 if screen else 0)
    old = RT.VERBOSE_MODE
    try:
        RT.VERBOSE_MODE = True
        tr = RayTracer()
        out = raytrace_camera(cam, sdf, tr, max_num_rays=max_rays or res * res)
        torch.cuda.synchronize()
        cnt = _counts()
    finally:
        RT.VERBOSE_MODE = old
        lib.iron_set_sampler_screen(prev)
    return out, dict(tr.last_stats), cnt


def _equal(sdf, res, max_rays=None):
    want, ws, _ = _trace(sdf, res, False, max_rays)
    got, gs, cnt = _trace(sdf, res, True, max_rays)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws, (gs, ws)
    print("screen counts", res, cnt, "n_evals", gs["n_evals"])
    assert cnt["screened"] > 0
    return cnt


@torch.no_grad()
@pytest.mark.parametrize("scene,res", [("S0", 800), ("S1", 800), ("S3", 400), ("bumpy03_s1", 256)])
def test_screened_sampler_is_bit_equal(scene, res):
    sdf = _field(scene)
    cnt = _equal(sdf, res)
    assert cnt["ratio"] <= 0.25, cnt
    assert cnt["overflow"] == 0, cnt


@torch.no_grad()
@pytest.mark.parametrize("seed", [0, 1])
def test_screened_sampler_on_generalised_nets(seed):
    import _nets
    from iron_amd.fields import SDFNetwork
    net = _nets.generalise(_nets.build(SDFNetwork, _nets.sdf_kw("prod"), "prod"), 1000 + seed).cuda()
    cnt = _equal(net, 256)
    assert cnt["ratio"] <= 0.25, cnt


@torch.no_grad()
def test_forced_overflow_is_bit_equal():
    lib = _lib.load()
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    _lib.check(lib.iron_sampler_screen_debug(1, 64.0))
    try:
        cnt = _equal(sdf, 256)
    finally:
        _lib.check(lib.iron_sampler_screen_debug(1, 0.0))
    assert cnt["overflow"] > 0, cnt


@torch.no_grad()
def test_stage_sampler_and_split_form():
    import iron_amd.raytracer as RT
    from iron_amd.raytracer import SDFHandle, intersect_sphere
    lib = _lib.load()
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    K, W2C = scenes.fixture_camera_matrices(128, 128)
    cam = Camera(128, 128, K.cuda(), W2C.cuda())
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    h = SDFHandle(sdf)
    outs = []
    for screen in (0, 1):
        prev = lib.iron_set_sampler_screen(screen)
        try:
            outs.append([x.clone() for x in RayTracer().ray_sampler(h, ro[hit], rd[hit], near[hit], far[hit])])
            torch.cuda.synchronize()
            if screen:
                assert _counts()["screened"] > 0   # iron_trace_stage(1) took the screened sampler
        finally:
            lib.iron_set_sampler_screen(prev)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    prev_split = lib.iron_set_trace_split(3)
    try:
        _equal(sdf, 160)
    finally:
        lib.iron_set_trace_split(prev_split)


@torch.no_grad()
def test_sharded_and_edges_are_bit_equal(monkeypatch):
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    from iron_amd.raytracer import render_camera
    from iron_amd.sharding import RECORD, render_emulated
    lib = _lib.load()
    nets = {k: v.cuda() for k, v in scenes.build_networks("S0").items()}
    fn = make_render_fn(GGXColocatedRenderer(use_cuda=True))
    K, W2C = scenes.fixture_camera_matrices(256, 256)
    cam = Camera(256, 256, K.cuda(), W2C.cuda())
    # the sharded phases allocate their trace workspaces with torch.empty: keep them, to read the screen's counts afterwards
    bufs, empty = [], torch.empty

    def keep(*a, **kw):
        t = empty(*a, **kw)
        if t.dtype == torch.uint8 and t.is_cuda and t.numel() > 4096 and sys._getframe(1).f_code.co_filename.endswith("raytracer.py"):
            bufs.append(t)
        return t
    res = []
    for screen in (0, 1):
        prev = lib.iron_set_sampler_screen(screen)
        try:
            a = render_camera(cam, nets["sdf_network"], RayTracer(), nets, fn, fill_holes=True, handle_edges=True)
            torch.cuda.synchronize()
            if screen:
                assert _screened_anywhere() > 0   # render_camera with edges took the screened sampler
            bufs.clear()
            with monkeypatch.context() as m:
                m.setattr(torch, "empty", keep)
                b, _, _ = render_emulated(8, [cam], nets["sdf_network"], nets, fn, RayTracer, fill_holes=False, handle_edges=False)
            torch.cuda.synchronize()
            if screen:
                assert bufs and max(_counts_of(x)["screened"] for x in bufs) > 0   # and so did the sharded phases
            res.append((a, b))
        finally:
            lib.iron_set_sampler_screen(prev)
    for k in res[0][0]:
        if torch.is_tensor(res[0][0][k]):
            assert torch.equal(res[0][0][k], res[1][0][k]), k
    for k, _ in RECORD:
        assert torch.equal(res[0][1][k][0], res[1][1][k][0]), k


@torch.no_grad()
def test_guard_turns_the_screen_off():
    lib = _lib.load()
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    want, ws, _ = _trace(sdf, 256, False)
    sdf.invalidate()   # a fresh handle: its own calibration and guard
    # a margin below the screen's typical error: the samples it leaves uncertain are resolved with |f1 - f| well above delta / 2
    _lib.check(lib.iron_sampler_screen_debug(0, 2e-5))
    try:
        _, _, cnt = _trace(sdf, 256, True)
    finally:
        _lib.check(lib.iron_sampler_screen_debug(0, 0.0))
    assert cnt["ratio"] > 0.5, cnt
    st = C.c_int32(0)
    h = sdf.hip_net()
    _lib.check(lib.iron_net_numeric_status(h.handle, C.byref(st), _lib.stream_ptr(torch.device("cuda", 0))))
    assert st.value & 8, st.value
    got, gs, cnt2 = _trace(sdf, 256, True)
    assert cnt2["screened"] == 0, cnt2
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws
