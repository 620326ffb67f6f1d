"""GPU: the adaptive march of the sampler's screen (csrc/trace.hip k_sampler_screen) changes nothing.  The march
with the slope bound and the stride-1 march run in one process through iron_set_sampler_stride; conv, points, sdf, dist, depth and
iron_trace_stats must be bit-equal -- on S0 / S1 / S3 frames, through iron_trace_stage(1), in the 8-tile sharded form, with a step
count that is not a multiple of 8, with one above 256 (which must report stride 1), and on generalised 8 x 256 nets.  On S0 the
screened evaluation count must fall.  The slope guard (largest watched slope relative to L) must stay below 0.75 on all of them; a
forced tiny margin and a forced tiny L must raise it, after which the network's next call marches at stride 1."""
import ctypes as C
import sys

import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, raytrace_camera

pytestmark = pytest.mark.gpu
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")
STRIDE_GUARD = 0.75   # kStrideGuard


def _field(scene):
    if scene in ("S0", "S1", "S3"):
        return scenes.build_networks(scene)["sdf_network"].cuda()
    import _hard_fields
    return _hard_fields.build(scene).cuda()


def _dev():
    return _lib.stream_ptr(torch.device("cuda", 0))


def _counts_of(ws):
    lib = _lib.load()
    a, b = (C.c_double * 5)(), (C.c_double * 4)()
    _lib.check(lib.iron_trace_screen_counts(ws.data_ptr(), a, _dev()))
    _lib.check(lib.iron_trace_stride_counts(ws.data_ptr(), b, _dev()))
    return {"screened": a[0], "resolved": a[1], "overflow": a[2], "ratio": a[3], "pending": a[4],
            "passes": b[0], "strided": b[1], "slope": b[2], "adaptive": b[3]}


def _counts():
    ws = _lib.current_workspace(torch.device("cuda", 0), "trace")   # this stream's: a process that rendered edges has a side stream's too
    assert ws is not None
    return _counts_of(ws)


def _trace(sdf, res, stride, max_rays=None, n_steps=128):
    import iron_amd.raytracer as RT
    lib = _lib.load()
    K, W2C = scenes.fixture_camera_matrices(res, res)
    cam = Camera(res, res, K.cuda(), W2C.cuda())
    prev = lib.iron_set_sampler_stride(1 if stride else 0)
    old = RT.VERBOSE_MODE
    try:
        RT.VERBOSE_MODE = True
        tr = RayTracer(n_steps=n_steps)
        out = raytrace_camera(cam, sdf, tr, max_num_rays=max_rays or res * res)
        torch.cuda.synchronize()
        cnt = _counts()
    finally:
        RT.VERBOSE_MODE = old
        lib.iron_set_sampler_stride(prev)
    return out, dict(tr.last_stats), cnt


def _equal(sdf, res, max_rays=None, n_steps=128, adaptive=True):
    want, ws, c0 = _trace(sdf, res, False, max_rays, n_steps)
    got, gs, c1 = _trace(sdf, res, True, max_rays, n_steps)
    print("stride counts", res, n_steps, "off", c0, "on", c1, "n_evals", gs["n_evals"])
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws, (gs, ws)
    assert c0["screened"] > 0 and c0["adaptive"] == 0 and c0["strided"] == 0, c0
    assert c1["adaptive"] == (1 if adaptive else 0), c1
    if adaptive:
        assert c1["slope"] < STRIDE_GUARD, c1
        assert c1["screened"] <= c0["screened"], (c0, c1)
    else:
        assert c1["strided"] == 0 and c1["screened"] == c0["screened"] and c1["passes"] == c0["passes"], (c0, c1)
    return c0, c1


@torch.no_grad()
@pytest.mark.parametrize("scene,res", [("S0", 800), ("S1", 800), ("S3", 400), ("bumpy03_s1", 256)])
def test_adaptive_march_is_bit_equal(scene, res):
    """bumpy03_s1 (tests/_hard_fields.py: bumpy(0.03, 1)): a third of its sampled rays have overshot and are sampled over
    [min_dis, acc_dis], hundreds change sign three and more times."""
    sdf = _field(scene)
    c0, c1 = _equal(sdf, res)
    assert c1["strided"] > 0, c1
    assert c1["overflow"] == 0, c1
    if scene == "S0":   # most of its sampled rays have no root: the screened evaluations fall to well under two thirds
        assert c1["screened"] < 0.67 * c0["screened"], (c0, c1)


@torch.no_grad()
@pytest.mark.parametrize("seed", [0, 1])
def test_adaptive_march_on_generalised_nets(seed):
    import _nets
    from iron_amd.fields import SDFNetwork
    net = _nets.generalise(_nets.build(SDFNetwork, _nets.sdf_kw("prod"), "prod"), 1000 + seed).cuda()
    _equal(net, 256)


@torch.no_grad()
def test_step_counts():
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    _equal(sdf, 256, n_steps=100)                    # not a multiple of the block
    _equal(sdf, 256, n_steps=250)                    # the largest indices the continuation word carries
    _equal(sdf, 192, n_steps=264, adaptive=False)    # above 256: stride 1


@torch.no_grad()
def test_stage_sampler():
    from iron_amd.raytracer import SDFHandle, intersect_sphere
    lib = _lib.load()
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    K, W2C = scenes.fixture_camera_matrices(128, 128)
    cam = Camera(128, 128, K.cuda(), W2C.cuda())
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    h = SDFHandle(sdf)
    outs, cnts = [], []
    for stride in (0, 1):
        prev = lib.iron_set_sampler_stride(stride)
        try:
            outs.append([x.clone() for x in RayTracer().ray_sampler(h, ro[hit], rd[hit], near[hit], far[hit])])
            torch.cuda.synchronize()
            cnts.append(_counts())
        finally:
            lib.iron_set_sampler_stride(prev)
    print("stage(1) stride counts", cnts)
    assert cnts[0]["adaptive"] == 0 and cnts[1]["adaptive"] == 1 and cnts[1]["strided"] > 0, cnts   # iron_trace_stage(1) marched adaptively
    assert cnts[1]["slope"] < STRIDE_GUARD, cnts
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@torch.no_grad()
def test_sharded_render_is_bit_equal(monkeypatch):
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    from iron_amd.sharding import RECORD, render_emulated
    lib = _lib.load()
    nets = {k: v.cuda() for k, v in scenes.build_networks("S0").items()}
    fn = make_render_fn(GGXColocatedRenderer(use_cuda=True))
    K, W2C = scenes.fixture_camera_matrices(256, 256)
    cam = Camera(256, 256, K.cuda(), W2C.cuda())
    # the sharded phases allocate their trace workspaces with torch.empty: keep them, to read the counts afterwards
    bufs, empty = [], torch.empty

    def keep(*a, **kw):
        t = empty(*a, **kw)
        if t.dtype == torch.uint8 and t.is_cuda and t.numel() > 4096 and sys._getframe(1).f_code.co_filename.endswith("raytracer.py"):
            bufs.append(t)
        return t
    res = []
    for stride in (0, 1):
        prev = lib.iron_set_sampler_stride(stride)
        try:
            bufs.clear()
            with monkeypatch.context() as m:
                m.setattr(torch, "empty", keep)
                b, _, _ = render_emulated(8, [cam], nets["sdf_network"], nets, fn, RayTracer, fill_holes=False, handle_edges=False)
            torch.cuda.synchronize()
            assert bufs
            cs = [_counts_of(x) for x in bufs]
            assert max(c["adaptive"] for c in cs) == stride, cs   # the sharded phases marched adaptively / did not
            assert max(c["slope"] for c in cs) < STRIDE_GUARD, cs
            res.append(b)
        finally:
            lib.iron_set_sampler_stride(prev)
    for k, _ in RECORD:
        assert torch.equal(res[0][k][0], res[1][k][0]), k


def _status(sdf):
    st = C.c_int32(0)
    _lib.check(_lib.load().iron_net_numeric_status(sdf.hip_net().handle, C.byref(st), _dev()))
    return st.value


@torch.no_grad()
@pytest.mark.parametrize("delta", [0.0, 2e-5])
def test_guard_puts_the_march_on_stride_1(delta):
    """A forced slope bound far below the network's slope (alone, and with a forced margin far below the screen's error) raises the
    guard in the call that uses it; the network's next call marches at stride 1 and gives the stride-1 results."""
    lib = _lib.load()
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    want, ws, _ = _trace(sdf, 256, False)
    sdf.invalidate()   # a fresh handle: its own calibration and guards
    assert not _status(sdf) & 16
    _lib.check(lib.iron_sampler_screen_debug(3, 1e-3))
    _lib.check(lib.iron_sampler_screen_debug(0, delta))
    try:
        _, _, cnt = _trace(sdf, 256, True)
    finally:
        _lib.check(lib.iron_sampler_screen_debug(3, 0.0))
        _lib.check(lib.iron_sampler_screen_debug(0, 0.0))
    print("guard", delta, cnt)
    assert cnt["adaptive"] == 1 and cnt["slope"] > STRIDE_GUARD, cnt
    assert _status(sdf) & 16
    got, gs, cnt2 = _trace(sdf, 256, True)   # the next call: stride 1 (with the forced margin unscreened: the screen's own guard rose too)
    assert cnt2["adaptive"] == 0 and cnt2["strided"] == 0, cnt2
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws
    lib.iron_net_force_exact(sdf.hip_net().handle, 0)   # clears the status
    assert not _status(sdf) & 16
