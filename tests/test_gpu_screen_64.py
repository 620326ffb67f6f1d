"""GPU: the screen at 64 samples per wave (csrc/mlp_h2.h: sdf_hidden_stack_h1 with two point tiles, one weight fragment feeding two
MFMAs; csrc/trace.hip: k_sampler_screen on 8 ray slots of 8 samples).

  * iron_sdf_screen_forward's 64-sample form gives the 32-sample form's values bit for bit (iron_sampler_screen_debug(2, 1) selects
    the 32-sample form), on S0 / S1 / S3 and a generalised net, at a point count that fills no whole wave;
  * the screened sampler stays bit-equal to the unscreened one when its list of rays is not a multiple of 8 ray slots;
  * and when the resolve list is forced to overflow."""
import ctypes as C

import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, raytrace_camera

pytestmark = pytest.mark.gpu
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    x = x / x.norm(dim=1, keepdim=True) * torch.rand(n, 1, generator=g) ** (1 / 3)
    # a few points outside the unit ball and on the axes as well
    extra = torch.tensor([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, -1.2, 0.3], [0.7, 0.7, 0.7]])
    return torch.cat([x, extra], 0).float().contiguous()


def _screen(net, x, point_tiles):
    lib = _lib.load()
    xd = x.cuda().contiguous()
    out = torch.full((x.shape[0],), float("nan"), device="cuda")
    _lib.check(lib.iron_sampler_screen_debug(2, 1.0 if point_tiles == 1 else 0.0))
    try:
        _lib.check(lib.iron_sdf_screen_forward(net.hip_net().handle, xd.data_ptr(), x.shape[0], out.data_ptr(),
                                               _lib.stream_ptr(xd.device)))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.iron_sampler_screen_debug(2, 0.0))
    return out.cpu()


def _bit_equal(net, x):
    f32 = _screen(net, x, 1)
    f64 = _screen(net, x, 2)
    assert torch.isfinite(f32).all()
    assert torch.equal(f64.view(torch.int32), f32.view(torch.int32)), int((f64 != f32).sum())


@torch.no_grad()
@pytest.mark.parametrize("scene", ["S0", "S1", "S3"])
def test_64_sample_screen_is_the_32_sample_screen(scene):
    net = scenes.build_networks(scene)["sdf_network"].cuda()
    _bit_equal(net, _points(100_003, 0))


@torch.no_grad()
def test_64_sample_screen_on_a_generalised_net():
    import _nets
    from iron_amd.fields import SDFNetwork
    net = _nets.generalise(_nets.build(SDFNetwork, _nets.sdf_kw("prod"), "prod"), 1000).cuda()
    _bit_equal(net, _points(70_001, 1))


def _counts():
    ws = [_lib.current_workspace(torch.device("cuda", 0), "trace")]   # this stream's, not a side stream's of an earlier render
    assert ws[0] is not None
    out = (C.c_double * 5)()
    _lib.check(_lib.load().iron_trace_screen_counts(ws[0].data_ptr(), out, _lib.stream_ptr(torch.device("cuda", 0))))
    return {"screened": out[0], "resolved": out[1], "overflow": out[2], "ratio": out[3], "pending": out[4]}


def _trace(sdf, res, screen):
    import iron_amd.raytracer as RT
    lib = _lib.load()
    K, W2C = scenes.fixture_camera_matrices(res, res)
    cam = Camera(res, res, K.cuda(), W2C.cuda())
    prev = lib.iron_set_sampler_screen(1 if screen else 0)
    old = RT.VERBOSE_MODE
    try:
        RT.VERBOSE_MODE = True
        tr = RayTracer()
        out = raytrace_camera(cam, sdf, tr, max_num_rays=res * res)
        torch.cuda.synchronize()
        cnt = _counts()
    finally:
        RT.VERBOSE_MODE = old
        lib.iron_set_sampler_screen(prev)
    return out, dict(tr.last_stats), cnt


def _equal(sdf, res):
    want, ws, _ = _trace(sdf, res, False)
    got, gs, cnt = _trace(sdf, res, True)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws, (gs, ws)
    assert cnt["screened"] > 0, cnt
    return gs, cnt


@torch.no_grad()
def test_sampler_list_not_a_multiple_of_the_ray_slots():
    sdf = scenes.build_networks("S0")["sdf_network"].cuda()
    odd = []
    for res in (61, 75, 97, 131):
        st, cnt = _equal(sdf, res)
        print("res", res, "n_sampler", st["n_sampler"], cnt)
        if st["n_sampler"] % 8:
            odd.append(res)
    assert odd, "no resolution gave a sampler list that is not a multiple of 8"


@torch.no_grad()
def test_forced_overflow_at_64_samples_per_wave():
    lib = _lib.load()
    sdf = scenes.build_networks("S0")["sdf_network"].cuda()
    _lib.check(lib.iron_sampler_screen_debug(1, 40.0))
    try:
        st, cnt = _equal(sdf, 199)
    finally:
        _lib.check(lib.iron_sampler_screen_debug(1, 0.0))
    print("n_sampler", st["n_sampler"], cnt)
    assert cnt["overflow"] > 0, cnt
