"""GPU: the dense sampler's screen reads a weight stream of its own, the h1 stream (csrc/pack_h2.hip: the hi pieces of the h2
fragments, written by the same pack launches; csrc/mlp_h2.h: sdf_hidden_stack_h1 walks it in head slots and pair slots).

  * iron_sdf_screen_forward agrees with the CPU emulation of the screen (tools/screen_margin.py) on the calibration set and on points
    of the tracer's unit ball, for S0 / S1 / S3 and a generalised net: the typical point to within fp32 summation-order noise, so a
    tile read from the wrong place in the stream (an error of the order of the SDF itself on most points) fails;
  * the stream follows a re-pack: after the parameters change, the screen's values are the new network's and the screened trace is
    still bit-equal to the unscreened one;
  * a network that has no h2 stream (a folded weight beyond fp16's range) has no h1 stream either: it traces unscreened, with the
    same result as the screen switched off, and iron_sdf_screen_forward refuses it."""
import ctypes as C
import os
import sys

import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, raytrace_camera

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import screen_margin as SM  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")
# |device - emulation|: the kernel and the emulation differ in fp32 summation order (and in the last ulps of softplus), which now and
# then moves an fp16-rounded activation by one ulp; a point where that happens early can differ by up to ~3e-3 (generalised net), but
# the median stays at 2e-7 .. 2.3e-5 (measured on S0 / S1 / S3 / gen0).  A misplaced tile moves the median to the SDF's own scale.
MEDIAN_TOL = 1e-4
MAX_TOL = 1e-2


def _points(n=100_000, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    x = x / x.norm(dim=1, keepdim=True) * torch.rand(n, 1, generator=g) ** (1 / 3)
    return torch.cat([SM.calibration_points(), x.float()], 0).contiguous()


def _screen(net, x):
    lib = _lib.load()
    xd = x.cuda().contiguous()
    out = torch.empty(x.shape[0], device="cuda")
    rc = lib.iron_sdf_screen_forward(net.hip_net().handle, xd.data_ptr(), x.shape[0], out.data_ptr(), _lib.stream_ptr(xd.device))
    torch.cuda.synchronize()
    return rc, out.cpu()


def _state(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _agrees(net, x, label):
    import oracle.iron_ref as R
    rc, f1 = _screen(net, x)
    _lib.check(rc)
    want = SM.screen_forward(_state(net), R.SDFSpec(), x)
    d = (f1 - want).abs()
    print(label, "max |device - emulation| %.3e, median %.3e" % (float(d.max()), float(d.median())))
    assert torch.isfinite(f1).all()
    assert float(d.median()) <= MEDIAN_TOL, (label, float(d.median()))
    assert float(d.max()) <= MAX_TOL, (label, float(d.max()))


def _counts():
    ws = [_lib.current_workspace(torch.device("cuda", 0), "trace")]   # this stream's, not a side stream's of an earlier render
    assert ws[0] is not None
    out = (C.c_double * 5)()
    _lib.check(_lib.load().iron_trace_screen_counts(ws[0].data_ptr(), out, _lib.stream_ptr(torch.device("cuda", 0))))
    return {"screened": out[0], "resolved": out[1], "overflow": out[2], "ratio": out[3]}


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


def _bit_equal(sdf, res):
    want, ws, _ = _trace(sdf, res, False)
    got, gs, cnt = _trace(sdf, res, True)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert gs == ws, (gs, ws)
    return cnt


@torch.no_grad()
@pytest.mark.parametrize("scene", ["S0", "S1", "S3"])
def test_screen_forward_matches_the_emulation(scene):
    net = scenes.build_networks(scene)["sdf_network"].cuda()
    _agrees(net, _points(), scene)


@torch.no_grad()
def test_screen_forward_matches_the_emulation_on_a_generalised_net():
    import _nets
    from iron_amd.fields import SDFNetwork
    net = _nets.generalise(_nets.build(SDFNetwork, _nets.sdf_kw("prod"), "prod"), 1000).cuda()
    _agrees(net, _points(seed=1), "gen0")


@torch.no_grad()
def test_the_screen_stream_follows_a_repack():
    net = scenes.build_networks("S1")["sdf_network"].cuda()
    x = _points(20_000, seed=2)
    _agrees(net, x, "before")
    cnt = _bit_equal(net, 256)
    assert cnt["screened"] > 0, cnt
    h0 = net.hip_net().handle
    _, f_before = _screen(net, x)
    # change every hidden layer a little (in place: torch bumps the version counter, the next call re-packs)
    g = torch.Generator().manual_seed(3)
    for l in range(1, 8):
        lin = getattr(net, "lin%d" % l)
        p = lin.weight_v if getattr(lin, "has_weight_norm", False) else lin.weight
        p.mul_((1.0 + 0.02 * torch.randn(p.shape, generator=g)).to(p.device))
    assert net.hip_net().handle != h0
    _agrees(net, x, "after")
    _, f_after = _screen(net, x)
    assert float((f_after - f_before).abs().median()) > 10 * MEDIAN_TOL   # the screen sees the new weights
    cnt = _bit_equal(net, 256)
    assert cnt["screened"] > 0, cnt
    assert cnt["ratio"] <= 0.25, cnt


@torch.no_grad()
def test_a_net_without_h2_stream_traces_unscreened():
    net = scenes.build_networks("S1")["sdf_network"].cuda()
    want, ws, _ = _trace(net, 256, False)
    # a feature row of the last layer beyond fp16's range: the h2 pack is dropped (and with it the h1 stream), the SDF row is untouched
    last = net.lin8
    if getattr(last, "has_weight_norm", False):
        last.weight_g[5] = 1.0e7
    else:
        last.weight[5].mul_(1.0e7)
    rc, _ = _screen(net, _points(1000))
    assert rc != 0, "no h1 stream: iron_sdf_screen_forward must refuse the network"
    got, gs, cnt = _trace(net, 256, True)
    assert cnt["screened"] == 0, cnt
    off, os_, _ = _trace(net, 256, False)
    for k in KEYS:
        assert torch.equal(got[k], off[k]), k
    assert gs == os_
    # the exact core traces the same surface as the h2 core did before the change (the SDF row did not change)
    same = (got["convergent_mask"] == want["convergent_mask"]).float().mean().item()
    assert same >= 0.999, same
    both = got["convergent_mask"] & want["convergent_mask"]
    assert float((got["points"][both] - want["points"][both]).abs().max()) <= 1e-3
