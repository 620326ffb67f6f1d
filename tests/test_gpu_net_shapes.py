"""MLP parity beyond the geometric init, at every network shape iron_net_create accepts (tests/_nets.py lists them).

Every network here is generalise()d: hidden biases, the skip layer's sin/cos columns and weight_g != |v| all carry weight, so a
pack or kernel that dropped, misplaced or swapped one of them fails (tests/test_net_shapes_oracle.py checks on the CPU that each
of those groups moves the oracle's output by >= 50x the tolerance applied here).  Each case is compared with the fp64 oracle on
the same parameters, on the default core and pinned to the exact-fp32 core, at row counts around the 32-row tile and the
128-row h2 group.  Shapes the kernels do not serve must refuse with IronError at the first call -- never return numbers.
"""

import numpy as np
import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.fields import NeRF, RenderingNetwork, SDFNetwork
from oracle import iron_ref as R
from oracle import neus_ref as NR
from oracle import train_ref as T

import _nets as N
from _nets import _compare_param_grads
from _shading_oracle import scene as _scene

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 33, 127, 129, 4099)
TOL_SDF = 1e-5       # SDF values, features, materials, NeRF outputs: rel-L2 (as tests/test_gpu_fields.py, test_gpu_render.py)
TOL_GRAD = 2e-5      # get_all's d sdf / dx (as tests/test_gpu_render.py)
TOL_PARAM = 2e-5     # parameter and input gradients of the backward passes (tests/test_gpu_train.py: 2e-4; measured <= 4e-6 here)
ROW_FACTOR = 10      # n <= 129: the worst row's error (relative to the batch's rms row) may exceed the rel-L2 bound by this much
CORES = ("default", "exact")

_cache = {}


def _check(tag, out, ref, tol, rms):
    """rel-L2 of `out` against `ref`, with the denominator held at or above sqrt(n) x `rms` (the rms row norm of the whole 4099-row
    reference): a batch of one point next to the zero level set has |sdf| ~ 0, and the error of a kernel is set by the size of
    its operands, not of that one result.  n <= 129: the worst single row, against `rms`, too."""
    out = out.detach().cpu().numpy() if torch.is_tensor(out) else out
    ref = ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    assert np.all(np.isfinite(out)), tag
    a, b = out.reshape(len(ref), -1).astype(np.float64), ref.reshape(len(ref), -1).astype(np.float64)
    r = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), np.sqrt(len(b)) * rms))
    rr = float(np.linalg.norm(a - b, axis=1).max() / rms) if len(b) <= 129 else 0.0
    key = tag.split(" ")[0]
    _check.worst[key] = max(_check.worst.get(key, 0.0), r)
    assert r <= tol, (tag, r)
    assert rr <= ROW_FACTOR * tol, (tag, "worst row", rr)
    return r


def _rms(ref):
    b = ref.detach().double().reshape(len(ref), -1)
    return float(b.pow(2).sum(dim=1).mean().sqrt())


_check.worst = {}


def _sdf_case(name):
    if ("sdf", name) not in _cache:
        kw = N.sdf_kw(name)
        net = N.build(SDFNetwork, kw, name)
        sd, spec = N.sd64(net), N.sdf_spec(kw)
        x = N.sdf_inputs(max(ROWS), N.seed_of(name) + 1, kw["scale"])
        full = R.sdf_forward(sd, spec, x.double())
        y, feat, grad = R.sdf_get_all(sd, spec, x.double())
        _cache[("sdf", name)] = (kw, net.cuda(), sd, spec, x, full, (y, feat, grad))
    return _cache[("sdf", name)]


def _get_all_forward_mode(net, x, want_feat):
    """iron_sdf_get_all with a NULL workspace: the forward-mode kernels (include/iron_hip.h), in process."""
    n = x.shape[0]
    y = torch.empty((n, 1), device="cuda")
    feat = torch.empty((n, net.d_out - 1), device="cuda") if want_feat else None
    grad = torch.empty((n, 3), device="cuda")
    h = net.hip_net()
    _lib.check(_lib.load().iron_sdf_get_all(h.handle, x.data_ptr(), n, y.data_ptr(), _lib.ptr(feat), grad.data_ptr(), None, 0,
                                            _lib.stream_ptr(x.device)))
    return y, feat, grad


@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("name", list(N.SDF_SHAPES))
@torch.no_grad()
def test_sdf_entry_points(name, core):
    """sdf / forward (iron_sdf_forward, out_cols 1 and d_out), get_all (reverse kernel with a workspace, forward-mode kernel
    without), get_sdf_and_gradient, against the fp64 oracle."""
    kw, net, sd, spec, x, full, (y, feat, grad) = _sdf_case(name)
    s_sdf, s_full, s_feat, s_grad = _rms(full[:, :1]), _rms(full), _rms(feat) if kw["d_out"] > 1 else 0.0, _rms(grad)
    net.force_exact(core == "exact")
    try:
        for n in ROWS:
            xs = x[:n].cuda()
            tag = "sdf:%s/%s n=%d" % (name, core, n)
            _check(tag, net.sdf(xs), full[:n, :1], TOL_SDF, s_sdf)
            _check(tag + " forward", net(xs), full[:n], TOL_SDF, s_full)
            y2, f2, g2 = net.get_all(xs, is_training=False)
            _check(tag + " get_all sdf", y2, y[:n], TOL_SDF, s_sdf)
            if kw["d_out"] > 1:
                _check(tag + " get_all feat", f2, feat[:n], TOL_SDF, s_feat)
            _check(tag + " get_all grad", g2, grad[:n], TOL_GRAD, s_grad)
            y3, f3, g3 = _get_all_forward_mode(net, xs, kw["d_out"] > 1)
            _check(tag + " get_all(fwd) sdf", y3, y[:n], TOL_SDF, s_sdf)
            if f3 is not None:
                _check(tag + " get_all(fwd) feat", f3, feat[:n], TOL_SDF, s_feat)
            _check(tag + " get_all(fwd) grad", g3, grad[:n], TOL_GRAD, s_grad)
            y4, g4 = net.get_sdf_and_gradient(xs)
            _check(tag + " sdf_and_grad sdf", y4, y[:n], TOL_SDF, s_sdf)
            _check(tag + " sdf_and_grad grad", g4, grad[:n], TOL_GRAD, s_grad)
        torch.cuda.synchronize()
        print("sdf %-10s %-7s worst: %s" % (name, core, {k: "%.1e" % v for k, v in _check.worst.items() if k.startswith("sdf:%s/%s" % (name, core))}))
    finally:
        net.force_exact(False)


@pytest.mark.parametrize("name", list(N.SDF_SHAPES))
def test_sdf_backward(name):
    """get_all(is_training=True) to second order (sdf, feature, and the gradient's eikonal term) vs fp64 torch autograd over the
    oracle; the shapes without a backward must refuse."""
    kw, net, _, spec, x, _, _ = _sdf_case(name)
    n = 301
    gen = torch.Generator().manual_seed(3)
    a, B, Cc = torch.randn(n, 1, generator=gen), torch.randn(n, kw["d_out"] - 1, generator=gen) * 0.1, torch.randn(n, 3, generator=gen)
    if name in N.SDF_NO_BACKWARD:
        y2, _, _ = net.get_all(x[:n].cuda(), is_training=True)
        with pytest.raises(_lib.IronError):
            (y2 * a.cuda()).sum().backward()
        for p in net.parameters():
            p.grad = None
        return
    sd = T.leaf_state(N.sd64(net))
    y, f, g = T.sdf_get_all_train(sd, spec, x[:n].double())
    ((y * a.double()).sum() + (f * B.double()).sum() + (g * Cc.double()).sum() + (g.norm(dim=-1) - 1).pow(2).sum()).backward()
    y2, f2, g2 = net.get_all(x[:n].cuda(), is_training=True)
    ((y2 * a.cuda()).sum() + (f2 * B.cuda()).sum() + (g2 * Cc.cuda()).sum() + (g2.norm(dim=-1) - 1).pow(2).sum()).backward()
    w = _compare_param_grads(net, sd, TOL_PARAM, "sdf backward %s" % name)
    print("sdf backward %-10s worst rel-L2 %.2e (%s)" % (name, w, getattr(_compare_param_grads, "last", "")))


@pytest.mark.parametrize("name", list(N.SDF_REFUSED))
def test_sdf_refused_shapes(name):
    torch.manual_seed(0)
    net = SDFNetwork(**N.sdf_kw(name)).cuda()
    with pytest.raises(_lib.IronError, match="unsupported"):
        with torch.no_grad():
            net.sdf(torch.zeros(4, 3, device="cuda"))


def _render_case(name):
    if ("render", name) not in _cache:
        kw = N.RENDER_SHAPES[name]
        net = N.build(RenderingNetwork, kw, name)
        sd, spec = N.sd64(net), N.render_spec(kw)
        ins = N.render_inputs(max(ROWS), N.seed_of(name) + 1)
        use_view = kw["mode"] in ("idr", "no_normal")
        ref = R.rendering_forward(sd, spec, ins[0].double(), ins[1].double(), ins[2].double() if use_view else None, ins[3].double())
        _cache[("render", name)] = (kw, net.cuda(), spec, ins, use_view, ref)
    return _cache[("render", name)]


@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("name", list(N.RENDER_SHAPES))
@torch.no_grad()
def test_render_forward(name, core):
    kw, net, _, ins, use_view, ref = _render_case(name)
    s_ref = _rms(ref)
    net.force_exact(core == "exact")
    try:
        for n in ROWS:
            g = [v[:n].cuda() for v in ins]
            out = net(g[0], g[1], g[2] if use_view else None, g[3])
            _check("render:%s/%s n=%d" % (name, core, n), out, ref[:n], TOL_SDF, s_ref)
    finally:
        net.force_exact(False)


@pytest.mark.parametrize("name", list(N.RENDER_SHAPES))
def test_render_backward(name):
    """Parameter and input gradients of RenderingNetwork.forward vs fp64 torch autograd over the oracle (4099 rows: the split-K
    weight-gradient path with a ragged tail)."""
    kw, net, spec, ins, use_view, _ = _render_case(name)
    n = 4099
    sd = T.leaf_state(N.sd64(net))
    up = torch.randn(n, kw["d_out"], generator=torch.Generator().manual_seed(11))
    # rows whose forward passes within rounding of a ReLU kink (a handful per batch) carry no loss: on them fp32 and fp64 may
    # take different sides of the kink, and one such element flips a whole unit's gradient
    kink = N.relu_kink_rows(N.sd64(net), spec, *(v[:n].double() for v in ins[:2]), ins[2][:n].double() if use_view else None,
                            ins[3][:n].double())
    up[kink] = 0
    cpu_in = [v[:n].double().requires_grad_(True) for v in ins]
    out = R.rendering_forward(sd, spec, cpu_in[0], cpu_in[1], cpu_in[2] if use_view else None, cpu_in[3])
    (out * up.double()).sum().backward()
    gpu_in = [v[:n].cuda().requires_grad_(True) for v in ins]
    out2 = net(gpu_in[0], gpu_in[1], gpu_in[2] if use_view else None, gpu_in[3])
    (out2 * up.cuda()).sum().backward()
    w = _compare_param_grads(net, sd, TOL_PARAM, "render backward %s" % name)
    for i, what in enumerate(("points", "normals", "view_dirs", "features")):
        if cpu_in[i].grad is None:
            assert gpu_in[i].grad is None or float(gpu_in[i].grad.abs().max()) == 0.0, what
            continue
        r = N.rel(gpu_in[i].grad.cpu().numpy(), cpu_in[i].grad.numpy())
        w = max(w, r)
        assert r <= TOL_PARAM, (name, what, r)
    print("render backward %-24s worst rel-L2 %.2e (%s), %d kink rows" % (name, w, getattr(_compare_param_grads, "last", ""), int(kink.sum())))


@pytest.mark.parametrize("name", list(N.RENDER_REFUSED))
def test_render_refused_shapes(name):
    kw = N.RENDER_REFUSED[name]
    torch.manual_seed(0)
    net = RenderingNetwork(**kw).cuda()
    p, nrm, view, feat = (v[:8].cuda() for v in N.render_inputs(8, 0))
    with pytest.raises(_lib.IronError, match="unsupported"):
        with torch.no_grad():
            net(p, nrm, view if kw["mode"] in ("idr", "no_normal") else None, feat)


def _nerf_case(name):
    if ("nerf", name) not in _cache:
        kw = N.nerf_kw(name)
        net = N.build(NeRF, kw, name)
        sd, spec = N.sd64(net), N.nerf_spec(kw)
        pts, views = N.nerf_inputs(max(ROWS), N.seed_of(name) + 1)
        alpha, rgb = NR.nerf_forward(sd, spec, pts.double(), views.double())
        _cache[("nerf", name)] = (kw, net.cuda(), spec, pts, views, alpha, rgb)
    return _cache[("nerf", name)]


@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("name", list(N.NERF_SHAPES))
@torch.no_grad()
def test_nerf_forward(name, core):
    kw, net, _, pts, views, alpha, rgb = _nerf_case(name)
    s_a, s_r = _rms(alpha), _rms(rgb)
    net.force_exact(core == "exact")
    try:
        for n in ROWS:
            a2, r2 = net(pts[:n].cuda(), views[:n].cuda())
            _check("nerf:%s/%s n=%d alpha" % (name, core, n), a2, alpha[:n], TOL_SDF, s_a)
            _check("nerf:%s/%s n=%d rgb" % (name, core, n), r2, rgb[:n], TOL_SDF, s_r)
    finally:
        net.force_exact(False)


@pytest.mark.parametrize("name", list(N.NERF_SHAPES))
def test_nerf_backward(name):
    kw, net, spec, pts, views, _, _ = _nerf_case(name)
    n = 4099
    gen = torch.Generator().manual_seed(6)
    ua, ur = torch.randn(n, 1, generator=gen), torch.randn(n, 3, generator=gen)
    sd = T.leaf_state(N.sd64(net))
    alpha, rgb = NR.nerf_forward(sd, spec, pts[:n].double(), views[:n].double())
    ((alpha * ua.double()).sum() + (rgb * ur.double()).sum()).backward()
    a2, r2 = net(pts[:n].cuda(), views[:n].cuda())
    ((a2 * ua.cuda()).sum() + (r2 * ur.cuda()).sum()).backward()
    w = _compare_param_grads(net, sd, TOL_PARAM, "nerf backward %s" % name)
    print("nerf backward %-10s worst rel-L2 %.2e (%s)" % (name, w, getattr(_compare_param_grads, "last", "")))


@pytest.mark.parametrize("name", list(N.NERF_REFUSED))
def test_nerf_refused_shapes(name):
    torch.manual_seed(0)
    net = NeRF(**N.nerf_kw(name)).cuda()
    pts, views = N.nerf_inputs(8, 0)
    with pytest.raises(_lib.IronError, match="unsupported"):
        with torch.no_grad():
            net(pts.cuda(), views.cuda())


# ---- tracing and shading ---------------------------------------------------------------------------------------------------------
FLIP_SDF = 5e-3      # a mask flip is allowed only on a ray that passes within this fp64 |sdf| of the surface (a grazing ray)
MIN_HITS = 0.3       # hit fraction the generalised scenes keep (S1: ~0.34): a perturbation that lost the surface fails here


def _ray_min_abs_sdf(sd64, o, d, near, far, m=1024):
    t = near[:, None] + (far - near)[:, None] * torch.linspace(0, 1, m, dtype=torch.float64)[None]
    p = o[:, None].double() + d[:, None].double() * t[..., None]
    return R.sdf_forward(sd64, R.SDFSpec(), p.reshape(-1, 3))[:, 0].reshape(-1, m).abs().min(dim=1).values


@pytest.mark.parametrize("variant,exact", [("s1", False), ("s1", True), ("mat2_6", False)])
@torch.no_grad()
def test_render_camera_generalised(variant, exact):
    """render_camera at 48x48 on generalised networks (trace, get_all, materials, fused GGX shading) vs the oracle's trace and
    render on the same parameters.  "mat2_6" reaches the fused shading path with runtime material depths."""
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    nets, sc = _scene(variant)
    K, W2C = scenes.fixture_camera_matrices(48, 48)
    ref = R.render_camera(sc, R.CameraSpec(48, 48, K, W2C))
    gpu = {k: m.cuda() for k, m in nets.items()}
    gpu["sdf_network"].force_exact(exact)
    cam = Camera(48, 48, K.cuda(), W2C.cuda())
    fn = make_render_fn(GGXColocatedRenderer(use_cuda=True))
    res = render_camera(cam, gpu["sdf_network"], RayTracer(), gpu, fn, fill_holes=False, handle_edges=False)
    conv, rconv = res["convergent_mask"].cpu().numpy(), ref["convergent_mask"].numpy()
    assert rconv.mean() >= MIN_HITS, rconv.mean()
    flip = conv != rconv
    if flip.any():
        o, d = ref["ray_o"].reshape(-1, 3)[flip.reshape(-1)], ref["ray_d"].reshape(-1, 3)[flip.reshape(-1)]
        _, near, far = R.intersect_sphere(o, d, 1.0)
        ms = _ray_min_abs_sdf({k: v.double() for k, v in sc.sdf_sd.items()}, o, d, near.double(), far.double())
        print("flipped pixels: min |sdf| along their rays", ms.numpy())
        assert float(ms.max()) <= FLIP_SDF
    both = conv & rconv
    dd = np.abs(res["distance"].cpu().numpy() - ref["distance"].numpy())[both]
    # shading (get_all, materials, GGX) against the oracle at the kernel's own hit points: the colour is then not the tracer's
    # hit-point difference (checked above through the mask and the distance) amplified by the specular lobe
    mine = {k: res[k].cpu() for k in ("convergent_mask", "points", "ray_o", "ray_d")}
    R.render_normal_and_color(sc, mine)
    r = N.rel(res["color"].cpu().numpy()[conv], mine["color"].numpy()[conv])
    print("%s exact=%s: hits %d flips %d colour rel-L2 %.2e |d distance| p99 %.2e" % (variant, exact, int(both.sum()), int(flip.sum()), r,
                                                                                     np.percentile(dd, 99)))
    assert int(flip.sum()) <= 2
    assert r <= 2e-5   # measured <= 7e-6 (the tracer-independent shading error)
    assert np.percentile(dd, 99) <= 2e-4
    for k in ("normal", "diffuse_albedo", "specular_albedo", "specular_roughness"):
        assert N.rel(res[k].cpu().numpy()[conv], mine[k].numpy()[conv]) <= 1e-4, k
