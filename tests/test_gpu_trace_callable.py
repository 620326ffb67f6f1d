"""GPU: the callable tracer (iron_amd.raytracer.SDFCallable, csrc/trace_any.hip) against the oracle's restatement of
models/raytracer.py:45-220, BIT FOR BIT.

The tracer's own arithmetic is a handful of separately rounded fp32 products and sums, and the evaluations come from the caller's
function, so with a field whose value has identical bits on the CPU and on the GPU the whole trace must be identical: the masks with
torch.equal, the float outputs as int32 views (NaN payloads included).  The fields below are closures over fp32 tensors that use only
+ - * minimum abs where -- one correctly rounded operation per torch kernel on either device -- and every test first asserts that
its field IS bit-equal on both devices at a few thousand points: a failure of that assertion points at the field, not the tracer.

Rays: the fixture camera at 48 x 48 (2 304 rays) through intersect_sphere, tracer defaults.  With q(x, c, r) = 0.5 |x - c|^2 - 0.5 r^2
(a distance that undershoots: sphere tracing crawls and leaves rays for the sampler):
    slow    = q(x, 0, 0.5)                                   converged 540, unfinished 1 140: bracketed root 676, no root 464
    two     = 3 min(q(x, (-0.35, 0, 0.3), 0.3), q(x, (0.3, 0.1, -0.3), 0.35))
                                                             unfinished 193: bracketed 125, no root 68; overshoot (s < 0) 92
    two_nan = two, NaN where 0.05 < y < 0.06                 130 NaN outputs
(counts measured with the oracle on the CPU; the tests assert >= 50 per category they rely on, on the oracle's side).  Every
bisection of these traces runs 7 iterations (asserted on the oracle's side too): the widest bracket of a call, a 127th of its
ray's sampling interval, lies in (0.0064, 0.0128] and halves until it is <= 1e-4.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import iron_ref as R
from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, SDFCallable, SDFHandle, intersect_sphere, raytrace_camera, raytrace_pixels

from _util import golden, oracle_scene, t

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _q(x, c, r):
    dx, dy, dz = x[:, 0] - c[0], x[:, 1] - c[1], x[:, 2] - c[2]
    return (dx * dx + dy * dy + dz * dz) * 0.5 - 0.5 * r * r


def slow(x):
    return _q(x, (0.0, 0.0, 0.0), 0.5)


def two(x):
    return torch.minimum(_q(x, (-0.35, 0.0, 0.3), 0.3), _q(x, (0.3, 0.1, -0.3), 0.35)) * 3.0


def two_nan(x):
    v = two(x)
    y = x[:, 1]
    return torch.where((y > 0.05) & (y < 0.06), torch.full_like(v, NAN), v)


FIELDS = {"slow": slow, "two": two, "two_nan": two_nan}


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype)
    diff = _bits(got) != _bits(want)
    assert not bool(diff.any()), "%s: %d of %d values differ in bits" % (what, int(diff.sum()), diff.numel())


def _same_result(got, want, what):
    assert got["convergent_mask"].dtype == torch.bool
    assert torch.equal(got["convergent_mask"].cpu(), want["convergent_mask"]), what + ": convergent_mask"
    for k in ("points", "sdf", "distance"):
        _same_bits(got[k], want[k], "%s: %s" % (what, k))


@functools.lru_cache(maxsize=None)
def _rays():
    """(device rays, the same tensors on the CPU): ray_o, ray_d, near, far, hit."""
    K, W2C = scenes.fixture_camera_matrices(48, 48)
    cam = Camera(48, 48, K.cuda(), W2C.cuda())
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(o, d, 1.0)
    dev = (o, d, near, far, hit)
    return dev, tuple(x.cpu() for x in dev)


def _field_is_bit_equal(f):
    (o, d, near, far, _), _ = _rays()
    g = torch.Generator().manual_seed(7)
    x = torch.cat([torch.rand(3000, 3, generator=g) * 2.4 - 1.2, (o + d * (0.5 * (near + far)).unsqueeze(-1)).cpu()[:2000]]).contiguous()
    _same_bits(f(x.cuda()), f(x), "the field itself, CPU against GPU")


class _Counting:
    def __init__(self, f):
        self.f, self.calls = f, []

    def __call__(self, x):
        self.calls.append(int(x.shape[0]))
        return self.f(x)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's trace of a field on the CPU, computed once and left alone: result, categories, evaluation count."""
    _, (o, d, near, far, hit) = _rays()
    f = _Counting(FIELDS[name])
    stats = {}
    ref = R.raytracer_forward(f, o, d, near, far, hit, R.TracerParams(), stats)
    conv, unf, p, s, tt = R.sphere_tracing(FIELDS[name], o, d, near, far, hit, R.TracerParams())
    cat = {"sphere_conv": int(conv.sum()), "unfinished": int(unf.sum()), "overshoot": int((unf & (s < 0)).sum()),
           "root": int((ref["convergent_mask"] & unf).sum()), "no_root": int((~ref["convergent_mask"] & unf).sum()),
           "nan_out": int(torch.isnan(ref["sdf"]).sum()), "bisect_iters": list(stats["bisect_iters"]), "n_sampler": stats["n_sampler"]}
    return ref, cat, sum(f.calls), (conv, unf, p, s, tt)


@pytest.mark.parametrize("name", ["slow", "two", "two_nan"])
def test_whole_tracer_bit_for_bit(name):
    f = FIELDS[name]
    _field_is_bit_equal(f)
    (o, d, near, far, hit), _ = _rays()
    ref, cat, _, _ = _oracle(name)
    print("   %s: oracle categories %s" % (name, cat))
    need = {"slow": ("sphere_conv", "root", "no_root"), "two": ("overshoot", "root", "no_root"), "two_nan": ("nan_out",)}[name]
    for c in need:
        assert cat[c] >= 50, (name, c, cat)
    assert cat["bisect_iters"] == [7], cat
    tr = RayTracer()
    out = tr(SDFCallable(f), o, d, near, far, hit, collect_stats=True)
    torch.cuda.synchronize()
    _same_result(out, ref, name)
    assert tr.last_stats["n_sampler"] == cat["n_sampler"] and tr.last_stats["n_bisect"] == cat["root"], (tr.last_stats, cat)
    assert tr.last_stats["n_bisect_iters"] == 7


@pytest.mark.parametrize("n_steps", [9, 100])
def test_other_step_counts_bit_for_bit(n_steps):
    """The row reduction walks a row 64 samples at a time: a row shorter than one wave, and one that ends inside its second pass."""
    _field_is_bit_equal(two)
    (o, d, near, far, hit), (co, cd, cnear, cfar, chit) = _rays()
    stats = {}
    ref = R.raytracer_forward(two, co, cd, cnear, cfar, chit, R.TracerParams(n_steps=n_steps), stats)
    tr = RayTracer(n_steps=n_steps)
    out = tr(SDFCallable(two), o, d, near, far, hit, collect_stats=True)
    _same_result(out, ref, "n_steps=%d" % n_steps)
    unfinished = _oracle("two")[3][1]          # sphere tracing does not depend on n_steps
    roots = int((ref["convergent_mask"] & unfinished).sum())
    assert roots >= 50 and int((~ref["convergent_mask"] & unfinished).sum()) >= 50, roots
    assert tr.last_stats["n_sampler"] == stats["n_sampler"] and tr.last_stats["n_bisect"] == roots
    assert tr.last_stats["n_bisect_iters"] == stats["bisect_iters"][0]


def test_stages_bit_for_bit():
    f = two
    _field_is_bit_equal(f)
    (o, d, near, far, hit), (co, cd, cnear, cfar, chit) = _rays()
    prm = R.TracerParams()
    tr, h = RayTracer(), SDFCallable(f)
    _, _, _, (rconv, runf, rp, rs, rt) = _oracle("two")

    conv, unf, p, s, tt = tr.sphere_tracing(h, o, d, near, far, hit)
    assert torch.equal(conv.cpu(), rconv) and torch.equal(unf.cpu(), runf)
    _same_bits(p, rp, "sphere_tracing points")
    _same_bits(s, rs, "sphere_tracing sdf")
    _same_bits(tt, rt, "sphere_tracing distance")

    m = runf
    assert int(m.sum()) >= 100
    pos = (rs[m] > 0.0).float()
    s_min = pos * rt[m] + (1.0 - pos) * cnear[m]
    s_max = pos * cfar[m] + (1.0 - pos) * rt[m]
    rroot, rsp, rss, rst, n_iter = R.ray_sampler(f, co[m], cd[m], s_min.clone(), s_max.clone(), prm)
    assert n_iter == 7 and int(rroot.sum()) >= 50 and int((~rroot).sum()) >= 50
    root, sp, ss, st = tr.ray_sampler(h, co[m].cuda(), cd[m].cuda(), s_min.cuda(), s_max.cuda())
    assert root.dtype == torch.bool and torch.equal(root.cpu(), rroot)
    _same_bits(sp, rsp, "ray_sampler points")
    _same_bits(ss, rss, "ray_sampler sdf")
    _same_bits(st, rst, "ray_sampler distance")

    # rootfind on hand-made brackets around the oracle's roots; two entries are no brackets (f_low = -1): they open no loop of
    # their own but the shared loop still moves them
    oo, dd = co[m][rroot].contiguous(), cd[m][rroot].contiguous()
    d_lo, d_hi = rst[rroot] - 0.013, rst[rroot] + 0.011
    f_lo, f_hi = f(oo + dd * d_lo.unsqueeze(-1)), f(oo + dd * d_hi.unsqueeze(-1))
    f_lo[:2] = -1.0
    assert int(((f_lo > 0) & (f_hi < 0)).sum()) >= 50
    want_p, want_d, want_f, it = R.rootfind(f, f_lo.clone(), f_hi.clone(), d_lo.clone(), d_hi.clone(), oo, dd, prm)
    assert it >= 7
    keep = [x.clone() for x in (f_lo, f_hi, d_lo, d_hi)]
    args = [x.cuda() for x in (f_lo, f_hi, d_lo, d_hi)]
    got_p, got_d, got_f = tr.rootfind(h, *args, oo.cuda(), dd.cuda())
    _same_bits(got_p, want_p, "rootfind p_mid")
    _same_bits(got_d, want_d, "rootfind d_mid")
    _same_bits(got_f, want_f, "rootfind f_mid")
    for a, k in zip(args, keep):   # the caller's brackets are left alone
        _same_bits(a, k, "rootfind argument")


def test_evaluation_accounting():
    _field_is_bit_equal(two)
    (o, d, near, far, hit), _ = _rays()
    ref, cat, ref_evals, _ = _oracle("two")
    n = o.shape[0]
    f = _Counting(two)
    tr = RayTracer()
    out = tr(SDFCallable(f), o, d, near, far, hit, collect_stats=True)
    _same_result(out, ref, "default max_num_pts")
    assert sum(f.calls) == ref_evals == tr.last_stats["n_evals"], (sum(f.calls), ref_evals, tr.last_stats)
    assert f.calls[0] == n and len(f.calls) == tr.last_stats["n_calls"]
    # the reference's own count: n + the unfinished lists + 128 per sampled ray + (7 + 1) per bisected ray
    sampler_and_bisect = 128 * cat["n_sampler"] + 8 * cat["root"]
    assert ref_evals > n + sampler_and_bisect
    assert f.calls[-8:] == [cat["root"]] * 8 and f.calls[-9] == 128 * cat["n_sampler"]

    g = _Counting(two)
    tr2 = RayTracer(max_num_pts=1000)
    out2 = tr2(SDFCallable(g), o, d, near, far, hit)
    _same_result(out2, ref, "max_num_pts=1000")
    assert sum(g.calls) == ref_evals
    k = len(f.calls) - 9                       # the sphere-tracing calls are the same list
    assert g.calls[:k] == f.calls[:k]
    sampler_calls = g.calls[k:-8]
    assert len(sampler_calls) > 1 and sum(sampler_calls) == 128 * cat["n_sampler"]
    assert max(sampler_calls) <= 1000 and all(c % 128 == 0 for c in sampler_calls), sampler_calls
    with pytest.raises(_lib.IronError):        # whole rays per call: fewer points than one ray's samples is refused, not exceeded
        RayTracer(max_num_pts=100)(SDFCallable(two), o, d, near, far, hit)


def test_a_real_network_through_the_opaque_path():
    """S1's SDFNetwork on the 64 x 64 C0 crop, evaluated by iron_sdf_forward through SDFCallable, against the oracle's trace of the
    same weights: the bounds tests/test_gpu_trace.py puts on the fused tracer."""
    g = golden("g67_S1_c0.npz")
    nets = scenes.build_networks("S1")
    sc = oracle_scene(nets)
    sdf = nets["sdf_network"].cuda()
    cam = Camera(int(g["W"]), int(g["H"]), t(g["K"]).cuda(), t(g["W2C"]).cuda())
    assert cam.W == 64 and cam.H == 64
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(o, d, 1.0)
    out = RayTracer()(SDFCallable(lambda x: sdf(x)[..., 0]), o, d, near, far, hit)
    ref = R.raytracer_forward(sc.sdf_fn, o.cpu(), d.cpu(), near.cpu(), far.cpu(), hit.cpu())
    conv, rconv = out["convergent_mask"].cpu().numpy(), ref["convergent_mask"].numpy()
    n = conv.size
    flips = int((conv != rconv).sum())
    both = conv & rconv
    dd = np.abs(out["distance"].cpu().numpy() - ref["distance"].numpy())[both].max()
    dp = np.abs(out["points"].cpu().numpy() - ref["points"].numpy())[both].max()
    ds = np.abs(out["sdf"].cpu().numpy()[both]).max()
    print("   flips %d / %d, max |d distance| %.3g, |d point| %.3g, |sdf| %.3g, hits %d" % (flips, n, dd, dp, ds, int(both.sum())))
    assert int(both.sum()) > 500
    assert flips <= max(1, n // 1000), "mask flips %d / %d" % (flips, n)
    assert dd <= 2e-4 and dp <= 2e-4 and ds <= 1e-4, (dd, dp, ds)


def test_interface_edges():
    _field_is_bit_equal(two)
    (o, d, near, far, hit), (co, cd, cnear, cfar, chit) = _rays()
    ref, _, _, _ = _oracle("two")
    n = o.shape[0]
    tr = RayTracer()

    e = torch.zeros(0, 3, device="cuda")
    out0 = tr(SDFCallable(two), e, e, e[:, 0], e[:, 0], torch.zeros(0, dtype=torch.bool, device="cuda"))
    assert out0["points"].shape == (0, 3) and out0["convergent_mask"].shape == (0,) and out0["convergent_mask"].dtype == torch.bool
    assert tr.ray_sampler(SDFCallable(two), e, e, e[:, 0], e[:, 0])[0].numel() == 0

    # nothing to do: the one evaluation on all rays, nothing convergent, the state the oracle leaves
    f = _Counting(two)
    none = torch.zeros(n, dtype=torch.bool)
    out = tr(SDFCallable(f), o, d, near, far, none.cuda())
    assert f.calls == [n] and not bool(out["convergent_mask"].any())
    _same_result(out, R.raytracer_forward(two, co, cd, cnear, cfar, none), "work_mask all false")

    # chunk: every chunk is a reference call of its own
    parts = [R.raytracer_forward(two, co[a:a + 1000], cd[a:a + 1000], cnear[a:a + 1000], cfar[a:a + 1000], chit[a:a + 1000])
             for a in range(0, n, 1000)]
    want = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    _same_result(tr(SDFCallable(two), o, d, near, far, hit, chunk=1000), want, "chunk=1000")

    # a bad result is refused on the host, before any kernel reads it
    for bad in (lambda x: two(x).cpu(), lambda x: two(x).double(), lambda x: two(x)[:-1], lambda x: two(x).unsqueeze(-1).expand(-1, 2)):
        with pytest.raises(_lib.IronError):
            tr(SDFCallable(bad), o, d, near, far, hit)
    torch.cuda.synchronize()
    # [m, 1] is m values: taken
    _same_result(tr(SDFCallable(lambda x: two(x).unsqueeze(-1)), o, d, near, far, hit), ref, "[m, 1] result")

    idx = torch.arange(n, device="cuda")
    with pytest.raises(_lib.IronError):
        tr.phase_begin(SDFCallable(two), o, d, near, far, hit, idx, 1, n)
    with pytest.raises(_lib.IronError):
        tr.forward_phased(SDFCallable(two), o, d, near, far, hit, idx, 1, n, lambda x: None)


class _Foreign(torch.nn.Module):
    """A network iron_amd knows nothing about: [m,3] -> [m,2], distance in column 0."""

    def forward(self, x):
        return torch.stack([two(x), x[:, 0]], dim=-1)


def test_foreign_network_through_raytrace_pixels():
    _field_is_bit_equal(two)
    K, W2C = scenes.fixture_camera_matrices(48, 48)
    cam = Camera(48, 48, K.cuda(), W2C.cuda())
    net = _Foreign().cuda()
    tr = RayTracer()
    res = raytrace_pixels(net, tr, cam.get_uv(), cam)
    ref, _, _, _ = _oracle("two")
    assert set(res.keys()) == {"convergent_mask", "points", "sdf", "distance", "depth", "uv", "ray_o", "ray_d", "ray_d_norm"}
    shapes = {"convergent_mask": (48, 48), "points": (48, 48, 3), "sdf": (48, 48), "distance": (48, 48), "depth": (48, 48),
              "uv": (48, 48, 2), "ray_o": (48, 48, 3), "ray_d": (48, 48, 3), "ray_d_norm": (48, 48)}
    for k, sh in shapes.items():
        assert tuple(res[k].shape) == sh, (k, res[k].shape)
        assert res[k].dtype == (torch.bool if k == "convergent_mask" else torch.float32), k
    _same_result({k: res[k].reshape(-1, 3) if k == "points" else res[k].reshape(-1) for k in ("convergent_mask", "points", "sdf", "distance")},
                 ref, "raytrace_pixels")
    assert torch.equal(res["depth"], res["distance"] / res["ray_d_norm"])
    # the fused path returns the same keys, shapes and dtypes
    fused = raytrace_pixels(scenes.build_networks("S1")["sdf_network"].cuda(), RayTracer(), cam.get_uv(), cam)
    assert {k: (tuple(v.shape), v.dtype) for k, v in fused.items()} == {k: (tuple(v.shape), v.dtype) for k, v in res.items()}
    cam_res = raytrace_camera(cam, net, tr, detect_edges=False)
    assert torch.equal(cam_res["convergent_mask"], res["convergent_mask"])
    assert bool((cam_res["depth"][~cam_res["convergent_mask"]] == 0).all())
    # not part of the callable tracer: the edge walk and the shading of a foreign network fail loudly
    with pytest.raises(_lib.IronError):
        raytrace_camera(cam, net, tr, detect_edges=True)
    from iron_amd.raytracer import render_normal_and_color
    with pytest.raises(_lib.IronError):
        render_normal_and_color(cam_res, net, {}, lambda *a: None)


def test_bare_lambdas_are_still_refused():
    (o, d, near, far, hit), _ = _rays()
    sdf = scenes.build_networks("S1")["sdf_network"].cuda()
    with pytest.raises(_lib.IronError, match="SDFCallable"):
        RayTracer()(lambda x: x.norm(dim=-1) - 0.5, o, d, near, far, hit)
    with pytest.raises(_lib.IronError):
        RayTracer()(lambda x: sdf(x)[..., 0] - 0.01, o, d, near, far, hit)
    # while the handle and the network-wrapping lambda run the fused tracer as before
    a = RayTracer()(SDFHandle(sdf), o, d, near, far, hit)
    b = RayTracer()(lambda x: sdf(x)[..., 0], o, d, near, far, hit)
    assert torch.equal(a["distance"], b["distance"])
