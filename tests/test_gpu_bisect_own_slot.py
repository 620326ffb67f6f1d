"""The bisection kernels (csrc/trace.hip: k_bisect_a evaluates the mid-point a ray's own iterations end on in the ray's slot,
k_bisect_b touches only the rays whose chunk ran longer) against a torch emulation on the device that evaluates with
sdf_network.sdf() -- bitwise the tracer's value -- and forms o + d * mid with a separate mul and add.  Scene S1, rays of a
56x56 view."""
import pytest
import torch

from iron_amd import scenes
from oracle import iron_ref as R

from _bisect_emul import chunk_totals, finish_phase, own_phase
from _util import oracle_scene

pytestmark = pytest.mark.gpu

N_BRACKETS = 1007   # no multiple of 32


@pytest.fixture(scope="module")
def ctx():
    from iron_amd.raytracer import Camera, RayTracer, SDFHandle, intersect_sphere
    dev = torch.device("cuda", 0)
    nets_cpu = scenes.build_networks("S1")
    sc = oracle_scene(nets_cpu)
    net = nets_cpu["sdf_network"].to(dev)
    K, W2C = scenes.fixture_camera_matrices(56, 56)
    cam = Camera(56, 56, K.to(dev), W2C.to(dev))
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    ref = R.raytrace_camera(sc, R.CameraSpec(56, 56, K, W2C))   # the oracle's roots: once, shared, left unchanged

    @torch.no_grad()
    def sdf_dev(x):
        return net.sdf(x.contiguous())[:, 0]

    sdf_cpu = lambda x: R.sdf_forward(sc.sdf_sd, sc.sdf_spec, x)[:, 0]
    return dict(dev=dev, net=net, cam=cam, ro=ro, rd=rd, hit=hit, near=near, far=far, tr=RayTracer(), h=SDFHandle(net),
                ref_conv=ref["convergent_mask"].reshape(-1), ref_dist=ref["distance"].reshape(-1), sdf_dev=sdf_dev, sdf_cpu=sdf_cpu,
                thr=R.TracerParams().sdf_threshold)


@pytest.fixture(scope="module")
def brackets(ctx):
    """1 007 hand-made brackets around the oracle's roots, widths cycling through 0.2 * 2^-j (j = 0 .. 12): own counts 0 .. ~11."""
    dev = ctx["dev"]
    idx = torch.nonzero(ctx["ref_conv"]).reshape(-1)
    assert idx.numel() > 200
    idx = idx[torch.arange(N_BRACKETS) % idx.numel()]
    root = ctx["ref_dist"][idx].to(dev)
    o, d = ctx["ro"][idx.to(dev)].contiguous(), ctx["rd"][idx.to(dev)].contiguous()
    w = 0.2 * torch.pow(2.0, -(torch.arange(N_BRACKETS) % 13).float()).to(dev)
    frac = (0.3 + 0.4 * ((torch.arange(N_BRACKETS) * 7 % 11).float() / 10.0)).to(dev)
    d_lo = root - frac * w
    d_hi = d_lo + w
    f_lo = ctx["sdf_dev"](o + d * d_lo.unsqueeze(-1)).clone()
    f_hi = ctx["sdf_dev"](o + d * d_hi.unsqueeze(-1)).clone()
    f_lo[torch.tensor([0, 31, 32, 500, N_BRACKETS - 1], device=dev)] = -1.0   # five that are no brackets
    st = own_phase(ctx["sdf_dev"], f_lo, f_hi, d_lo, d_hi, o, d, ctx["thr"])
    total = st["k"].max().expand_as(st["k"])   # one call = one chunk
    want = finish_phase(ctx["sdf_dev"], st, o, d, total)
    return dict(o=o, d=d, f_lo=f_lo, f_hi=f_hi, d_lo=d_lo, d_hi=d_hi, own=st["k"], want=want)


def _rootfind(ctx, b, sel=None):
    g = (lambda t: t if sel is None else t[sel].contiguous())
    return ctx["tr"].rootfind(ctx["h"], g(b["f_lo"]), g(b["f_hi"]), g(b["d_lo"]), g(b["d_hi"]), g(b["o"]), g(b["d"]))


def test_mixed_counts_in_one_call(ctx, brackets):
    b = brackets
    assert int(b["own"].min()) == 0 and int(b["own"].max()) >= 10 and len(set(b["own"].tolist())) >= 10
    got_p, got_d, got_f = _rootfind(ctx, b)
    want_p, want_d, want_f = b["want"]
    print("max |d - emu| %.3e  |f - emu| %.3e" % (float((got_d - want_d).abs().max()), float((got_f - want_f).abs().max())))
    assert torch.equal(got_d, want_d)
    assert torch.equal(got_f, want_f)
    assert torch.equal(got_p, want_p)
    # and the oracle's rootfind on the CPU, within the tracer's tolerance
    c = lambda t: t.cpu().clone()
    ref_p, ref_d, ref_f, _ = R.rootfind(ctx["sdf_cpu"], c(b["f_lo"]), c(b["f_hi"]), c(b["d_lo"]), c(b["d_hi"]), c(b["o"]), c(b["d"]),
                                        R.TracerParams())
    print("max |d - oracle| %.3e  |f - oracle| %.3e" % (float((got_d.cpu() - ref_d).abs().max()), float((got_f.cpu() - ref_f).abs().max())))
    assert float((got_d.cpu() - ref_d).abs().max()) <= 2e-4 and float((got_f.cpu() - ref_f).abs().max()) <= 2e-4


def test_order_independence(ctx, brackets):
    b = brackets
    base = _rootfind(ctx, b)
    perm = torch.randperm(N_BRACKETS, generator=torch.Generator().manual_seed(3)).to(ctx["dev"])
    got = _rootfind(ctx, b, perm)
    for x, y in zip(got, base):
        assert torch.equal(x, y[perm])
    dup = torch.cat([torch.arange(N_BRACKETS), torch.arange(100)]).to(ctx["dev"])
    got = _rootfind(ctx, b, dup)
    for x, y in zip(got, base):
        assert torch.equal(x, y[dup])


def _sampler_brackets(ctx):
    """The brackets the dense sampler hands to the bisection in forward(), restated in torch on the device (raytracer.py:59-65,
    142-197): -> (ray ids, f_lo, f_hi, d_lo, d_hi)."""
    from iron_amd.raytracer import _linspace_steps
    tr, dev = ctx["tr"], ctx["dev"]
    _, unf, _, s, t = tr.sphere_tracing(ctx["h"], ctx["ro"], ctx["rd"], ctx["near"], ctx["far"], ctx["hit"])
    ids = torch.nonzero(unf).reshape(-1)
    pos = s[ids] > 0.0
    smin = torch.where(pos, t[ids], ctx["near"][ids])
    smax = torch.where(pos, ctx["far"][ids], t[ids])
    lin = _linspace_steps(tr.n_steps, dev)
    z = smin.unsqueeze(-1) + lin.unsqueeze(0) * (smax - smin).unsqueeze(-1)
    pts = ctx["ro"][ids].unsqueeze(1) + ctx["rd"][ids].unsqueeze(1) * z.unsqueeze(-1)
    f = ctx["sdf_dev"](pts.reshape(-1, 3)).reshape(z.shape)
    neg = f < 0.0
    first = torch.argmax(neg.int(), dim=-1)
    root = neg.any(dim=-1) & (first >= 1)
    ids, z, f, first = ids[root], z[root], f[root], first[root]
    r = torch.arange(ids.numel(), device=dev)
    return ids, f[r, first - 1], f[r, first], z[r, first - 1], z[r, first]


@pytest.mark.parametrize("max_num_rays", [500, 3136])
def test_chunked_forward_and_two_phases(ctx, max_num_rays):
    from iron_amd.raytracer import raytrace_camera
    tr, dev, n = ctx["tr"], ctx["dev"], 56 * 56
    keys = ("convergent_mask", "points", "sdf", "distance")
    full = raytrace_camera(ctx["cam"], ctx["net"], tr, max_num_rays=max_num_rays)
    full = {k: full[k].reshape(n, -1).clone() for k in keys}
    fwd = tr(ctx["h"], ctx["ro"], ctx["rd"], ctx["near"], ctx["far"], ctx["hit"], chunk=max_num_rays, collect_stats=True)
    fwd = {k: fwd[k].reshape(n, -1).clone() for k in keys}
    fwd_stats = dict(tr.last_stats)
    for k in keys:
        assert torch.equal(full[k], fwd[k]), k

    n_chunks = (n + max_num_rays - 1) // max_num_rays
    ray_index = torch.arange(n, dtype=torch.int64, device=dev)
    ids, f_lo, f_hi, d_lo, d_hi = _sampler_brackets(ctx)
    assert ids.numel() > 50
    o, d = ctx["ro"][ids].contiguous(), ctx["rd"][ids].contiguous()
    st = own_phase(ctx["sdf_dev"], f_lo, f_hi, d_lo, d_hi, o, d, ctx["thr"])
    totals = chunk_totals(st, ray_index[ids] // max_num_rays, n_chunks)
    rest = torch.ones(n, dtype=torch.bool, device=dev)
    rest[ids] = False

    for extra in (0, 1, 5):
        state = tr.phase_begin(ctx["h"], ctx["ro"], ctx["rd"], ctx["near"], ctx["far"], ctx["hit"], ray_index, n_chunks, max_num_rays,
                               collect_stats=True)
        assert torch.equal(state["chunk_iters"].long(), totals)   # the table phase a leaves: the chunks' largest own counts
        state["chunk_iters"] += extra
        got = tr.phase_finish(state)
        got = {k: got[k].reshape(n, -1) for k in keys}
        if extra == 0:
            for k in keys:
                assert torch.equal(got[k], fwd[k]), k
            assert tr.last_stats == fwd_stats
        want_p, want_d, want_f = finish_phase(ctx["sdf_dev"], st, o, d, (totals + extra)[ray_index[ids] // max_num_rays])
        assert bool(got["convergent_mask"][ids].all())
        assert torch.equal(got["distance"][ids, 0], want_d), extra
        assert torch.equal(got["sdf"][ids, 0], want_f), extra
        assert torch.equal(got["points"][ids], want_p), extra
        for k in keys:   # every other ray is as forward() leaves it
            assert torch.equal(got[k][rest], fwd[k][rest]), (k, extra)


def test_nothing_to_bisect(ctx):
    """C0: the 64x64 crop (ul = 224, 224) of the 512^2 fixture camera -- every ray converges by sphere tracing."""
    from iron_amd.raytracer import Camera, intersect_sphere
    dev, tr = ctx["dev"], ctx["tr"]
    K, W2C = scenes.fixture_camera_matrices(512, 512)
    cam, _, _ = Camera(512, 512, K.to(dev), W2C.to(dev)).crop_region(64, 64, ul_corner=(224, 224))
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    a = {k: v.clone() for k, v in tr(ctx["h"], ro, rd, near, far, hit, collect_stats=True).items()}
    stats = dict(tr.last_stats)
    b = tr(ctx["h"], ro, rd, near, far, hit, collect_stats=True)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert stats["n_bisect"] == 0
    assert stats["n_evals"] == stats["n_evals_sphere"]
    assert tr.last_stats == stats
