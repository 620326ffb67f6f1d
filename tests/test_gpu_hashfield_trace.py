"""GPU: the device-resident tracer of the hash-grid field (TCNNSDF.as_traced -> HashFieldSDF; iron_amd/csrc/hashgrid_trace.hip,
DESIGN.md §30) against the callable arm, RayTracer on field.as_callable(scale, offset): the same reference call with the values
supplied batch by batch from the host (csrc/trace_any.hip).  The fused evaluation is row-independent, so every output must agree
BIT FOR BIT, NaN payloads included: floats are compared through .view(torch.int32).

Fields (built once per module):
  (a) the 2 x 32 ReLU field of test_gpu_hashgrid_fit fitted to a sphere for 30 steps;
  (b) that field with randn * SIGMA_B (seeded) added to its table: a bumpy sphere with overshoots, several roots and rootless rays;
  (c) the zero-mean random table of _hashgrid_oracle's check configuration under a 64 x 2 head with no activation: sign noise,
      nearly every ray goes to the sampler and bisects.
SIGMA_B and the seeds were chosen by running the CALLABLE arm alone; test_the_callable_arm_covers_every_branch asserts on that arm
that sphere-converged, sampled, rootless, bisected rays, T >= 3 and the reversed interval (s < 0 after sphere tracing) all occur."""
import functools
import tempfile

import pytest
import torch

import _hashfield_oracle as H
from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, HashFieldSDF, RayTracer, SDFCallable, intersect_sphere, raytrace_pixels
from test_gpu_hashfield import make_field
from test_gpu_hashgrid_fit import fit, make_field as make_fit_field

pytestmark = pytest.mark.gpu
SIDE = 48
SIGMA_B, SEED_B = 0.05, 11
NAN_ENTRY = 40              # the table row of field (b) set to NaN in test_a_nan_table_entry...
KEYS = ("convergent_mask", "points", "sdf", "distance")
MAP = (0.5, 0.5)            # the tracer works in the unit sphere, the field lives in the unit cube


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want, what=""):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert torch.equal(bits(got[k]), bits(want[k])), "%s: %s differs in %d entries" % (
            what, k, int((bits(got[k]) != bits(want[k])).sum()))


@functools.lru_cache(maxsize=None)
def rays():
    K, W2C = scenes.fixture_camera_matrices(SIDE, SIDE)
    cam = Camera(SIDE, SIDE, K.cuda(), W2C.cuda())
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(o, d, 1.0)
    return cam, o, d, near.contiguous(), far.contiguous(), hit.contiguous()


def fresh_fit_field():
    with tempfile.TemporaryDirectory() as tmp:
        return make_fit_field(tmp + "/fit.json")


def clone(f):
    """another field with the parameters of field (a) or (b)"""
    g = fresh_fit_field()
    g.load_state_dict(f.state_dict())
    return g.cuda()


@functools.lru_cache(maxsize=None)
def field(which):
    if which == "a":
        f = fresh_fit_field().cuda()

        def sdf_and_gradient(p):
            sdf, _, g = f.get_all(p, is_training=True)
            return sdf, g

        fit(list(f.parameters()), sdf_and_gradient, torch.device("cuda"), steps=30)
        return f
    if which == "b":
        f = clone(field("a"))
        noise = torch.randn(f.sdf_encoding.params.shape, generator=torch.Generator().manual_seed(SEED_B)) * SIGMA_B
        with torch.no_grad():
            f.sdf_encoding.params.add_(noise.cuda())
        return f
    return head_field((64, 2), "None")


@functools.lru_cache(maxsize=None)
def head_field(head, act):
    """field (c)'s table under another head"""
    c, _ = H.case_encoding("check_uniform")
    return make_field(c["cfg"], head, act, 1, c["table"], H.case_weights("check_uniform", head, 1))


def arms(f, m=MAP):
    return f.as_callable(*m), f.as_traced(*m)


def sliced(n, work="hit"):
    """n rays from the middle of the image on (where the sphere is), or all of them"""
    _, o, d, near, far, hit = rays()
    a = 0 if n >= o.shape[0] - 27 else (SIDE // 2) * SIDE + 5
    s = slice(a, a + n)
    w = hit[s].clone()
    if work == "thirds":
        w[::3] = False
    elif work == "none":
        w[:] = False
    return o[s], d[s], near[s], far[s], w


def both(f, n=SIDE * SIDE, work="hit", chunk=0, stats=False, **tracer):
    call, traced = arms(f)
    args = sliced(n, work)
    tc, tn = RayTracer(**tracer), RayTracer(**tracer)
    want = tc(call, *args, chunk=chunk, collect_stats=stats)
    got = tn(traced, *args, chunk=chunk, collect_stats=stats)
    return got, want, tn.last_stats, tc.last_stats


def test_the_callable_arm_covers_every_branch():
    """the minima the comparisons below rest on, asserted on the yardstick arm before anything is compared"""
    _, o, d, near, far, hit = rays()
    seen = dict(sphere_conv=0, sampled=0, rootless=0, bisected=0, T=0, reversed=0)
    for which in "abc":
        call = field(which).as_callable(*MAP)
        tr = RayTracer()
        out = tr(call, o, d, near, far, hit, collect_stats=True)
        st = tr.last_stats
        conv, unf, _, s, _ = tr.sphere_tracing(call, o, d, near, far, hit)
        row = dict(sphere_conv=int(conv.sum()), sampled=st["n_sampler"], rootless=int((unf & ~out["convergent_mask"]).sum()),
                   bisected=st["n_bisect"], T=st["n_bisect_iters"], reversed=int((unf & (s < 0)).sum()))
        print("   field (%s), callable arm: %s" % (which, row))
        assert row["sampled"] == int(unf.sum())
        for k, v in row.items():
            seen[k] = max(seen[k], v)
    assert seen["sphere_conv"] > 0 and seen["sampled"] > 0 and seen["rootless"] > 0 and seen["bisected"] > 0
    assert seen["T"] >= 3 and seen["reversed"] > 0


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_defaults_match_the_callable_arm_bit_for_bit(which):
    got, want, sn, sc = both(field(which), stats=True)
    same(got, want, which)
    for k in ("n_sampler", "n_bisect", "n_bisect_iters"):
        assert sn[k] == sc[k], (k, sn[k], sc[k])
    assert sn["incomplete"] == 0 and sn["n_evals_issued"] >= sn["n_evals"] > 0
    assert sn["n_evals"] <= sc["n_evals"]          # the samples behind a ray's first negative one are not evaluated
    print("   field (%s): issued / live lane evaluations %.2f; live %d against the callable's %d" %
          (which, sn["n_evals_issued"] / sn["n_evals"], sn["n_evals"], sc["n_evals"]))
    # a second run, and the mask alone
    call, traced = arms(field(which))
    _, o, d, near, far, hit = rays()
    tr = RayTracer()
    same(tr(traced, o, d, near, far, hit), got, "second run")
    occ = tr.occluded(traced, o, d, near, far, hit, collect_stats=True)
    assert occ.dtype == torch.bool and torch.equal(occ, got["convergent_mask"])
    assert tr.last_stats["n_sampler"] == sn["n_sampler"] and tr.last_stats["n_bisect"] == sn["n_bisect"]
    assert torch.equal(tr.occluded(traced, o, d, near, far), tr(call, o, d, near, far, torch.ones_like(hit))["convergent_mask"])


# chunk, n_steps, sphere_tracing_iters, n, work_mask: every value of the issue's lists at least once, on field (b)
RUNS = [
    (1, 128, 16, 65, "hit"),
    (100, 128, 16, SIDE * SIDE, "hit"),
    (5000, 128, 16, SIDE * SIDE, "thirds"),
    (0, 2, 16, 1, "hit"),
    (0, 65, 16, 63, "hit"),
    (0, 100, 16, 64, "thirds"),
    (100, 65, 1, SIDE * SIDE - 27, "hit"),
    (0, 128, 0, SIDE * SIDE, "hit"),
    (0, 128, 1, 65, "hit"),
    (0, 128, 16, SIDE * SIDE, "none"),
]


@pytest.mark.parametrize("chunk,n_steps,iters,n,work", RUNS)
def test_parameters_sizes_and_masks_on_the_bumpy_field(chunk, n_steps, iters, n, work):
    got, want, sn, sc = both(field("b"), n=n, work=work, chunk=chunk, stats=True, n_steps=n_steps, sphere_tracing_iters=iters)
    same(got, want, "chunk %d n_steps %d iters %d n %d %s" % (chunk, n_steps, iters, n, work))
    for k in ("n_sampler", "n_bisect", "n_bisect_iters"):
        assert sn[k] == sc[k], (k, sn[k], sc[k])
    if work == "none":
        assert not bool(got["convergent_mask"].any()) and sn["n_sampler"] == 0


def test_sign_noise_field_with_chunks():
    for chunk in (1, 100):
        n = 65 if chunk == 1 else SIDE * SIDE
        got, want, sn, sc = both(field("c"), n=n, chunk=chunk, stats=True)
        same(got, want, "chunk %d" % chunk)
        assert sn["n_bisect_iters"] == sc["n_bisect_iters"] and sn["n_bisect"] == sc["n_bisect"] > 0


@pytest.mark.parametrize("head,act", [((16, 1), "None"), ((128, 3), "Softplus"), ((64, 4), "ReLU")])
def test_other_head_shapes(head, act):
    got, want, sn, sc = both(head_field(head, act), stats=True)
    same(got, want, "%s %s" % (head, act))
    assert sn["n_sampler"] == sc["n_sampler"] and sn["n_bisect"] == sc["n_bisect"] and sn["n_bisect_iters"] == sc["n_bisect_iters"]
    # the bisection kernels of this head whatever the sampler found: the brackets [near, middle of the chord] of the rays that hit
    call, traced = arms(head_field(head, act))
    _, o, d, near, far, hit = rays()
    at = torch.nonzero(hit)[:, 0]
    oh, dh, nh = o[at].contiguous(), d[at].contiguous(), near[at].contiguous()
    mid = (nh + far[at]) / 2
    f_low, f_high = call(oh + dh * nh[:, None]), call(oh + dh * mid[:, None])
    tr = RayTracer()
    for x, y in zip(tr.rootfind(traced, f_low, f_high, nh, mid, oh, dh), tr.rootfind(call, f_low, f_high, nh, mid, oh, dh)):
        assert torch.equal(bits(x), bits(y))


def test_no_rays():
    call, traced = arms(field("b"))
    _, o, d, near, far, hit = rays()
    tr = RayTracer()
    out = tr(traced, o[:0], d[:0], near[:0], far[:0], hit[:0], collect_stats=True)
    assert out["points"].shape == (0, 3) and out["convergent_mask"].shape == (0,) and out["sdf"].shape == (0,) and out["distance"].shape == (0,)
    assert tr.occluded(traced, o[:0], d[:0], near[:0], far[:0]).shape == (0,)
    assert tr.ray_sampler(traced, o[:0], d[:0], near[:0], far[:0])[0].numel() == 0


def test_a_permutation_of_the_rays_permutes_the_outputs():
    _, traced = arms(field("b"))
    _, o, d, near, far, hit = rays()
    tr = RayTracer()
    out = tr(traced, o, d, near, far, hit)
    perm = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(3)).cuda()
    outp = tr(traced, o[perm].contiguous(), d[perm].contiguous(), near[perm], far[perm], hit[perm])
    same(outp, {k: out[k][perm] for k in KEYS}, "permutation")


def test_the_three_stages_match_the_callables():
    call, traced = arms(field("b"))
    _, o, d, near, far, hit = rays()
    tr = RayTracer()
    a, b = tr.sphere_tracing(traced, o, d, near, far, hit), tr.sphere_tracing(call, o, d, near, far, hit)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x), bits(y)), "sphere_tracing output %d" % i
    assert bool(a[1].any())
    at = torch.nonzero(hit)[:, 0]
    oh, dh, nh, fh = o[at].contiguous(), d[at].contiguous(), near[at].contiguous(), far[at].contiguous()
    for n_steps in (128, 100):
        tr = RayTracer(n_steps=n_steps)
        a, b = tr.ray_sampler(traced, oh, dh, nh, fh), tr.ray_sampler(call, oh, dh, nh, fh)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(bits(x), bits(y)), "ray_sampler output %d" % i
        assert 0 < int(a[0].sum()) < a[0].numel()
    # brackets [near, middle of the chord]: open where the chord's middle is inside the surface; every fifth one starts inside
    # (f_low <= 0: it opens no loop of its own and still moves with the call)
    tr = RayTracer()
    mid = (nh + fh) / 2
    d_low = nh.clone()
    d_low[::5] = mid[::5]
    f_low, f_high = call(oh + dh * d_low[:, None]), call(oh + dh * mid[:, None])
    is_open = (f_low > 0) & (f_high < 0)
    assert bool(is_open.any()) and bool((f_low <= 0).any()) and bool((~is_open & (f_low > 0)).any())
    a = tr.rootfind(traced, f_low, f_high, d_low, mid, oh, dh)
    b = tr.rootfind(call, f_low, f_high, d_low, mid, oh, dh)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x), bits(y)), "rootfind output %d" % i
    assert tr.last_stats["n_bisect"] == oh.shape[0] and tr.last_stats["n_bisect_iters"] >= 3


def test_a_power_of_two_scale_equals_scaling_the_rays_first():
    """x = fma(p, 0.5, 0) = p / 2 exactly, and rays scaled by 0.5 give exactly the halved points (a power of two commutes with every
    rounding of o + d t), so as_traced(0.5) on rays (o, d) and as_traced() on rays (o / 2, d / 2) with the same distances evaluate
    the field at the same bits.  The rays' origin is shifted by (1, 1, 1) first, so that the sphere sits in the cube's middle.  (With
    an offset the two sides add in a different order, (o + d t) / 2 + 1/2 against (o / 2 + 1/2) + (d / 2) t, and differ by
    roundings; the offset is covered by every other test here, against as_callable(0.5, 0.5).)"""
    f = field("b")
    _, o, d, near, far, hit = rays()
    o2 = o + 1.0
    tr = RayTracer()
    a = tr(f.as_traced(0.5, 0.0), o2, d, near, far, hit)
    b = tr(f.as_traced(), (o2 * 0.5).contiguous(), (d * 0.5).contiguous(), near, far, hit)
    same(a, tr(f.as_callable(0.5, 0.0), o2, d, near, far, hit), "scale 0.5 against its callable")
    for k in ("convergent_mask", "sdf", "distance"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(bits(a["points"] * 0.5), bits(b["points"]))
    assert 0 < int(a["convergent_mask"].sum()) < hit.numel()


def test_an_optimiser_step_is_seen_by_the_handle():
    f = clone(field("a"))
    call, traced = arms(f)
    _, o, d, near, far, hit = rays()
    tr = RayTracer()
    first = tr(traced, o, d, near, far, hit)
    opt = torch.optim.Adam(f.parameters(), lr=3e-2)
    x = torch.rand(512, 3, generator=torch.Generator().manual_seed(1)).cuda()
    (f.sdf(x) - 0.1).square().sum().backward()
    opt.step()
    second = tr(traced, o, d, near, far, hit)
    assert not torch.equal(bits(first["sdf"]), bits(second["sdf"]))
    same(second, tr(call, o, d, near, far, hit), "after the step")


def test_a_nan_table_entry_falls_where_the_callable_puts_it():
    """Row NAN_ENTRY of field (b)'s table (level 0, read by many rays; the callable arm ends without its 256-iteration error).  The
    ReLU head turns the NaN features into zeros, so what changes are values and counts; NaN values themselves reach the outputs in
    the all-NaN test below, under a head without activation."""
    f = clone(field("b"))
    clean = RayTracer()(f.as_traced(*MAP), *sliced(SIDE * SIDE))
    with torch.no_grad():
        f.sdf_encoding.params.view(-1, 2)[NAN_ENTRY] = float("nan")
    got, want, sn, sc = both(f, stats=True)
    same(got, want, "NaN entry")
    assert any(not torch.equal(bits(got[k]), bits(clean[k])) for k in KEYS)       # the entry is one the rays read
    assert sn["n_bisect_iters"] == sc["n_bisect_iters"]


def test_an_all_nan_table_stops_after_256_iterations_on_both_sides():
    c, _ = H.case_encoding("check_mixed")
    f = make_field(c["cfg"], (16, 1), "None", 1)         # no activation: a ReLU would turn the NaN features into zeros
    with torch.no_grad():
        f.sdf_encoding.params.fill_(float("nan"))
    _, o, d, near, far, hit = rays()
    at = torch.nonzero(hit)[:100, 0]
    oh, dh, nh, fh = o[at].contiguous(), d[at].contiguous(), near[at].contiguous(), far[at].contiguous()
    f_low, f_high = torch.ones_like(nh), -torch.ones_like(nh)
    calls = []

    def counted(x):
        calls.append(x.shape[0])
        return f.eval_fused(x, scale=0.5, offset=0.5)[..., 0]

    tr = RayTracer()
    with pytest.raises(_lib.IronError, match="does not close"):
        tr.rootfind(SDFCallable(counted), f_low, f_high, nh, fh, oh, dh)
    assert len(calls) == 256
    with pytest.raises(_lib.IronError, match="does not close"):
        tr.rootfind(f.as_traced(*MAP), f_low, f_high, nh, fh, oh, dh)
    assert tr.last_stats["incomplete"] == 1 and tr.last_stats["n_bisect_iters"] == 256
    # forward(): NaN values end sphere tracing unconverged on both sides, with the same payloads
    work = torch.ones_like(nh, dtype=torch.bool)
    got, want = RayTracer()(f.as_traced(*MAP), oh, dh, nh, fh, work), RayTracer()(f.as_callable(*MAP), oh, dh, nh, fh, work)
    same(got, want, "all NaN")
    assert bool(torch.isnan(got["sdf"]).all())
    tr = RayTracer(sphere_tracing_iters=0)
    assert not bool(tr(f.as_traced(*MAP), oh, dh, nh, fh, torch.ones_like(nh, dtype=torch.bool))["convergent_mask"].any())


def test_refusals():
    f = field("b")
    traced = f.as_traced(*MAP)
    assert isinstance(traced, HashFieldSDF) and traced.field is f
    _, o, d, near, far, hit = rays()
    tr = RayTracer()
    with pytest.raises(_lib.IronError, match="CUDA"):
        tr(traced, o.cpu(), d.cpu(), near.cpu(), far.cpu(), hit.cpu())
    with pytest.raises(_lib.IronError, match="CUDA"):
        tr(traced, o, d, near.cpu(), far, hit)
    with pytest.raises(_lib.IronError, match="float32"):
        tr(traced, o, d.double(), near, far, hit)
    with pytest.raises(_lib.IronError, match="work_mask"):
        tr(traced, o, d, near, far, hit[:-1])
    with pytest.raises(_lib.IronError, match="work_mask"):
        tr(traced, o, d, near, far, hit.float())
    with pytest.raises(_lib.IronError, match="one entry per ray"):
        tr(traced, o, d, near[:-1], far, hit)
    with pytest.raises(_lib.IronError, match="n_steps"):
        RayTracer(n_steps=1)(traced, o, d, near, far, hit)
    with pytest.raises(_lib.IronError, match="n_steps"):
        RayTracer(n_steps=5000).occluded(traced, o, d, near, far, hit)
    c, _ = H.case_encoding("check_mixed")
    odd = make_field(c["cfg"], (48, 2), "ReLU", 1)
    with pytest.raises(_lib.IronError, match="n_neurons"):
        odd.as_traced()
    with pytest.raises(_lib.IronError, match="TCNNSDF"):
        HashFieldSDF(torch.nn.Linear(3, 1))
    idx = torch.arange(o.shape[0], device="cuda")
    with pytest.raises(_lib.IronError, match="HashFieldSDF"):
        tr.phase_begin(traced, o, d, near, far, hit, idx, 1, o.shape[0])
    with pytest.raises(_lib.IronError, match="HashFieldSDF"):
        tr.forward_phased(traced, o, d, near, far, hit, idx, 1, o.shape[0], lambda x: None)
    with pytest.raises(_lib.IronError, match="the table"):
        tr(clone(f).cpu().as_traced(*MAP), o, d, near, far, hit)


def test_raytrace_pixels_takes_the_handle():
    f = field("b")
    cam, o, d, near, far, hit = rays()
    tr = RayTracer()
    uv = cam.get_uv()
    res = raytrace_pixels(f.as_traced(*MAP), tr, uv, cam)
    assert set(res) == {"convergent_mask", "points", "sdf", "distance", "depth", "uv", "ray_o", "ray_d", "ray_d_norm"}
    sh = tuple(uv.shape[:-1])
    assert res["convergent_mask"].shape == sh and res["sdf"].shape == sh and res["distance"].shape == sh and res["depth"].shape == sh
    assert res["points"].shape == sh + (3,)
    direct = tr(f.as_traced(*MAP), o, d, near, far, hit, chunk=200000)
    for k in KEYS:
        assert torch.equal(bits(res[k].reshape(direct[k].shape)), bits(direct[k])), k
    foreign = raytrace_pixels(lambda x: f.eval_fused(x, scale=0.5, offset=0.5), tr, uv, cam)      # the routing of anything else stays
    for k in KEYS:
        assert torch.equal(bits(res[k]), bits(foreign[k])), k


def test_neural_relight_takes_the_handle():
    """occluded / forward(chunk=1) on a HashFieldSDF inside relight_results: the same colours as on the callable"""
    import _envlight_oracle as EO
    from iron_amd.envmap import EnvMap
    from iron_amd.neural_relight import relight_results
    f = field("a")
    call, traced = arms(f)
    o, d, near, far, hit = sliced(256)
    tr = RayTracer()
    g = tr(call, o, d, near, far, hit)
    n = o.shape[0]
    normal = torch.nn.functional.normalize(g["points"] + 1e-6, dim=-1)
    gb = {"convergent_mask": g["convergent_mask"], "points": g["points"], "normal": normal, "ray_d": d,
          "diffuse_albedo": torch.full((n, 3), 0.5, device="cuda"), "specular_albedo": torch.full((n, 3), 0.2, device="cuda"),
          "specular_roughness": torch.full((n,), 0.3, device="cuda")}
    env = EnvMap(EO.hot_map().cuda().float())

    def surface(points, ray_d):
        m = points.shape[0]
        return {"normal": torch.nn.functional.normalize(points + 1e-6, dim=-1), "diffuse_albedo": torch.full((m, 3), 0.5, device="cuda"),
                "specular_albedo": torch.full((m, 3), 0.2, device="cuda"), "specular_roughness": torch.full((m,), 0.3, device="cuda")}

    kw = dict(n_light=4, n_brdf=4, seed=5, max_depth=2, n_paths=2, surface_fn=surface)
    a = relight_results(gb, traced, RayTracer(), env, **kw)
    b = relight_results(gb, call, RayTracer(), env, **kw)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert float(a["color"].sum()) > 0
    with pytest.raises(_lib.IronError, match="surface_fn"):
        relight_results(gb, traced, RayTracer(), env, n_light=4, n_brdf=4, max_depth=2, n_paths=4)
