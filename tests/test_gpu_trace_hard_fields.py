"""GPU: the tracer's stages (csrc/trace.hip through RayTracer.sphere_tracing / ray_sampler / rootfind) and the whole tracer against
the fp64 oracle on the fields of tests/_hard_fields.py -- bumpy spheres and generalised nets with hundreds of overshoot rays (sampler
range [min_dis, acc_dis], raytracer.py:59-65), rays with three and more sign changes (the first bracket must be taken), rays whose
first sample is negative (no root) and reversed sampler ranges.  S0 / S1 have next to none of these, and the generalised nets
were only ever compared with the project's own other modes: a mistake shared by all modes passed every test.

Every stage gets the oracle's inputs, identical on both sides.  The sampler is held to the oracle's outcome on every ray that is
`decided`: whose deciding values (tests/_hard_fields.py classify_sampler) are further than tau from zero, tau = max(1e-5, 4 x the
reference's own fp32-vs-fp64 difference on the field).  tests/test_hard_fields_oracle.py pins from the oracle alone that the subsets
are populated and that the rays left out are under 2 %.  The rootfind stage leaves no ray out (see test d).  The screen and the adaptive stride run at their defaults; test f repeats
the sampler stage and the whole tracer with each of them off and wants bit-equal outputs.

The lines printed per field are the table of DESIGN.md 3.2."""
import ctypes as C
import functools

import pytest
import torch

from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, SDFHandle, intersect_sphere, raytrace_camera

import _hard_fields as HF

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-4               # |d distance|, |d point|: the tracer bisects to 1e-4-wide brackets (tests/test_gpu_trace.py)
EXCLUDED_CAP = 0.02
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")


@functools.lru_cache(maxsize=None)
def _net(name):
    return HF.build(name).to(DEV)      # a second build: the oracle's copy stays on the CPU, parameters bit-identical


def _status(net) -> int:
    st = C.c_int32(0)
    _lib.check(_lib.load().iron_net_numeric_status(net.hip_net().handle, C.byref(st), _lib.stream_ptr(torch.device(DEV, 0))))
    return st.value


def _counts():
    """Screen and stride counts of the last traced call on the current stream (a process that has also traced on a side stream,
    render_camera's silhouette pass, holds several trace workspaces)."""
    d = torch.device(DEV, 0)
    ws = _lib.current_workspace(d, "trace")
    assert ws is not None
    lib, dev = _lib.load(), _lib.stream_ptr(d)
    a, b = (C.c_double * 5)(), (C.c_double * 4)()
    _lib.check(lib.iron_trace_screen_counts(ws.data_ptr(), a, dev))
    _lib.check(lib.iron_trace_stride_counts(ws.data_ptr(), b, dev))
    return {"screened": a[0], "resolved": a[1], "overflow": a[2], "ratio": a[3], "pending": a[4],
            "passes": b[0], "strided": b[1], "slope": b[2], "adaptive": b[3]}


def _gpu_sampler(name, net=None):
    sg = HF.stage(name)
    m = sg.m
    out = RayTracer().ray_sampler(SDFHandle(net or _net(name)), sg.ro[m].to(DEV), sg.rd[m].to(DEV), sg.s_min.to(DEV), sg.s_max.to(DEV))
    torch.cuda.synchronize()
    return [x.clone() for x in out]


def _gpu_trace(name, net=None):
    import iron_amd.raytracer as RT
    K, W2C = scenes.fixture_camera_matrices(HF.RES, HF.RES, HF.yaw_of(name))
    cam = Camera(HF.RES, HF.RES, K.to(DEV), W2C.to(DEV))
    old = RT.VERBOSE_MODE
    try:
        RT.VERBOSE_MODE = True
        tr = RayTracer()
        res = raytrace_camera(cam, net or _net(name), tr, max_num_rays=HF.CHUNK)
        torch.cuda.synchronize()
    finally:
        RT.VERBOSE_MODE = old
    return {k: res[k].clone() for k in KEYS}, dict(tr.last_stats), cam


# ---- a. values -----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_a_values_on_the_samplers_points(name):
    """net.sdf against the fp64 oracle on the sampler's own sample points: within tau / 2, so that `decided` means what it says."""
    sg = HF.stage(name)
    got = torch.cat([_net(name).sdf(c.to(DEV))[..., 0].cpu() for c in torch.split(sg.pts, 65536)]).double()
    err = float((got - sg.pts_f64).abs().max())
    print("\n[a] %-18s points %d max|f_gpu - f64| %.2e (oracle fp32: %.2e) tau %.2e" % (name, got.numel(), err, sg.oracle_noise, sg.tau))
    assert err <= sg.tau / 2, (name, err, sg.tau)


# ---- b. sampler stage ------------------------------------------------------------------------------------------------------------
def _check_sampler(name, out):
    sg = HF.stage(name)
    sa, dec = sg.sa, sg.decided
    root, sp, ss, st = (x.cpu() for x in out)
    k = int(sg.m.sum())
    assert root.shape == (k,) and sp.shape == (k, 3)
    flips = root != sa.root
    excluded = float((~dec).float().mean())
    lo, hi = torch.minimum(sa.z_lo, sa.z_hi), torch.maximum(sa.z_lo, sa.z_hi)
    t = st.double()
    inside = (t >= lo - 1e-6) & (t <= hi + 1e-6)
    dt, dp = (t - sa.t).abs(), (sp.double() - sa.p).abs().amax(dim=1)
    rooted = dec & sa.root & root
    print("\n[b] %-18s sampler rays %d roots gpu/oracle %d/%d flips %d (decided: %d) excluded %.2f %% | outside bracket %d max|dt| %.2e "
          "max|dp| %.2e | reversed+rooted %d" % (name, k, int(root.sum()), int(sa.root.sum()), int(flips.sum()), int((flips & dec).sum()),
                                                100 * excluded, int((~inside & rooted).sum()), float(dt[rooted].max()), float(dp[rooted].max()),
                                                int((sg.sets.reversed_rooted & rooted).sum())))
    assert excluded <= EXCLUDED_CAP
    assert int((flips & dec).sum()) == 0, (name, (flips & dec).nonzero().reshape(-1).tolist())
    # the first bracket, in either orientation: a root of a later sign change, or of the wrong end of a reversed range, is outside it
    assert bool(inside[rooted].all()), (name, (~inside & rooted).nonzero().reshape(-1).tolist())
    assert float(dt[rooted].max()) <= TOL and float(dp[rooted].max()) <= TOL
    none = ~root
    assert float(st[none].abs().max()) == 0.0 and float(sp[none].abs().max()) == 0.0 and float(ss[none].abs().max()) == 0.0
    passed = dec & ~flips & (none | (inside & (dt <= TOL) & (dp <= TOL)))
    subsets = ["overshoot", "multi"] + (["first_neg"] if name in HF.GEN else [])
    for s in subsets:
        assert int((getattr(sg.sets, s) & passed).sum()) >= 50, (name, s)
    # reversed ranges (s_max < s_min): rooted ones on the fields that must offer some (HF.REVERSED_ROOTED_FLOOR, pinned on the CPU),
    # their root on the far side of z_lo; the rootless ones came back as zeros above
    rev = sg.sets.reversed_rooted
    assert int((rev & passed).sum()) >= HF.REVERSED_ROOTED_FLOOR.get(name, 0), (name, int(rev.sum()), int((rev & passed).sum()))
    assert bool((st.double() <= sa.z_lo + 1e-6)[rev & rooted].all())
    return {s: int((getattr(sg.sets, s) & passed).sum()) for s in subsets + ["reversed", "reversed_rooted"]}


@torch.no_grad()
@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_b_sampler_stage_on_the_oracles_inputs(name):
    """Root mask equal on every decided ray (no allowance), every root inside the oracle's first bracket, rootless rays exact zeros;
    the overshoot, first-sample-negative and >= 3-sign-change subsets each with >= 50 decided rays that passed."""
    got = _check_sampler(name, _gpu_sampler(name))
    print("    passed per subset", got)


# ---- c. sphere tracing -----------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_c_sphere_tracing_stage(name):
    sg = HF.stage(name)
    st, st32 = sg.st, sg.st32
    conv, unf, p, s, t = (x.cpu() for x in RayTracer().sphere_tracing(SDFHandle(_net(name)), sg.ro.to(DEV), sg.rd.to(DEV), sg.near.to(DEV),
                                                                     sg.far.to(DEV), sg.hit.to(DEV)))
    f_conv, f_unf = int((conv != st.conv).sum()), int((unf != st.unf).sum())
    r_conv, r_unf = int((st32.conv != st.conv).sum()), int((st32.unf != st.unf).sum())     # the reference against itself
    both = conv & st.conv
    dt = float((t.double() - st.t)[both].abs().max())
    ub = unf & st.unf
    sign_bad = ub & ((s.double() < 0) != (st.s < 0)) & (st.s.abs() > sg.tau)
    print("\n[c] %-18s conv gpu/oracle %d/%d unfinished %d/%d overshoot %d/%d | flips conv %d unfinished %d (oracle fp32 vs fp64: %d, %d) | "
          "max|dt| on convergent %.2e | sign of s differs on %d" % (name, int(conv.sum()), int(st.conv.sum()), int(unf.sum()), int(st.unf.sum()),
                                                                   int((unf & (s < 0)).sum()), int((st.unf & (st.s < 0)).sum()), f_conv, f_unf,
                                                                   r_conv, r_unf, dt, int(sign_bad.sum())))
    assert int(st.unf.sum()) > 500
    if name in HF.BUMPY:
        assert int(st.conv.sum()) > 500
        assert f_conv <= 2 and f_unf <= 2
        assert dt <= TOL
        assert int(sign_bad.sum()) == 0
    else:   # slope ~20: sphere tracing is chaotic in the reference itself (tests/test_gpu_s3.py's form of allowance)
        assert f_conv <= max(2, 2 * r_conv) and f_unf <= max(2, 2 * r_unf)


# ---- d. rootfind -----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_d_rootfind_stage_on_the_oracles_brackets(name):
    """Every d_mid inside its bracket and within 2e-4 of the oracle's, reversed brackets (d_high < d_low) and two non-brackets
    included, with no exclusions.

    Leaving out the rays whose fp64 bisection branched on some |f_mid| <= tau, under a 2 % cap, is not possible: the oracle alone puts
    31-53 % of the rays there (printed below; 5-20 % even counting only branches taken while the bracket was still wider than 2e-4),
    because a bisection that ends 3e-5 wide has |f_mid| of the order of slope x 1e-5 in its last steps by construction.  Nor is it
    needed: a branch taken the other way on such a value keeps the root within tau / slope of the new end, so the two runs close in
    on the same sign change.  Measured: max |d d_mid| 7.9e-5 over all rays of all fields."""
    sg = HF.stage(name)
    sa, r = sg.sa, sg.sa.root
    f_lo, f_hi, d_lo, d_hi = (x[r].float().clone() for x in (sa.f_lo, sa.f_hi, sa.z_lo, sa.z_hi))
    oo, dd = sg.ro[sg.m][r], sg.rd[sg.m][r]
    f_lo[:2] = -1.0      # not a bracket: no step of their own, but moved by the call's shared loop
    _, want_d, _, n_iter, met = HF.bisect64(sg.f64, f_lo, f_hi, d_lo, d_hi, oo, dd, sg.prm)
    got_p, got_d, got_f = (x.cpu() for x in RayTracer().rootfind(SDFHandle(_net(name)), f_lo.to(DEV), f_hi.to(DEV), d_lo.to(DEV), d_hi.to(DEV),
                                                                 oo.to(DEV), dd.to(DEV)))
    lo, hi = torch.minimum(d_lo, d_hi), torch.maximum(d_lo, d_hi)
    outside = (got_d < lo) | (got_d > hi)
    clear = met > sg.tau
    dd_ = (got_d.double() - want_d).abs()
    print("\n[d] %-18s brackets %d (reversed %d) iterations %d | outside %d | max|dd| %.2e over all rays, %.2e over the %.1f %% that never "
          "branched on |f_mid| <= tau" % (name, int(r.sum()), int((d_hi < d_lo).sum()), n_iter, int(outside.sum()), float(dd_.max()),
                                          float(dd_[clear].max()), 100 * float(clear.float().mean())))
    assert int(outside.sum()) == 0, (name, outside.nonzero().reshape(-1).tolist())
    assert float(dd_.max()) <= TOL
    # p_mid = o + d * d_mid in fp32: two roundings of values below 8 (2^-22 each), with room for a fused multiply-add
    assert float((got_p.double() - (oo.double() + dd.double() * got_d.double().unsqueeze(-1))).abs().max()) <= 2e-6


# ---- e. the whole tracer, several chunks -------------------------------------------------------------------------------------------
def _check_trace(name, res, stats, cam, net=None):
    ref, evals_ref, _ = HF.oracle_trace(name, "fp64")
    n = HF.RES * HF.RES
    conv, rconv = res["convergent_mask"].cpu().reshape(-1), ref["convergent_mask"]
    flips = int((conv != rconv).sum())
    both = conv & rconv
    dd = float((res["distance"].cpu().reshape(-1).double() - ref["distance"])[both].abs().max())
    dp = float((res["points"].cpu().reshape(-1, 3).double() - ref["points"])[both].abs().max())
    # |sdf| at a hit: 1e-4 on S0 / S1 (tests/test_gpu_trace.py), where the slope along a ray is ~1 and a bisected hit, the mid-point of a
    # bracket <= 1e-4 wide, is <= 5e-5 from the sign change.  These fields are steeper and the fp64 oracle's own hits reach 1.0e-4 to
    # 1.24e-4 (pinned <= 2e-4 in tests/test_hard_fields_oracle.py), so a fixed figure is the wrong yardstick.  Ray by ray instead: the two
    # hits lie |d distance| apart on the same ray, so the values differ by the oracle's slope along the ray times that, plus tau for the
    # evaluation itself (test a: <= tau / 2) and the field's curvature over <= 2e-4 (HF.sdf_excess; the CPU module holds the oracle's
    # own fp32 run to the same bound)
    sdf_gpu = res["sdf"].cpu().reshape(-1)
    sdf_excess, slope = HF.sdf_excess(name, ref, sdf_gpu, res["distance"].cpu().reshape(-1), both)
    sdf_gpu = sdf_gpu[both]
    sdf, sdf_ref = float(sdf_gpu.abs().max()), float(ref["sdf"][rconv].abs().max())
    # the GPU's own unfinished count, from the stage call on the GPU camera's rays
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    _, unf, _, s, _ = RayTracer().sphere_tracing(SDFHandle(net or _net(name)), ro, rd, near, far, hit)
    print("\n[e] %-18s rays %d hits gpu/oracle %d/%d flips %d max|d distance| %.2e max|dp| %.2e max|sdf| %.2e (oracle %.2e; slope <= %.2f, max |d sdf| - bound %.2e) | unfinished %d overshoot %d "
          "roots %d | evals gpu %d ref(gpu count) %d ref(oracle) %d | %s" % (name, n, int(conv.sum()), int(rconv.sum()), flips, dd, dp, sdf,
                                                                            sdf_ref, float(slope.max()), float(sdf_excess.max()), int(unf.sum()), int((unf & (s < 0)).sum()), stats["n_bisect"],
                                                                            stats["n_evals"], stats["n_evals_ref"], evals_ref, stats))
    assert int(both.sum()) > 1000
    assert flips <= max(2, n // 1000)
    assert dd <= TOL and dp <= TOL
    assert float(sdf_excess.max()) <= 0.0, (name, float(sdf_excess.max()))
    assert bool((res["depth"].cpu().reshape(-1)[~conv] == 0.0).all())
    assert stats["n_evals"] <= stats["n_evals_ref"] and stats["n_evals"] <= evals_ref
    assert stats["n_sampler"] == int(unf.sum())
    assert stats["n_conv"] == int(conv.sum())
    assert stats.get("reserved", 0) == 0


@torch.no_grad()
@pytest.mark.parametrize("name", list(HF.BUMPY))
def test_e_whole_tracer_in_chunks(name):
    """raytrace_camera with max_num_rays = 1000 (four bisection chunks at 56 x 56) against the fp64 oracle in the same chunks."""
    _check_trace(name, *_gpu_trace(name))


# ---- f. modes --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _modes(name):
    """The sampler stage (b) and the whole tracer (e) on a net of their own (own handle: own calibration, no guard raised yet) at the
    defaults, then with the adaptive stride off, then with the screen off.  Runs only; the tests below judge.  Cached because
    test_f_some_bumpy_field_meets_the_stride_path reads the same runs."""
    lib = _lib.load()
    net = HF.build(name).to(DEV)
    rec = {"net": net, "status_before": _status(net), "runs": {}}
    samp = _gpu_sampler(name, net)
    rec["sampler"], rec["status_sampler"] = _counts(), _status(net)
    tr, stats, cam = _gpu_trace(name, net)
    rec["trace"], rec["status_trace"] = _counts(), _status(net)
    rec["runs"]["default"] = (samp, tr, stats, cam, rec["sampler"], rec["trace"])
    for mode, setter in (("stride off", lib.iron_set_sampler_stride), ("screen off", lib.iron_set_sampler_screen)):
        prev = setter(0)
        try:
            samp2 = _gpu_sampler(name, net)
            c_s = _counts()
            tr2, stats2, _ = _gpu_trace(name, net)
            c_t = _counts()
        finally:
            setter(prev)
        rec["runs"][mode] = (samp2, tr2, stats2, cam, c_s, c_t)
    return rec


@torch.no_grad()
@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_f_modes_are_bit_equal(name):
    rec = _modes(name)
    for k in ("sampler", "trace"):
        c = rec[k]
        print("\n[f] %-18s %-7s screened %d resolved %d overflow %d screen ratio %.3f | passes %d strided %d slope ratio %.3f adaptive %d | "
              "status bit 3 (screen guard) %d bit 4 (slope guard) %d" % (name, k, c["screened"], c["resolved"], c["overflow"], c["ratio"], c["passes"],
                                                                       c["strided"], c["slope"], c["adaptive"], rec["status_" + k] >> 3 & 1,
                                                                       rec["status_" + k] >> 4 & 1))
    assert rec["status_before"] & 24 == 0
    # a guard raised later is recorded above, not failed: parity with the oracle and between the modes must hold either way
    samp, tr, stats, cam, _, _ = rec["runs"]["default"]
    _check_sampler(name, samp)
    if name in HF.BUMPY:
        _check_trace(name, tr, stats, cam, rec["net"])
    for mode in ("stride off", "screen off"):
        samp2, tr2, stats2, _, c_s, c_t = rec["runs"][mode]
        if mode == "stride off":
            assert c_s["adaptive"] == 0 and c_s["strided"] == 0 and c_t["adaptive"] == 0 and c_t["strided"] == 0, (c_s, c_t)
        else:
            assert c_s["screened"] == 0 and c_t["screened"] == 0, (c_s, c_t)
        for a, b in zip(samp, samp2):
            assert torch.equal(a, b), (name, mode)
        for k in KEYS:
            assert torch.equal(tr[k], tr2[k]), (name, mode, k)
        assert stats2 == stats, (name, mode, stats2, stats)


@torch.no_grad()
def test_f_some_bumpy_field_meets_the_stride_path():
    """Otherwise none of the above would have met the adaptive march: at least one bumpy field's sampler stage strode, with no guard."""
    seen = {}
    for name in HF.BUMPY:
        rec = _modes(name)
        c = rec["sampler"]
        seen[name] = (c["adaptive"], c["strided"], rec["status_sampler"] & 24)
        if c["adaptive"] == 1 and c["strided"] > 0 and rec["status_sampler"] & 24 == 0:
            return
    raise AssertionError(seen)
