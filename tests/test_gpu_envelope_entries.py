"""GPU: the numeric envelope of the default (split-fp16, "h2") core, entry by entry and row by row (csrc/envelope.hip).

For every entry that runs a network on the h2 core and every row it returns:
  R1  finite => right: a finite value agrees with the fp64 oracle within the yardstick of tests/_envelope_cases.py; a row whose
      operands are all in range is finite and right even when other rows of the same call overflow;
  R2  wrong => flagged: numeric_status()["pending"] is true after the call iff some returned value is non-finite or outside the
      yardstick; a clean call leaves the status all-false;
  R3  afterwards exact: the next call reports exact_core, and every row is finite and right by the plain yardstick;
  R4  not vacuous: in the layer-0 probe case the rows that are dirty by the oracle come back non-finite.  The tracer and the edge
      walk return uint8 masks too: there the call leaves `pending`, and every ray (candidate) whose outcome differs from a second
      handle pinned to the exact core carries a non-finite value in sdf_out / dist / points.
The worst ratio (|kernel - fp64| / yardstick) per entry and stratum is printed; DESIGN.md 3.1b has the table."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from iron_amd import _lib, scenes

import _envelope_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CLEAN = {"overflow_seen": False, "exact_core": False, "pending": False}
DEV = torch.device("cuda", 0)


def _rows(case, idx):
    return [None if t is None else t[np.asarray(idx)].contiguous().to(DEV) for t in case.inputs]


# ---- the entries: (network on the device, inputs) -> {block: tensor} ------------------------------------------------------------
def _e_sdf(net, x):
    return {"sdf": net.sdf(x)}


def _e_get_all(net, x):                      # the reverse-mode kernel with its tape (getall_rev.hip)
    s, f, g = net.get_all(x, is_training=False)
    return {"sdf": s, "feature": f, "gradient": g}


def _e_get_all_train(net, x):                # get_all(is_training=True): the forward of the differentiable operator
    with torch.enable_grad():
        s, f, g = net.get_all(x, is_training=True)
    return {"sdf": s.detach(), "feature": f.detach(), "gradient": g.detach()}


def _e_get_all_forward_mode(net, x):         # iron_sdf_get_all without a workspace: the forward-mode kernels (k_sdf_grad_h2)
    n = x.shape[0]
    s = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    f = torch.empty((n, net.d_out - 1), dtype=torch.float32, device=x.device)
    g = torch.empty((n, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().iron_sdf_get_all(net.hip_net().handle, x.data_ptr(), n, s.data_ptr(), f.data_ptr(), g.data_ptr(), None, 0,
                                                _lib.stream_ptr(x.device)))
    return {"sdf": s, "feature": f, "gradient": g}


def _e_sdf_and_gradient(net, x):
    s, g = net.get_sdf_and_gradient(x)
    return {"sdf": s, "gradient": g}


def _e_render(net, pts, nrm, view, feat):
    return {"out": net(pts, nrm, view, feat)}


def _e_nerf(net, pts, views):
    a, c = net(pts, views)
    return {"alpha": a, "rgb": c}


SDF_ENTRIES = {"sdf": _e_sdf, "get_all": _e_get_all, "get_all_train": _e_get_all_train, "get_all_forward_mode": _e_get_all_forward_mode,
               "get_sdf_and_gradient": _e_sdf_and_gradient}
_table = {}


@pytest.fixture(scope="module", autouse=True)
def _print_the_table():
    """After the module's last test: the worst ratio |kernel - fp64| / yardstick per entry, block and stratum over the tests that
    ran.  A report, not a check: every ratio in it has been asserted <= 1 where it was measured."""
    yield
    rows = {}
    for (tag, block, stratum), r in _table.items():
        key = (tag.split("@")[0], block)
        rows.setdefault(stratum, {})[key] = max(rows.get(stratum, {}).get(key, 0.0), r)
    for stratum in E.STRATA:
        if stratum in rows:
            print("envelope table %-6s %s" % (stratum, "  ".join("%s/%s %.2f" % (k[0], k[1], v) for k, v in sorted(rows[stratum].items()))))


def _note(tag, worst):
    for k, r in worst.items():
        _table[(tag,) + k] = max(_table.get((tag,) + k, 0.0), r)


def _check(case, entry, tag, arrangement, idx):
    """One fresh handle, one call on the rows `idx`: R1, R2, R4; when the call was flagged, a second call: R3."""
    net = copy.deepcopy(case.net).to(DEV)
    ins = _rows(case, idx)
    assert net.numeric_status() == CLEAN
    got = entry(net, *ins)
    st = net.numeric_status()
    fwd = entry is _e_get_all_forward_mode
    problems, any_bad, worst, nonfinite = E.judge(case, idx, got, forward_mode=fwd)
    _note(tag, worst)
    where = "%s %s %s" % (case.name, tag, arrangement)
    assert not problems, (where, problems)                                                     # R1
    assert st["pending"] == any_bad, (where, "pending %s, a returned value is bad: %s" % (st["pending"], any_bad))   # R2
    dirty = case.stratum[np.asarray(idx)] == "dirty"
    if case.loud:
        assert bool(nonfinite[dirty].all()), (where, "%d of %d dirty rows came back finite" % (int((~nonfinite[dirty]).sum()), int(dirty.sum())))   # R4
    if not any_bad:
        assert st == CLEAN, (where, st)
        return worst
    got2 = entry(net, *ins)                                                                    # R3
    st2 = net.numeric_status()
    assert st2["overflow_seen"] and st2["exact_core"] and not st2["pending"], (where, st2)
    problems2, any_bad2, worst2, _ = E.judge(case, idx, got2, exact=True)
    _note(tag + " (exact after)", worst2)
    assert not problems2 and not any_bad2, (where, "exact core after the overflow", problems2)
    return worst


@torch.no_grad()
@pytest.mark.parametrize("entry", sorted(SDF_ENTRIES))
def test_sdf_entries_probe_in_layer_0_every_arrangement(entry):
    case = E.get_case("sdf/a")
    for name, idx in E.arrangements(case).items():
        _check(case, SDF_ENTRIES[entry], entry, name, idx)
    print(E.table_line("sdf/a " + entry, {k[1:]: v for k, v in _table.items() if k[0] == entry}))


@torch.no_grad()
@pytest.mark.parametrize("site", [s for s in E.SDF_SITES if s != "a"])
def test_sdf_entries_other_sites(site):
    """b: the next layer's column is exactly 0 (0 x inf in the h2 core); c: the BLOW_UP net; d: a probe in front of the skip layer;
    e: in the last hidden layer (the heads read fp32 accumulators: finite and right is allowed); f: coordinates of 7e4; h: G < 0,
    every row clean."""
    case = E.get_case("sdf/" + site)
    arr = E.arrangements(case)
    for entry in sorted(SDF_ENTRIES):
        if site == "f" and entry not in ("sdf", "get_all", "get_all_forward_mode"):
            continue
        tag = "%s@%s" % (entry, site)
        for name in ("n300", "last_dirty") if "last_dirty" in arr else ("n300",):
            _check(case, SDF_ENTRIES[entry], tag, name, arr[name])
        print(E.table_line("sdf/%s %s" % (site, entry), {k[1:]: v for k, v in _table.items() if k[0] == tag}))
    if site == "h":
        assert not any(s in ("dirty", "band") for s in case.stratum)


@torch.no_grad()
@pytest.mark.parametrize("key", E.RENDER_KEYS)
def test_material_nets(key):
    """RenderingNetwork.forward for the four h2 instances launch_material can pick (idr PE 0/4, no_view_dir PE 6, points_only PE 6,
    the 8-layer skip-4 PE 10/4 colour net).  g: half the rows carry features of 1e5, the ordinary half is right in the same call."""
    case = E.get_case("render/" + key)
    arr = E.arrangements(case)
    names = list(arr) if key.endswith("/a") else [n for n in ("n300", "last_dirty") if n in arr]
    for name in names:
        _check(case, _e_render, key, name, arr[name])
    print(E.table_line(key, {k[1:]: v for k, v in _table.items() if k[0] == key}))


@torch.no_grad()
@pytest.mark.parametrize("site", E.NERF_SITES)
def test_nerf(site):
    """NeRF.forward under no_grad: the probe in the points layer, and in the views layer (whose outputs the rgb head reads as fp32
    accumulators: only R1 and R2 apply), and a view component of 7e4 (alpha does not depend on the view: a dirty row placed last is
    seen by the rgb scan alone, and by its last third)."""
    case = E.get_case("nerf/" + site)
    for name, idx in E.arrangements(case).items():
        _check(case, _e_nerf, "nerf@" + site, name, idx)
    print(E.table_line("nerf/" + site, {k[1:]: v for k, v in _table.items() if k[0] == "nerf@" + site}))


@torch.no_grad()
def test_rerun_mode_on_get_all(monkeypatch):
    """IRON_H2_OVERFLOW=rerun semantics on get_all: the wrapper synchronises, sees the flag and repeats the call on the exact core."""
    import iron_amd.fields as F
    case = E.get_case("sdf/a")
    idx = E.arrangements(case)["n300"]
    monkeypatch.setattr(F, "_OVERFLOW_RERUN", True)
    net = copy.deepcopy(case.net).to(DEV)
    got = _e_get_all(net, *_rows(case, idx))
    st = net.numeric_status()
    assert st["overflow_seen"] and st["exact_core"] and not st["pending"], st
    problems, any_bad, _, _ = E.judge(case, idx, got, exact=True)
    assert not problems and not any_bad, problems


# ---- the tracer ---------------------------------------------------------------------------------------------------------------------
THR = 5.0e-5


def _tracer_setup():
    """S1's SDF net with the layer-0 probe at p = -0.3 (the dirty half-space x_0 >= 0.792 lies outside the surface and cuts the unit
    sphere the rays cross), and 2 x 144 rays of the fixture camera orbited by 35 and -55 degrees: rays that enter the unit sphere
    inside the dirty half-space, rays that only leave through it, and rays that stay 0.01 clear of it ("clean") -- over [near, far]
    and one unit beyond, because a sphere-tracing step (at most the SDF's value, < 1 inside the unit sphere) may overshoot `far` and
    the kernel, like the reference, evaluates the point it lands on."""
    from iron_amd.raytracer import Camera, intersect_sphere
    p = -0.3
    cut = p + E.F16_OVER / E.G_PROBE
    ros, rds = [], []
    for yaw in (35.0, -55.0):
        K, W2C = scenes.fixture_camera_matrices(12, 12, yaw_deg=yaw)
        cam = Camera(12, 12, K.to(DEV), W2C.to(DEV))
        ro, rd, _ = cam.get_rays(cam.get_uv())
        ros.append(ro.reshape(-1, 3))
        rds.append(rd.reshape(-1, 3))
    ro, rd = torch.cat(ros).contiguous(), torch.cat(rds).contiguous()
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    hit, near, far = hit.reshape(-1), near.reshape(-1).contiguous(), far.reshape(-1).contiguous()
    assert bool(hit.all())
    x_near, x_far = ro[:, 0] + rd[:, 0] * near, ro[:, 0] + rd[:, 0] * far
    clean = torch.maximum(x_near, ro[:, 0] + rd[:, 0] * (far + 1.0)) <= cut - 0.01
    enters_dirty = x_near >= cut + 0.01
    leaves_dirty = (x_far >= cut + 0.01) & (x_near <= cut - 0.01)
    assert int(clean.sum()) >= 60 and int(enters_dirty.sum()) >= 40 and int(leaves_dirty.sum()) >= 15

    def make(exact):
        net = E.probe_layer0(scenes.build_networks("S1")["sdf_network"], E.G_PROBE, p).to(DEV)
        if exact:
            net.force_exact(True)
        return net
    return make, ro, rd, near, far, clean, enters_dirty, leaves_dirty


def _compare_rays(tag, a, b, clean, need_lost, again):
    """a: the h2 handle's first call, b: the exact handle's, again: the h2 handle's second call.  Each (mask, points, sdf, dist)."""
    ma, pa, sa, da = a
    mb, pb, sb, db = b
    loud = ~(torch.isfinite(sa) & torch.isfinite(da) & torch.isfinite(pa).all(dim=-1))
    both = ma & mb
    differs = (ma != mb) | (both & ~((da - db).abs() <= 2e-4))
    on_thr = ((sa.abs() - THR).abs() <= 2e-5) | ((sb.abs() - THR).abs() <= 2e-5)
    print("envelope tracer %-12s rays %d: clean %d (hits %d), loud %d, outcome differs %d, of them quiet %d; clean flips on the threshold %d"
          % (tag, len(ma), int(clean.sum()), int((clean & mb).sum()), int(loud.sum()), int(differs.sum()), int((differs & ~loud).sum()),
             int((clean & (ma != mb) & on_thr).sum())))
    assert not bool((differs & ~loud & ~clean).any()), (tag, "rays with another outcome than the exact core's and plausible values",
                                                         torch.nonzero(differs & ~loud & ~clean).reshape(-1).tolist()[:8])   # R4
    assert int(loud.sum()) >= need_lost, (tag, "the case met no overflow", int(loud.sum()))
    assert not bool((loud & clean).any()), (tag, "clean rays came back non-finite")
    assert not bool((clean & (ma != mb) & ~on_thr).any()), tag
    assert not bool((clean & both & ~((da - db).abs() <= 2e-4)).any()), tag
    assert int((clean & mb).sum()) >= 5, (tag, "no clean hits")
    m2, p2, s2, d2 = again                                                                                                       # R3
    assert torch.equal(m2, mb) and torch.equal(d2, db) and torch.equal(s2, sb) and torch.equal(p2, pb), (tag, "exact after the overflow")


@torch.no_grad()
@pytest.mark.parametrize("entry", ["stage0", "stage1", "stage2", "trace"])
def test_tracer(entry):
    """iron_trace_stage 0 (sphere tracing), 1 (the dense sampler and its bisection, on intervals whose start is clean: only samples
    enter the dirty half-space -- a ray without a root must not look like a miss), 2 (the bisection on brackets that reach into it),
    and iron_trace."""
    from iron_amd.raytracer import RayTracer, SDFHandle
    make, ro, rd, near, far, clean, enters, leaves = _tracer_setup()
    sel = torch.ones_like(clean) if entry in ("stage0", "trace") else (clean | leaves)
    ro, rd, near, far, clean = ro[sel].contiguous(), rd[sel].contiguous(), near[sel].contiguous(), far[sel].contiguous(), clean[sel]
    n = ro.shape[0]
    assert 96 <= n <= 300
    work = torch.ones(n, dtype=torch.bool, device=DEV)

    def run(net):
        tr, h = RayTracer(), SDFHandle(net)
        if entry == "stage0":
            m, _, p, s, d = tr.sphere_tracing(h, ro, rd, near, far, work)
        elif entry == "stage1":
            m, p, s, d = tr.ray_sampler(h, ro, rd, near, far)
        elif entry == "stage2":     # f_low > 0 > f_high as given: the bisection walks towards d_high while the SDF stays positive
            p, d, s = tr.rootfind(h, torch.ones(n, device=DEV), -torch.ones(n, device=DEV), near, far, ro, rd)
            m = torch.ones(n, dtype=torch.bool, device=DEV)
        else:
            r = tr(h, ro, rd, near, far, work)
            m, p, s, d = r["convergent_mask"], r["points"], r["sdf"], r["distance"]
        return m.clone(), p.clone(), s.clone(), d.clone()

    h2, exact = make(False), make(True)
    assert h2.numeric_status() == CLEAN
    a = run(h2)
    st = h2.numeric_status()
    assert st["pending"], (entry, "overflowed evaluations left no flag", st)
    b = run(exact)
    again = run(h2)
    st2 = h2.numeric_status()
    assert st2["exact_core"] and st2["overflow_seen"] and not st2["pending"], st2
    _compare_rays(entry, a, b, clean, 10, again)


@torch.no_grad()
def test_tracer_clean_rays_raise_no_flag():
    from iron_amd.raytracer import RayTracer, SDFHandle
    make, ro, rd, near, far, clean, _, _ = _tracer_setup()
    ro, rd, near, far = ro[clean].contiguous(), rd[clean].contiguous(), near[clean].contiguous(), far[clean].contiguous()
    n = ro.shape[0]
    h2, exact = make(False), make(True)
    work = torch.ones(n, dtype=torch.bool, device=DEV)
    outs = []
    for net in (h2, exact):
        tr, h = RayTracer(), SDFHandle(net)
        r = tr(h, ro, rd, near, far, work)
        outs.append((r["convergent_mask"].clone(), r["points"].clone(), r["sdf"].clone(), r["distance"].clone()))
        s1 = tr.ray_sampler(h, ro, rd, near, far)
        assert bool(torch.isfinite(s1[2]).all() and torch.isfinite(s1[3]).all())
    assert h2.numeric_status() == CLEAN
    (ma, pa, sa, da), (mb, pb, sb, db) = outs
    assert bool(torch.isfinite(sa).all() and torch.isfinite(da).all() and torch.isfinite(pa).all())
    on_thr = ((sa.abs() - THR).abs() <= 2e-5) | ((sb.abs() - THR).abs() <= 2e-5)
    assert not bool(((ma != mb) & ~on_thr).any())
    assert float((da - db)[ma & mb].abs().max()) <= 2e-4 and int((ma & mb).sum()) >= 5


# ---- the edge walk ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_edge_walk():
    """iron_edge_walk on candidates on both sides of the dirty half-space (p = -0.8: x_0 >= 0.292 cuts the surface), 64 of them just
    in front of it.  A candidate whose gradient overflowed "counts as found" at its start position: it must leave with NaN points."""
    from iron_amd.raytracer import _edge_walk_fused
    p = -0.8
    cut = p + E.F16_OVER / E.G_PROBE
    g = torch.Generator().manual_seed(7)
    d = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=-1)
    start = d * (0.5 + 0.01 * torch.randn(300, 1, generator=g))
    start[:64, 0] = cut - 0.012 * torch.rand(64, generator=g) - 1e-3
    start = start.to(DEV).contiguous()
    cam_o = torch.tensor([[0.3, 0.4, 2.0]], device=DEV)
    clean = start[:, 0] <= cut - 0.03          # 17 evaluations, 16 steps of 1e-3: such a candidate cannot reach the half-space
    starts_dirty = start[:, 0] >= cut + 1e-3
    assert int(clean.sum()) >= 100 and int(starts_dirty.sum()) >= 30

    def make(exact):
        net = E.probe_layer0(scenes.build_networks("S1")["sdf_network"], E.G_PROBE, p).to(DEV)
        if exact:
            net.force_exact(True)
        return net
    def walk_by_launches(net):      # the reference's loop, one get_sdf_and_gradient launch per step: what the product falls back to
        cur, found = start.clone(), torch.zeros(300, dtype=torch.bool, device=DEV)
        for i in range(17):
            sv, gr = net.get_sdf_and_gradient(cur)
            view = cam_o - cur
            view = view / (view.norm(dim=-1, keepdim=True) + 1e-10)
            nrm = gr / (gr.norm(dim=-1, keepdim=True) + 1e-10)
            dot = (nrm * view).sum(dim=-1)
            found |= ~(dot.abs() > 5e-2)
            if i == 16:
                break
            walk = nrm - view / dot.unsqueeze(-1)
            walk = walk / (walk.norm(dim=-1, keepdim=True) + 1e-10)
            walk = walk - sv * nrm
            cur = torch.where(found.unsqueeze(-1), cur, cur + 1e-3 * walk)
        return cur, found

    h2, exact = make(False), make(True)
    pa, fa = _edge_walk_fused(h2, start, cam_o, 16, 1e-3, 5e-2)
    st = h2.numeric_status()
    pb, fb = walk_by_launches(exact)     # (the fused kernel is the h2 core's)
    loud = ~torch.isfinite(pa).all(dim=-1)
    differs = (fa != fb) | ~((pa - pb).abs().max(dim=-1).values <= 1e-4)
    print("envelope edge walk: candidates 300, clean %d, start dirty %d, loud %d, outcome differs %d, of them quiet %d, found (exact) %d"
          % (int(clean.sum()), int(starts_dirty.sum()), int(loud.sum()), int(differs.sum()), int((differs & ~loud).sum()), int(fb.sum())))
    assert st["pending"], "an overflow in the walk left no flag"
    assert bool(loud[starts_dirty].all()), "candidates that start in the dirty half-space came back with plausible points"
    assert not bool((differs & ~loud).any()), torch.nonzero(differs & ~loud).reshape(-1).tolist()[:8]       # R4
    assert not bool(loud[clean].any()) and not bool(differs[clean].any())                                   # R1
    assert int((loud & ~starts_dirty).sum()) >= 1, "no candidate walked into the half-space: the case does not test the carried bit"
    # R3: the handle is on the exact core now, which has no fused walk; the launches the product then walks with equal the pinned handle's
    assert _edge_walk_fused(h2, start, cam_o, 16, 1e-3, 5e-2) is None
    st2 = h2.numeric_status()
    assert st2["exact_core"] and st2["overflow_seen"] and not st2["pending"], st2
    p2, f2 = walk_by_launches(h2)
    assert torch.equal(p2, pb) and torch.equal(f2, fb)
    # the product's caller of the walk: a lost candidate is "found" but has no position, so it claims no pixel
    from iron_amd.raytracer import Camera, locate_edge_points
    K, W2C = scenes.fixture_camera_matrices(32, 32)
    h3 = make(False)
    out = locate_edge_points(Camera(32, 32, K.to(DEV), W2C.to(DEV)), start, h3, max_step=16, step_size=1e-3, dot_threshold=5e-2)
    assert h3.numeric_status()["pending"]
    assert int(out["edge_mask"].sum()) == out["edge_points"].shape[0] >= 1
    assert bool(torch.isfinite(out["edge_points"]).all()) and bool(torch.isfinite(out["edge_uv"]).all())


# ---- the fused shade ------------------------------------------------------------------------------------------------------------------
MATS = ("diffuse_albedo_network", "specular_albedo_network", "specular_roughness_network")


def _frame_nets(sdf_p=None, mat=None, mat_p=None, exact=False, comp=False):
    """S1's networks for iron_shade_ggx; comp: scene S2's, the SDF net and the eight material nets of iron_shade_composite."""
    nets = scenes.build_comp_networks() if comp else scenes.build_networks("S1")
    if sdf_p is not None:
        E.probe_layer0(nets["sdf_network"], E.G_PROBE, sdf_p)
    if mat is not None:
        E.probe_layer0(nets[mat], E.G_PROBE, mat_p)
    nets = {k: v.to(DEV) for k, v in nets.items()}
    if exact:
        for k, v in nets.items():
            if hasattr(v, "force_exact"):
                v.force_exact(True)
    return nets


def _frame(nets, comp=False):
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    from iron_amd.renderer_ggx import CompositeRenderer, GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn, make_render_fn_comp
    K, W2C = scenes.fixture_camera_matrices(32, 32)
    cam = Camera(32, 32, K.to(DEV), W2C.to(DEV))
    fn = make_render_fn_comp(CompositeRenderer(use_cuda=True)) if comp else make_render_fn(GGXColocatedRenderer(use_cuda=True))
    assert getattr(fn, "iron_fused_ggx", None) is not None
    res = render_camera(cam, nets["sdf_network"], RayTracer(), nets, fn, fill_holes=False, handle_edges=False)
    return cam, fn, res


def _close(a, b, tag):
    a, b = a.double(), b.double()
    assert bool(torch.isfinite(a).all()), tag
    assert float((a - b).norm() / b.norm().clamp_min(1e-30)) <= 1e-4, tag


@torch.no_grad()
@pytest.mark.parametrize("mat", ["metallic_network", "specular_albedo_network", "dielectric_eta_network"])
def test_composite_shade_with_a_probe_in_one_material_net(mat):
    """iron_shade_composite (render_camera with the composite render_fn): one 32 x 32 frame of scene S2, the probe in one of the
    eight material nets (a 1-wide head in the middle of the list, the 3-wide one, the last one).  Of the nine handles that one alone
    is flagged; its output, and the colour where it depends on it, is non-finite on the dirty hits (x_0 >= 0.192); clean hits equal
    the all-exact frame."""
    p = -0.9
    cut = p + E.F16_OVER / E.G_PROBE
    _, _, ref = _frame(_frame_nets(mat=mat, mat_p=p, exact=True, comp=True), comp=True)
    nets = _frame_nets(mat=mat, mat_p=p, comp=True)
    _, _, res = _frame(nets, comp=True)
    for k in ("sdf_network",) + scenes.COMP_ORDER:
        st = nets[k].numeric_status()
        assert st["pending"] == (k == mat) and not st["exact_core"], (k, st)
    conv = ref["convergent_mask"]
    assert torch.equal(res["convergent_mask"], conv)
    x0 = ref["points"][..., 0]
    dirty, clean = conv & (x0 >= cut + 1e-3), conv & (x0 <= cut - 1e-3)
    assert int(dirty.sum()) >= 20 and int(clean.sum()) >= 100
    own = mat[: -len("_network")]
    assert not bool(torch.isfinite(res[own][dirty].reshape(int(dirty.sum()), -1)).all(dim=-1).any()), "dirty hits came back with a plausible " + own
    if mat != "metallic_network":   # (the composite ignores the metallic weight, renderer_ggx.py:829-831; the other two reach the colour,
        # through clamps that would turn a NaN into their bound: ggx_core.h nan_of)
        assert not bool(torch.isfinite(res["color"][dirty]).all(dim=-1).any()), "dirty hits came back with a plausible colour"
    for k in ("color", "normal", "metallic", "specular_albedo", "dielectric_eta", "specular_roughness"):
        _close(res[k][clean], ref[k][clean], k)


@torch.no_grad()
def test_composite_shade_with_a_probe_sdf_net():
    """iron_shade_composite on the h2 core with the probe in the SDF net (p = -0.75), on the hits of the plain S2 frame: the SDF handle
    is flagged by the scan of its gradient and every material net by the non-finite features of the dirty hits; clean hits equal the
    same shading with every net pinned exact."""
    from iron_amd.raytracer import render_normal_and_color
    p = -0.75
    cut = p + E.F16_OVER / E.G_PROBE
    _, fn, base = _frame(_frame_nets(exact=True, comp=True), comp=True)
    base = {k: base[k] for k in ("convergent_mask", "points", "ray_o", "ray_d", "sdf", "distance", "depth") if k in base}
    nets_e, nets2 = _frame_nets(sdf_p=p, exact=True, comp=True), _frame_nets(sdf_p=p, comp=True)
    ref2, res2 = {k: v.clone() for k, v in base.items()}, {k: v.clone() for k, v in base.items()}
    render_normal_and_color(ref2, nets_e["sdf_network"], nets_e, fn)
    render_normal_and_color(res2, nets2["sdf_network"], nets2, fn)
    conv, x0 = base["convergent_mask"], base["points"][..., 0]
    dirty, clean = conv & (x0 >= cut + 1e-3), conv & (x0 <= cut - 1e-3)
    assert int(dirty.sum()) >= 20 and int(clean.sum()) >= 100
    for k in ("sdf_network",) + scenes.COMP_ORDER:
        st = nets2[k].numeric_status()
        assert st["pending"] and not st["exact_core"], (k, st)
    assert not bool(torch.isfinite(res2["color"][dirty]).all(dim=-1).any()), "dirty hits came back with a plausible colour"
    for k in ("color", "normal", "metallic", "specular_albedo"):
        _close(res2[k][clean], ref2[k][clean], k)


@torch.no_grad()
def test_fused_shade_with_a_probe_in_one_material_net():
    """One 32 x 32 render_camera frame; the specular-albedo net carries the probe on the hit point's x_0 (p = -0.9: hits with
    x_0 >= 0.192 are dirty).  Its handle alone is flagged (iron_shade_ggx scans with the device-side hit count); clean hits' pixels
    equal the frame rendered with every net pinned to the exact core."""
    mat, p = "specular_albedo_network", -0.9
    cut = p + E.F16_OVER / E.G_PROBE
    _, _, ref = _frame(_frame_nets(mat=mat, mat_p=p, exact=True))
    nets = _frame_nets(mat=mat, mat_p=p)
    _, _, res = _frame(nets)
    assert nets["sdf_network"].numeric_status() == CLEAN
    for k in MATS:
        st = nets[k].numeric_status()
        assert st["pending"] == (k == mat) and not st["exact_core"], (k, st)
    conv = ref["convergent_mask"]
    assert torch.equal(res["convergent_mask"], conv)
    x0 = ref["points"][..., 0]
    dirty, clean = conv & (x0 >= cut + 1e-3), conv & (x0 <= cut - 1e-3)
    assert int(dirty.sum()) >= 20 and int(clean.sum()) >= 100
    assert not bool(torch.isfinite(res["specular_albedo"][dirty]).all(dim=-1).any()), "dirty hits came back with a plausible albedo"
    for k in ("color", "specular_albedo", "diffuse_albedo", "normal"):
        a, b = res[k][clean].double(), ref[k][clean].double()
        assert bool(torch.isfinite(a).all()), k
        assert float((a - b).norm() / b.norm()) <= 1e-4, k


@torch.no_grad()
def test_fused_shade_with_a_probe_sdf_net():
    """The SDF net carries the probe (p = -0.75: x_0 >= 0.342 cuts the surface).  (i) render_camera: the tracer's call is the loud
    one and raises the flag, so the shading that follows in the same frame already runs the SDF net on the exact core; rays clear of
    the half-space give the pixels of the all-exact frame.  (ii) iron_shade_ggx itself on the h2 core, on the plain S1 frame's hits: the
    SDF handle is flagged, and so is every material net -- the features that reach them from a dirty hit are non-finite."""
    from iron_amd.raytracer import intersect_sphere, render_normal_and_color
    p = -0.75
    cut = p + E.F16_OVER / E.G_PROBE
    cam, fn, ref = _frame(_frame_nets(sdf_p=p, exact=True))
    nets = _frame_nets(sdf_p=p)
    _, _, res = _frame(nets)
    st = nets["sdf_network"].numeric_status()
    assert st["overflow_seen"] and st["exact_core"], st
    for k in MATS:
        assert nets[k].numeric_status() == CLEAN, k
    ro, rd = ref["ray_o"].reshape(-1, 3), ref["ray_d"].reshape(-1, 3)
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    seg = torch.maximum(ro[:, 0] + rd[:, 0] * near.reshape(-1), ro[:, 0] + rd[:, 0] * far.reshape(-1))
    clean_ray = (hit.reshape(-1) & (seg <= cut - 0.01)).reshape(ref["convergent_mask"].shape)
    ch = clean_ray & ref["convergent_mask"]
    assert int(ch.sum()) >= 50, int(ch.sum())
    on_thr = ((res["sdf"].abs() - THR).abs() <= 2e-5) | ((ref["sdf"].abs() - THR).abs() <= 2e-5)
    assert not bool((clean_ray & (res["convergent_mask"] != ref["convergent_mask"]) & ~on_thr).any())
    both = ch & res["convergent_mask"]
    a, b = res["color"][both].double(), ref["color"][both].double()
    assert bool(torch.isfinite(a).all()) and float((a - b).norm() / b.norm()) <= 1e-4
    # R4 for the frame: a pixel with another outcome than the all-exact frame's carries a non-finite traced value
    loud = ~(torch.isfinite(res["sdf"]) & torch.isfinite(res["distance"]) & torch.isfinite(res["points"]).all(dim=-1))
    differs = (res["convergent_mask"] != ref["convergent_mask"]) | (res["convergent_mask"] & ref["convergent_mask"]
                                                                    & ~((res["distance"] - ref["distance"]).abs() <= 2e-4))
    print("envelope frame (probe SDF): clean hits %d, loud rays %d, outcome differs %d, of them quiet %d"
          % (int(ch.sum()), int(loud.sum()), int(differs.sum()), int((differs & ~loud & ~on_thr).sum())))
    assert int(loud.sum()) >= 20 and not bool((differs & ~loud & ~on_thr).any())
    # (ii) the fused shade on the h2 core.  The probe pushes this net's own surface out of the dirty half-space, so the hits are those
    # of the plain S1 frame (any points may be shaded); the reference is the same shading with every net pinned exact
    _, _, base = _frame(_frame_nets(exact=True))
    base = {k: base[k] for k in ("convergent_mask", "points", "ray_o", "ray_d", "sdf", "distance", "depth") if k in base}
    nets_e, nets2 = _frame_nets(sdf_p=p, exact=True), _frame_nets(sdf_p=p)
    ref2 = {k: v.clone() for k, v in base.items()}
    res2 = {k: v.clone() for k, v in base.items()}
    render_normal_and_color(ref2, nets_e["sdf_network"], nets_e, fn)
    render_normal_and_color(res2, nets2["sdf_network"], nets2, fn)
    conv, x0 = base["convergent_mask"], base["points"][..., 0]
    dirty, clean = conv & (x0 >= cut + 1e-3), conv & (x0 <= cut - 1e-3)
    print("envelope fused shade (probe SDF): hits %d, dirty %d, clean %d" % (int(conv.sum()), int(dirty.sum()), int(clean.sum())))
    assert int(dirty.sum()) >= 20 and int(clean.sum()) >= 100
    for k in ("sdf_network",) + MATS:
        st = nets2[k].numeric_status()
        assert st["pending"] and not st["exact_core"], (k, st)
    assert not bool(torch.isfinite(res2["color"][dirty]).all(dim=-1).any()), "dirty hits came back with a plausible colour"
    for k in ("color", "normal", "specular_albedo"):
        a, b = res2[k][clean].double(), ref2[k][clean].double()
        assert bool(torch.isfinite(a).all()), k
        assert float((a - b).norm() / b.norm()) <= 1e-4, k


# ---- IRON_H2_OVERFLOW=error ---------------------------------------------------------------------------------------------------------------
def test_error_mode_in_a_child_process():
    """The mode is read once per process: overflow -> the next call is IRON_ERR_RANGE -> force_exact(True) -> the next call runs on
    the exact core and is right -> force_exact(False) clears the status (tests/run_envelope_error_check.py)."""
    env = dict(os.environ, IRON_H2_OVERFLOW="error")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "run_envelope_error_check.py")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ENVELOPE_ERROR_CHECK OK" in r.stdout
    print(r.stdout.strip().splitlines()[-1])
