"""GPU: interreflections on the neural scene (iron_amd/neural_relight.py with max_depth > 1, csrc/envlight.hip k_npath_*; DESIGN.md
§20).  The method is tests/test_gpu_envpath.py's: every vertex of every path is checked from the device's own upstream state.  The
vertex record that led to a vertex (the G-buffer pixel, or the dumped record of the bounce hit before) goes into the oracle's fp64
restatement of the samples and terms (tests/_neuralpath_oracle.py on tests/_envpath_oracle.py), and the dumped rays go back through
the product's own tracer and shading, whose answers the dumps must repeat bit for bit.

Bounds described as measured are the oracle's own fp32 evaluation against its fp64 one on the same inputs, times 4, with a floor
of 1e-6 (tests/test_gpu_envlight.py): what fp32 can give, not what the kernel gives.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _envlight_oracle as EO
import _envpath_oracle as PO
import _neuralenv_oracle as NO
import _neuralpath_oracle as NP
import test_gpu_neural_relight as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
dev, tables, measured, STEP_MARGIN, STEP_SHARE = T.dev, T.tables, T.measured, T.STEP_MARGIN, T.STEP_SHARE
SEED = NP.SEED
EPS = NP.EPS
DIRECT = dict(n_light=4, n_brdf=4)   # the direct term of the runs here: small, it is not what these tests are about
ORACLE_RAYS = 4096                   # bounce rays per setting that go through the oracle's CPU tracer (an even stride over the list)


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def rel(a, ref):
    return (a - ref).abs() / ref.abs().clamp_min(1e-300)


def top(x):
    return float(x.max()) if x.numel() else 0.0


def few(mask, share):
    return int(mask.sum()) <= share * mask.numel() + 1


@functools.lru_cache(maxsize=None)
def s0_gbuffer():
    """T.bumpy_gbuffer's recipe on the near-sphere S0"""
    from iron_amd import scenes
    from iron_amd.neural_relight import GBUFFER, _ggx_render_fn
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    K, W2C = scenes.fixture_camera_matrices(33, 31, 0.0)
    cam = Camera(33, 31, K.to(dev()), W2C.to(dev()))
    res = render_camera(cam, T.net_on_device("S0"), RayTracer(), T.material_nets(), _ggx_render_fn(), handle_edges=False)
    torch.cuda.synchronize()
    return {k: res[k].reshape(33 * 31, -1).squeeze(-1).contiguous() for k in GBUFFER}


def run(gb, name, n_paths, max_depth, seed=SEED, **kw):
    from iron_amd.neural_relight import relight_results
    from iron_amd.raytracer import RayTracer
    args = dict(DIRECT, seed=seed, max_depth=max_depth, n_paths=n_paths, color_network_dict=T.material_nets())
    args.update(kw)
    out = relight_results(gb, T.net_on_device(name), RayTracer(), T.hot_env()[0], **args)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def dumped(setting):
    """one dumped run per setting on the bumpy G-buffer, shared by the tests below and never changed"""
    return run(T.bumpy_gbuffer(), "bumpy04_s1", setting[0], setting[1], dump=True)


def surface_of(net, o, d, points, hit):
    """the product's G-buffer shading of the rays (o, d) that end at `points` where `hit`"""
    from iron_amd.neural_relight import SURFACE, _ggx_render_fn
    from iron_amd.raytracer import render_normal_and_color
    rec = {"ray_o": o, "ray_d": d, "points": points, "convergent_mask": hit}
    render_normal_and_color(rec, net, T.material_nets(), _ggx_render_fn())
    return {k: rec[k] for k in SURFACE}


# ---- 1. chunk = 1 is a call per ray --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chosen_rays():
    """48 of the recipe's shadow rays of bumpy04_s1, chosen on the CPU from the oracle's fp64 stages: 16 that sphere tracing
    converges, 16 that the sampler brackets and the bisection finishes, 16 that run free"""
    from oracle import iron_ref as R
    import _hard_fields as H
    s = NO.shadow_rays("bumpy04_s1")
    f64, _ = H.oracle_fns(NO.build("bumpy04_s1"))
    a = lambda x: x.double()  # noqa: E731
    conv, _, _, _, _ = R.sphere_tracing(f64, a(s.o), a(s.w), a(s.near), a(s.far), s.work, R.TracerParams(n_steps=H.N_STEPS))
    occ = NO.oracle_occluded("bumpy04_s1", "fp64")
    kinds = (conv & occ, ~conv & occ & s.work, ~occ & s.work)
    pick = []
    for m in kinds:
        at = torch.nonzero(m)[:, 0]
        assert at.numel() >= 16
        pick.append(at[torch.linspace(0, at.numel() - 1, 16).long()])
    return torch.cat(pick), [int(m.sum()) for m in kinds]


def test_chunk_one_is_a_call_per_ray():
    from iron_amd.neural_relight import closest_hits
    from iron_amd.raytracer import RayTracer, SDFCallable, SDFHandle
    sel, population = chosen_rays()
    s = NO.shadow_rays("bumpy04_s1")
    o, d, near, far, work = (x[sel].contiguous().to(dev()) for x in (s.o, s.w, s.near, s.far, s.work))
    net = T.net_on_device("bumpy04_s1")
    tr = RayTracer()
    both = tr.forward(SDFHandle(net), o, d, near, far, work, chunk=1)
    torch.cuda.synchronize()
    assert set(both.keys()) == {"convergent_mask", "points", "sdf", "distance"}
    for k in range(48):
        one = tr.forward(SDFHandle(net), o[k:k + 1], d[k:k + 1], near[k:k + 1], far[k:k + 1], work[k:k + 1])
        for key in both:
            assert torch.equal(bits(both[key][k:k + 1]), bits(one[key])), (key, k)
    # and with the whole-call count the bracketed rays do differ somewhere, or the test above proves nothing about chunk
    whole = tr.forward(SDFHandle(net), o, d, near, far, work)
    assert torch.equal(whole["convergent_mask"], both["convergent_mask"])
    moved = int((bits(whole["points"]) != bits(both["points"])).any(-1).sum())
    # the mask against the oracle's fp64 answer ray by ray (a ray's mask does not depend on the call it is in: it is final before
    # the bisection), within what the oracle's own fp32 run leaves open on these rays
    o64, o32 = NO.oracle_occluded("bumpy04_s1", "fp64")[sel], NO.oracle_occluded("bumpy04_s1", "fp32")[sel]
    gap, differ = int((o64 != o32).sum()), int((both["convergent_mask"].cpu() != o64).sum())
    print("chunk = 1: of %s (sphere-converged, bracketed, free) shadow rays 16 each; rays whose point differs under the whole-call count %d; "
          "mask differs from the fp64 oracle on %d (the oracle's fp32 / fp64 gap on them: %d)" % (population, moved, differ, gap))
    assert differ <= gap and moved > 0
    assert int(both["convergent_mask"][:32].sum()) >= 32 - gap and int(both["convergent_mask"][32:].sum()) <= gap
    # the opaque-callable form of the integrator's closest hit: forward(chunk = 1) on every ray that hits
    fn = SDFCallable(lambda x: net.sdf(x)[..., 0])
    slow, fast = tr.forward(fn, o, d, near, far, work, chunk=1), closest_hits(tr, fn, o, d, near, far, work)
    hit = slow["convergent_mask"]
    assert torch.equal(fast["convergent_mask"], hit) and int(hit.sum()) >= 16
    for key in ("points", "distance", "sdf"):
        assert torch.equal(bits(fast[key][hit]), bits(slow[key][hit])), key


# ---- 3. every vertex through the dumps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", NP.SETTINGS)
def test_paths_through_the_dumps(setting):
    from iron_amd.raytracer import RayTracer, SDFHandle, intersect_sphere
    gb = T.bumpy_gbuffer()
    env, e64, e32 = T.hot_env()
    net = T.net_on_device("bumpy04_s1")
    P, D = setting
    out = dumped(setting)
    hit = gb["convergent_mask"]
    H = int(hit.sum())
    assert 100 < H < hit.numel() - 100
    for k, v in out.items():
        if v.dtype == torch.float32 and k != "dump_distance":
            assert torch.isfinite(v).all(), k   # under the 1e4 texel
    assert torch.equal(out["indirect_color"], out["indirect_diffuse"] + out["indirect_specular"])
    assert (out["dump_reached"][~hit] == -2).all()
    for k, v in out.items():
        if k != "dump_reached":
            assert (v[~hit] == 0).all(), k
    n = H * P
    pix = torch.nonzero(hit)[:, 0].repeat_interleave(P)
    path = torch.arange(P, device=dev()).repeat(H)
    rep = lambda a: a[hit].repeat_interleave(P, 0)  # noqa: E731
    # the record that leads to the vertex: the G-buffer's at vertex 0
    up = {"x": rep(gb["points"]), "n": rep(gb["normal"]), "d": rep(gb["ray_d"]), "kd": rep(gb["diffuse_albedo"]),
          "ks": rep(gb["specular_albedo"]), "rough": rep(gb["specular_roughness"])}
    reached = torch.ones(n, dtype=torch.bool, device=dev())
    T_prev = torch.ones((n, 3), dtype=torch.float64, device=dev())
    gathered = torch.zeros((n, 3), dtype=torch.float64, device=dev())
    gathered_abs = torch.zeros_like(gathered)
    worst, counted = {}, {"bounce rays": 0, "hits": 0, "light rays": 0, "occluded": 0, "oracle rays": 0, "oracle differs": 0, "oracle gap": 0}
    field = NP.field("bumpy04_s1")
    tr = RayTracer()

    def note(key, err, bound):
        worst[key] = (max(worst.get(key, (0.0, 0.0))[0], err), max(worst.get(key, (0.0, 0.0))[1], bound))
        assert err <= bound, (key, j, err, bound)

    for j in range(D):
        col = lambda key: out["dump_" + key][hit][:, :, j].reshape(n, *out["dump_" + key].shape[3:])  # noqa: E731
        wb, org, code, dist, wl, lv = col("bounce_dir"), col("bounce_org"), col("reached").long(), col("distance"), col("light_dir"), col("light_vis").bool()
        dl, db, lt, et, tp = col("denom_light"), col("denom_brdf"), col("light_term"), col("escape_term"), col("throughput")
        rec = {k: col("vertex_" + k) for k in ("points", "normal", "diffuse_albedo", "specular_albedo", "roughness")}
        gathered += lt.double() + et.double()
        gathered_abs += lt.double().abs() + et.double().abs()
        assert (code[~reached] == -2).all()
        for a in (wb, org, dist, wl, lv, dl, db, lt, et, tp) + tuple(rec.values()):
            assert (a[~reached] == 0).all()
        idx = torch.nonzero(reached)[:, 0]
        if idx.numel() == 0:
            continue
        wb, org, code, dist, wl, lv, dl, db, lt, et, tp = (a[idx] for a in (wb, org, code, dist, wl, lv, dl, db, lt, et, tp))
        rec = {k: v[idx] for k, v in rec.items()}
        Tp = T_prev[idx]
        u = {k: v[idx] for k, v in up.items()}
        s64 = NP.vertex(u["x"], u["n"], u["d"], u["kd"], u["ks"], u["rough"])
        s32 = NP.vertex(u["x"], u["n"], u["d"], u["kd"], u["ks"], u["rough"], dtype=torch.float32)
        S64 = PO.vertex_samples(e64, s64, pix[idx], path[idx], j, SEED)
        S32 = PO.vertex_samples(e32, s32, pix[idx], path[idx], j, SEED, dtype=torch.float32)
        nv = EO._dot(s64["n"], s64["v"])
        # (a) the BRDF sample's direction
        ok_dev = (wb != 0).any(-1)
        odd = S64["ok_b"] != ok_dev   # a GGX sample whose v.h changes sign between fp32 and fp64
        assert few(odd, 1e-4)
        same = ~odd & (S32["ok_b"] == S64["ok_b"])
        note("bounce direction", top((wb.double() - S64["wb"]).abs()[~odd]), measured(S32["wb"], S64["wb"], False, keep=same[:, None].expand(-1, 3)))
        # (b) does it count, and where does its ray start: x + eps n in fp32, one rounding per step, bit for bit
        cast = code != -2
        cnt64 = PO.counts(s64, wb.double(), ok_dev)
        grazing = (EO._dot(s64["n"], wb.double()).abs() < NP.SIDE) | (nv.abs() < NP.SIDE)
        assert (cast == cnt64)[~grazing].all() and few(grazing & ok_dev, 1e-3)
        assert (org[~cast] == 0).all() and (dist[~cast] == 0).all() and (db[~cast] == 0).all()
        c = torch.nonzero(cast)[:, 0]
        assert torch.equal(bits(org[c]), bits(NP.origin(s32, EPS, torch.float32)[c]))
        # 3a. the bounce ray is the trace: the dumped rays through intersect_sphere, forward(chunk = 1) and the G-buffer shading
        o_c, w_c = org[c].contiguous(), wb[c].contiguous()
        work, near, far = intersect_sphere(o_c, w_c, r=1.0)
        trace = tr.forward(SDFHandle(net), o_c, w_c, near, far, work, chunk=1)
        got = trace["convergent_mask"]
        assert torch.equal(code[c], torch.where(got, 1, -1))
        assert torch.equal(bits(dist[c][got]), bits(trace["distance"][got])) and (dist[c][~got] == INF).all()
        assert torch.equal(bits(rec["points"][c][got]), bits(trace["points"][got]))
        shade = surface_of(net, o_c, w_c, trace["points"], got)
        for key, name in (("normal", "normal"), ("diffuse_albedo", "diffuse_albedo"), ("specular_albedo", "specular_albedo"),
                          ("roughness", "specular_roughness")):
            assert torch.equal(bits(rec[key][c][got]), bits(shade[name][got])), key
            assert (rec[key][c][~got] == 0).all() and (rec[key][~cast] == 0).all()
        counted["bounce rays"] += int(c.numel())
        counted["hits"] += int(got.sum())
        # 3c. hit / miss against the oracle's fp64 tracer on the same rays (an even stride over the list; the oracle runs on the CPU)
        some = torch.arange(0, c.numel(), max(1, -(-c.numel() * D // ORACLE_RAYS)), device=dev())
        m64, _, _ = field.trace(o_c[some].cpu(), w_c[some].cpu())
        m32, _, _ = field.trace(o_c[some].cpu(), w_c[some].cpu(), "fp32")
        counted["oracle rays"] += int(some.numel())
        counted["oracle differs"] += int((got[some].cpu() != m64).sum())
        counted["oracle gap"] += int((m64 != m32).sum())
        # (d) the two denominators, against the oracle's own samples
        anywhere = torch.tensor([0.3, 0.5, 0.8], dtype=torch.float64, device=dev())
        clear = (e64.texel_margin(torch.where(S64["ok_b"][:, None], S64["wb"], anywhere[None])) >= STEP_MARGIN) | ~S64["ok_b"]
        assert few(~clear, STEP_SHARE)
        den64, den32 = S64["pl_b"] + S64["pb_b"], S32["pl_b"] + S32["pb_b"]
        pos = same & clear & cast & PO.counts(s64, S64["wb"], S64["ok_b"]) & (den64 > 0) & torch.isfinite(den64)
        note("BRDF sample's denominator", top(rel(db.double(), den64)[pos]), measured(den32, den64, True, keep=pos))
        flipped = S64["gap"] <= 4
        if j >= 1:
            assert few(flipped, EO.FLIP_SHARE)
            note("light direction", top((wl.double() - S64["wl"]).abs()[~flipped]),
                 measured(S32["wl"], S64["wl"], False, keep=(~flipped)[:, None].expand(-1, 3)))
            dl64, dl32 = S64["pl_l"] + S64["pb_l"], S32["pl_l"] + S32["pb_l"]
            pos_l = ~flipped & PO.counts(s64, S64["wl"], ~flipped) & (dl64 > 0) & torch.isfinite(dl64)
            note("light sample's denominator", top(rel(dl.double(), dl64)[pos_l]), measured(dl32, dl64, True, keep=pos_l))
            # 3b. V is the query: the shadow rays rebuilt from the dumped directions, through occluded
            nw = EO._dot(s64["n"], wl.double())
            decided = (nw.abs() > NP.SIDE) & (nv.abs() > NP.SIDE)
            counting = (nw > 0) & (nv > 0) & torch.isfinite(wl).all(-1)
            shadow = decided & counting & (dl > 0)
            o_s, w_s = NP.origin(s32, EPS, torch.float32)[shadow].contiguous(), wl[shadow].contiguous()
            work, near, far = intersect_sphere(o_s, w_s, r=1.0)
            occ = torch.zeros_like(shadow)
            occ[shadow] = tr.occluded(SDFHandle(net), o_s, w_s, near, far, work)
            assert few(~decided, EO.VIS_SHARE)
            assert torch.equal(lv[shadow], ~occ[shadow]) and not bool(lv[decided & ~counting].any())
            counted["light rays"] += int(shadow.sum())
            counted["occluded"] += int(occ.sum())
            # the light term from the device's own direction, denominator, V and upstream throughput
            fd64, fs64 = PO.plastic(s64, wl.double(), tables())
            fd32, fs32 = PO.plastic(s32, wl, tables(), dtype=torch.float32)
            step_clear = (EO.table_margin(s64["n"], s64["v"], wl.double(), s64["rough"]) >= STEP_MARGIN) & ~flipped
            assert few(~step_clear, 2 * STEP_SHARE)
            lit = lv & (dl > 0) & step_clear
            L = e64.image[S64["texel"][:, 0], S64["texel"][:, 1]]
            ref = Tp * L * (fd64 + fs64) / dl.double().clamp_min(1e-300)[:, None]
            # the products with T and L and the division: one rounding each
            note("light term", top(rel(lt.double(), ref)[lit]), measured(fd32 + fs32, fd64 + fs64, True, keep=lit[:, None].expand(-1, 3)) + 6e-7)
            assert (lt[~(lv & (dl > 0))] == 0).all()
        else:
            assert (wl == 0).all() and (~lv).all() and (dl == 0).all() and (lt == 0).all()
        # (g) the BRDF sample's own terms: escape (j >= 1), the primary's lobe weights (j = 0) or the throughput
        fd64, fs64 = PO.plastic(s64, wb.double(), tables())
        fd32, fs32 = PO.plastic(s32, wb, tables(), dtype=torch.float32)
        pb64, pb32 = EO.brdf_pdf(s64["n"], s64["v"], wb.double(), s64["alpha"]), EO.brdf_pdf(s32["n"], s32["v"], wb, s32["alpha"])
        step_b = (EO.table_margin(s64["n"], s64["v"], wb.double(), s64["rough"]) >= STEP_MARGIN) & cast & ~grazing
        assert few(cast & ~step_b, 2 * STEP_SHARE)
        esc = (code == -1) & (j >= 1)
        assert (et[~esc] == 0).all()
        if esc.any():
            tex_clear = e64.texel_margin(wb.double()) >= STEP_MARGIN
            keep = esc & step_b & tex_clear & (db > 0)
            ref = Tp * e64.lookup(wb.double()) * (fd64 + fs64) / db.double().clamp_min(1e-300)[:, None]
            note("escape term", top(rel(et.double(), ref)[keep]), measured(fd32 + fs32, fd64 + fs64, True, keep=keep[:, None].expand(-1, 3)) + 6e-7)
        goes_on = (tp != 0).any(-1)
        behind = EO._dot(rec["normal"].double(), wb.double())   # the surface met is seen from its front when this is negative
        assert (goes_on == ((code == 1) & (behind < 0)))[behind.abs() >= NP.SIDE].all()
        keep = goes_on & step_b
        w64, w32 = (fd64 + fs64) / pb64[:, None], (fd32 + fs32) / pb32[:, None]
        if j == 0:
            assert (tp[goes_on] == 1).all()
            lobe_d, lobe_s = (out["dump_lobe_" + k][hit].reshape(n, 3) for k in ("diffuse", "specular"))
            assert (lobe_d[~goes_on] == 0).all() and (lobe_s[~goes_on] == 0).all()
            bound = measured(w32, w64, True, keep=keep[:, None].expand(-1, 3)) + 4e-7
            note("primary lobe weights", max(top(rel(lobe_d.double(), fd64 / pb64[:, None])[keep]),
                                             top(rel(lobe_s.double(), fs64 / pb64[:, None])[keep])), bound)
        elif keep.any():
            note("throughput", top(rel(tp.double(), Tp * w64)[keep]), measured(w32, w64, True, keep=keep[:, None].expand(-1, 3)) + 6e-7)
        # hand the paths on: the next vertex's record is the one this bounce ray reached
        reached = torch.zeros_like(reached)
        reached[idx[goes_on]] = True
        T_prev[idx] = tp.double()
        up["x"][idx], up["n"][idx], up["d"][idx] = rec["points"], rec["normal"], wb
        up["kd"][idx], up["ks"][idx], up["rough"][idx] = rec["diffuse_albedo"], rec["specular_albedo"], rec["roughness"]
    print("bumpy04_s1 %s: hits %d, paths %d; %s" % (setting, H, n, ", ".join("%s %d" % kv for kv in counted.items())))
    print("bumpy04_s1 %s: largest error (measured bound): %s" % (setting, "; ".join("%s %.3e (%.3e)" % (k, *v) for k, v in worst.items())))
    assert counted["hits"] > 1000 and 0 < counted["occluded"] < counted["light rays"]
    assert counted["oracle differs"] <= counted["oracle gap"] + EO.VIS_SHARE * counted["oracle rays"]
    # 3f. the pixel sums against the fp64 sum of the dumped terms
    lobe_d, lobe_s = (out["dump_lobe_" + k][hit].reshape(n, 3).double() for k in ("diffuse", "specular"))
    value = out["dump_path_value"][hit].reshape(n, 3).double()
    ref_v = (lobe_d + lobe_s) * gathered
    assert float(((value - ref_v).abs() / ((lobe_d + lobe_s) * gathered_abs).clamp_min(1e-300))[ref_v != 0].max()) <= 1e-5
    for key, lobe in (("indirect_diffuse", lobe_d), ("indirect_specular", lobe_s)):
        ref, mag = (lobe * gathered).reshape(H, P, 3).sum(1) / P, (lobe * gathered_abs).reshape(H, P, 3).sum(1) / P
        got = out[key][hit].double()
        e = float(((got - ref).abs() / mag.clamp_min(1e-300))[mag > 0].max()) if (mag > 0).any() else 0.0
        print("bumpy04_s1 %s: %s against the fp64 sum of the dumped terms: %.3e of the sum of absolute terms (bound 1e-5)" % (setting, key, e))
        assert e <= 1e-5 and (got[mag == 0] == 0).all()
    assert float(out["indirect_color"].max()) > 0 and float(out["indirect_color"].min()) >= 0
    # the colours are the direct run's plus these
    direct = run(gb, "bumpy04_s1", P, 1)
    assert torch.equal(bits(out["diffuse_color"]), bits(direct["diffuse_color"] + out["indirect_diffuse"]))
    assert torch.equal(bits(out["specular_color"]), bits(direct["specular_color"] + out["indirect_specular"]))
    assert torch.equal(bits(out["color"]), bits(out["diffuse_color"] + out["specular_color"]))


# ---- 4. the prefix property ----------------------------------------------------------------------------------------------------------
def test_first_vertices_do_not_depend_on_max_depth():
    from iron_amd.neural_relight import PATH_DUMPS
    deep, short = dumped(NP.SETTINGS[2]), run(T.bumpy_gbuffer(), "bumpy04_s1", NP.SETTINGS[2][0], 2, dump=True)
    assert NP.SETTINGS[2][1] == 4
    for k in PATH_DUMPS:
        assert torch.equal(bits(deep["dump_" + k][:, :, :2]), bits(short["dump_" + k])), k
    assert torch.equal(bits(deep["dump_lobe_diffuse"]), bits(short["dump_lobe_diffuse"]))
    assert torch.equal(bits(deep["dump_lobe_specular"]), bits(short["dump_lobe_specular"]))
    assert not torch.equal(deep["indirect_color"], short["indirect_color"])   # the longer paths do gather more
    assert int((deep["dump_reached"][:, :, 3] == 1).sum()) > 100


# ---- 5. nothing depends on the run or the block --------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_block_free():
    gb = T.bumpy_gbuffer()
    P, D = 21, 3   # a ragged last round
    out = run(gb, "bumpy04_s1", P, D, dump=True)
    again = run(gb, "bumpy04_s1", P, D, dump=True)
    plain = run(gb, "bumpy04_s1", P, D)
    rect = (torch.arange(31)[:, None] * 33 + torch.arange(33)[None, :])[7:20, 5:23].reshape(-1).to(dev())
    part = run({k: t[rect] for k, t in gb.items()}, "bumpy04_s1", P, D, pixel_idx=rect.int(), dump=True)
    # just above one pixel's need: one pixel per block (on the sub-rectangle: a block costs the host a wait per depth)
    small = run({k: t[rect] for k, t in gb.items()}, "bumpy04_s1", P, D, pixel_idx=rect.int(), dump=True, max_shadow_rays=P + 2)
    colours = ("color", "diffuse_color", "specular_color", "indirect_diffuse", "indirect_specular", "indirect_color")
    assert set(plain.keys()) == set(colours)
    for k in out:
        assert torch.equal(bits(out[k]), bits(again[k])), k
        assert torch.equal(bits(out[k][rect]), bits(part[k])), k
        assert torch.equal(bits(out[k][rect]), bits(small[k])), k
        if k in plain:
            assert torch.equal(bits(out[k]), bits(plain[k])), k
    assert not torch.equal(run(gb, "bumpy04_s1", P, D, seed=SEED + 1)["indirect_color"], out["indirect_color"])


# ---- 6. exact zeros and the unchanged default ----------------------------------------------------------------------------------------
def test_exact_zeros_and_the_unchanged_default():
    gb = s0_gbuffer()
    assert 100 < int(gb["convergent_mask"].sum()) < 33 * 31 - 100
    stats = {}
    deep = run(gb, "S0", 16, 3, dump=True, stats=stats)
    direct = run(gb, "S0", 16, 1, dump=True)
    from iron_amd.neural_relight import relight_results
    from iron_amd.raytracer import RayTracer
    before = relight_results(gb, T.net_on_device("S0"), RayTracer(), T.hot_env()[0], seed=SEED, dump=True, **DIRECT)
    print("S0 (16, 3): %s" % {k: v for k, v in stats.items() if k != "ms"})
    assert stats["bounce_rays"] > 1000 and stats["bounce_hits"] == 0 and stats["alive"][1:] == [0, 0]
    for k in ("indirect_color", "indirect_diffuse", "indirect_specular", "dump_light_term", "dump_escape_term", "dump_path_value"):
        assert (deep[k] == 0).all(), k
    assert (deep["dump_reached"] < 0).all() and int((deep["dump_reached"] == -1).sum()) == stats["bounce_rays"]
    assert set(direct.keys()) == set(before.keys()) == {"color", "diffuse_color", "specular_color", "dump_dir", "dump_denom", "dump_vis", "dump_contrib"}
    for k in before:
        assert torch.equal(bits(direct[k]), bits(before[k])), k          # max_depth = 1: the direct run, key for key
        assert torch.equal(bits(deep[k]), bits(before[k])), k            # and adding exact zeros changes no bit of it
    bumpy = T.bumpy_gbuffer()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(run(bumpy, "bumpy04_s1", 5, 1).values(),
                                                             T.relight(bumpy, T.net_on_device("bumpy04_s1"), T.hot_env()[0], 4, 4).values()))


# ---- 7. one estimator, two scenes ----------------------------------------------------------------------------------------------------
N_TWO = 2048


def test_one_estimator_two_scenes():
    """The crease of two boxes (tests/_neuralpath_oracle.py): the mesh integrator on its 24 faces against this one on the minimum of
    the two box distances with the boxes' face normals, fed the mesh's G-buffer, same random numbers, origins that coincide.  A wrong
    factor or a wrong rule in either shows as a difference of many standard errors; the precision is the dumps test's business.
    The tracer runs 64 sphere-tracing steps instead of 16: on an opaque callable every ray the bisection finishes is traced in a
    call of its own (neural_relight.closest_hits), and at 16 steps that is every other ray that meets the wall at a low angle."""
    from iron_amd.mesh_render import MeshAsset
    from iron_amd.neural_relight import relight_results
    from iron_amd.raytracer import RayTracer, SDFCallable
    env = T.hot_env()[0]
    sc = NP.crease()
    f = lambda x: x.float().to(dev())  # noqa: E731
    asset = MeshAsset(f(sc["V"]), sc["F"].to(dev()), f(sc["uvs"]), sc["face_uvs"].to(dev()), f(sc["material"]), normals="face")
    o, d = f(sc["ray_o"]), f(sc["ray_d"])
    t, face, bary = asset.bvh.raycast(o, d)
    assert (face >= 0).all()
    first = asset.shade_env(o, d, t, face, bary, env, tables(), n_light=1, n_brdf=1, seed=9)
    mesh = asset.shade_env_indirect(o, d, t, face, bary, env, tables(), n_paths=N_TWO, max_depth=2, seed=9, shadow_eps=EPS / sc["diag"], dump=True)
    gb = {"convergent_mask": face >= 0, "ray_d": d}
    gb.update({k: first[k] for k in ("points", "normal", "diffuse_albedo", "specular_albedo", "specular_roughness")})
    stats = {}
    ours = relight_results(gb, SDFCallable(NP.crease_sdf), RayTracer(sphere_tracing_iters=64), env, n_light=1, n_brdf=1, seed=9, shadow_eps=EPS, max_depth=2,
                           n_paths=N_TWO, surface_fn=NP.crease_surface, dump=True, stats=stats)
    torch.cuda.synchronize()
    assert torch.equal(bits(ours["dump_bounce_dir"][:, :, 0]), bits(mesh["dump_bounce_dir"][:, :, 0]))   # the same random numbers
    worst = 0.0
    for lobe in ("diffuse", "specular"):
        est, se = [], []
        for r in (ours, mesh):
            C = (r["dump_light_term"].double() + r["dump_escape_term"].double()).sum(2)    # [8, N, 3]
            v = r["dump_lobe_" + lobe].double() * C
            est.append(r["indirect_" + lobe].double())
            se.append(v.std(1, unbiased=True) / N_TWO ** 0.5)
            assert float((v.mean(1) - est[-1]).abs().max()) <= 1e-4 * float(est[-1].max())
        z = (est[0] - est[1]).abs() / (se[0] ** 2 + se[1] ** 2).sqrt().clamp_min(1e-300)
        print("two scenes, %s lobe: neural / mesh per probe (channel 0) %s; largest difference %.3f standard errors (bound 5); standard error / "
              "estimate: median %.3e" % (lobe, [round(float(a), 4) for a in est[0][:, 0] / est[1][:, 0]], float(z.max()),
                                         float((se[1] / est[1]).median())))
        assert (est[0] > 0).all() and (est[1] > 0).all()
        assert float(z.max()) <= 5.0
        worst = max(worst, float(z.max()))
    print("two scenes: bounce rays %d, hits %d (neural); mesh hits %d" % (stats["bounce_rays"], stats["bounce_hits"], int((mesh["dump_face"][:, :, 0] >= 0).sum())))


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------
def test_relight_camera_with_interreflections(tmp_path):
    from iron_amd import scenes
    from iron_amd.envmap import EnvMap
    from iron_amd.mesh_render import subpixel_uvs
    from iron_amd.neural_relight import relight_camera, relight_uv
    from iron_amd.raytracer import Camera, RayTracer
    from iron_amd.relight import load_networks
    net, nets, tr = T.net_on_device("bumpy04_s1"), T.material_nets(), RayTracer()
    K, W2C = scenes.fixture_camera_matrices(40, 30, 0.0)
    cam = Camera(40, 30, K.to(dev()), W2C.to(dev()))
    env = T.hot_env()[0]
    kw = dict(n_light=8, n_brdf=8, seed=3, samples_per_axis=2)
    res = relight_camera(cam, net, tr, nets, env, max_depth=3, n_paths=8, **kw)
    direct = relight_camera(cam, net, tr, nets, env, **kw)
    assert set(res.keys()) == set(direct.keys()) | {"indirect_color"}
    m = res["convergent_mask"]
    assert 100 < int(m.sum()) < 40 * 30 - 50
    assert torch.isfinite(res["color"]).all() and float(res["indirect_color"].min()) >= 0 and float(res["indirect_color"][m].mean()) > 0
    assert torch.equal(bits(res["color"]), bits(res["diffuse_color"] + res["specular_color"]))
    for k in direct:
        if k not in ("color", "diffuse_color", "specular_color"):
            assert torch.equal(res[k], direct[k]), k   # the geometry and material maps are the direct run's
    dsum = ssum = isum = None
    for k, uv in enumerate(subpixel_uvs(cam, 2)):
        plain = relight_uv(cam, net, tr, nets, env, uv, n_light=8, n_brdf=8, seed=3 + k)
        deep = relight_uv(cam, net, tr, nets, env, uv, n_light=8, n_brdf=8, seed=3 + k, max_depth=3, n_paths=8)
        ik = deep["indirect_color"]
        dk, sk = deep["diffuse_color"], deep["specular_color"]
        # a frame's lobes are the direct lobes plus what the paths add
        assert float((dk - plain["diffuse_color"]).min()) >= 0 and torch.equal(bits(dk + sk), bits(deep["color"]))
        assert torch.allclose((dk - plain["diffuse_color"]) + (sk - plain["specular_color"]), ik, rtol=1e-4, atol=1e-5)
        dsum, ssum, isum = (dk, sk, ik) if dsum is None else (dsum + dk, ssum + sk, isum + ik)
    assert torch.equal(bits(res["diffuse_color"]), bits(dsum / 4.0)) and torch.equal(bits(res["specular_color"]), bits(ssum / 4.0))
    assert torch.equal(bits(res["indirect_color"]), bits(isum / 4.0))
    same = relight_camera(cam, net, tr, nets, env, max_depth=1, n_paths=5, **kw)
    assert set(same.keys()) == set(direct.keys()) and all(torch.equal(same[k], direct[k]) for k in direct)
    # the command line writes the API's float image bit for bit
    full = dict(nets, sdf_network=net)
    ckpt = os.path.join(tmp_path, "ckpt_1000.pth")
    torch.save({k: v.state_dict() for k, v in full.items()}, ckpt)
    cams = {"7.png": {"K": K.reshape(-1).tolist(), "W2C": W2C.reshape(-1).tolist(), "img_size": [40, 30]}}
    with open(os.path.join(tmp_path, "cam_dict_norm.json"), "w") as fp:
        json.dump(cams, fp)
    np.save(os.path.join(tmp_path, "probe.npy"), EO.hot_map().float().numpy())
    rdir = os.path.join(tmp_path, "relit")
    r = subprocess.run([sys.executable, "-m", "iron_amd.relight", "--ckpt", ckpt, "--cam_dict", os.path.join(tmp_path, "cam_dict_norm.json"),
                        "--envmap", os.path.join(tmp_path, "probe.npy"), "--out", rdir, "--n-light", "8", "--n-brdf", "8", "--seed", "3",
                        "--samples-per-axis", "2", "--max-depth", "3", "--n-paths", "8"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if os.path.exists(os.path.join(rdir, "image", "7.npy")):
        img = np.load(os.path.join(rdir, "image", "7.npy"))
    else:
        import imageio
        img = np.asarray(imageio.imread(os.path.join(rdir, "image", "7.exr")), dtype=np.float32)
    sdf_network, mats = load_networks(ckpt, dev())
    cam_json = Camera(40, 30, torch.tensor(cams["7.png"]["K"], dtype=torch.float32).reshape(4, 4).to(dev()),
                      torch.tensor(cams["7.png"]["W2C"], dtype=torch.float32).reshape(4, 4).to(dev()))
    api = relight_camera(cam_json, sdf_network, RayTracer(), mats, EnvMap(np.load(os.path.join(tmp_path, "probe.npy"))), max_depth=3, n_paths=8,
                         **kw)["color"].cpu().numpy()
    assert img.dtype == np.float32 and img.shape == (30, 40, 3) and np.array_equal(img.view(np.int32), api.view(np.int32))
    assert np.abs(api - direct["color"].cpu().numpy()).max() > 0
    bad = subprocess.run([sys.executable, "-m", "iron_amd.relight", "--ckpt", ckpt, "--cam_dict", os.path.join(tmp_path, "cam_dict_norm.json"),
                          "--envmap", os.path.join(tmp_path, "probe.npy"), "--out", rdir, "--max-depth", "9"],
                         cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0


def test_refusals():
    import ctypes as C
    from iron_amd import _lib
    from iron_amd.neural_relight import relight_camera, relight_results
    from iron_amd.raytracer import Camera, RayTracer, SDFCallable
    from iron_amd import scenes
    gb = T.bumpy_gbuffer()
    env = T.hot_env()[0]
    net, nets, tr = T.net_on_device("bumpy04_s1"), T.material_nets(), RayTracer()
    # ranges
    for bad in (dict(max_depth=0), dict(max_depth=9), dict(max_depth=2.5), dict(max_depth=2, n_paths=0), dict(max_depth=2, n_paths=(1 << 16) + 1)):
        with pytest.raises(_lib.IronError):
            relight_results(gb, net, tr, env, color_network_dict=nets, **bad)
    K, W2C = scenes.fixture_camera_matrices(8, 8, 0.0)
    cam = Camera(8, 8, K.to(dev()), W2C.to(dev()))
    for bad in (dict(max_depth=0), dict(max_depth=9), dict(max_depth=2, n_paths=0)):
        with pytest.raises(_lib.IronError):
            relight_camera(cam, net, tr, nets, env, **bad)
    with pytest.raises(_lib.IronError):
        relight_results(gb, net, tr, env, max_depth=2, n_paths=64, max_shadow_rays=63, color_network_dict=nets)
    # nothing to shade the bounce hits with
    with pytest.raises(_lib.IronError):
        relight_results(gb, net, tr, env, max_depth=2)
    fn = SDFCallable(lambda x: net.sdf(x)[..., 0])
    with pytest.raises(_lib.IronError):
        relight_results(gb, fn, tr, env, max_depth=2, color_network_dict=nets)
    # a surface_fn that returns the wrong keys or shapes
    good = lambda x, d: {"normal": x / x.norm(dim=-1, keepdim=True), "diffuse_albedo": torch.full_like(x, 0.5),  # noqa: E731
                         "specular_albedo": torch.full_like(x, 0.3), "specular_roughness": torch.full_like(x[:, 0], 0.4)}
    few_hits = torch.nonzero(gb["convergent_mask"])[:12, 0]
    small = {k: v[few_hits] for k, v in gb.items()}
    ok = relight_results(small, fn, tr, env, max_depth=2, n_paths=4, surface_fn=good, **DIRECT)
    assert torch.isfinite(ok["indirect_color"]).all()
    for spoil in (lambda r: {k: v for k, v in r.items() if k != "normal"}, lambda r: dict(r, specular_roughness=r["specular_roughness"][:, None]),
                  lambda r: dict(r, normal=r["normal"][:-1]), lambda r: dict(r, diffuse_albedo=r["diffuse_albedo"].double()),
                  lambda r: dict(r, specular_albedo=r["specular_albedo"].cpu()), lambda r: None):
        with pytest.raises(_lib.IronError):
            relight_results(small, fn, tr, env, max_depth=2, n_paths=4, surface_fn=lambda x, d, spoil=spoil: spoil(good(x, d)), **DIRECT)
    with pytest.raises(_lib.IronError):
        relight_results(small, fn, tr, env, max_depth=2, n_paths=4, surface_fn=3, **DIRECT)
    # CPU tensors
    with pytest.raises(_lib.IronError):
        relight_results({k: v.cpu() for k, v in gb.items()}, net, tr, env, max_depth=2, color_network_dict=nets)
    # the C entries themselves: IRON_ERR_BAD_ARG for the ranges
    lib = _lib.load()
    hit = gb["convergent_mask"]
    g = _lib.iron_neural_gbuffer(hit.data_ptr(), gb["points"].data_ptr(), gb["normal"].data_ptr(), gb["ray_d"].data_ptr(),
                                 gb["diffuse_albedo"].data_ptr(), gb["specular_albedo"].data_ptr(), gb["specular_roughness"].data_ptr(), None,
                                 hit.shape[0])
    size = C.c_size_t(0)
    assert lib.iron_neural_path_workspace_bytes(0, C.byref(size)) == -1 and lib.iron_neural_path_workspace_bytes(64, None) == -1
    assert lib.iron_neural_path_workspace_bytes(64, C.byref(size)) == 0 and size.value > 64 * 28 * 4
    ws = torch.empty(size.value, dtype=torch.uint8, device=dev())
    for n_paths, depth in ((8, 1), (8, 9), (0, 2), ((1 << 16) + 1, 2)):
        assert lib.iron_neural_path_begin(C.byref(g), 0, 1, n_paths, depth, 64, ws.data_ptr(), ws.numel(), None) == -1
        assert lib.iron_neural_path_finish(C.byref(g), 0, 1, n_paths, depth, 64, ws.data_ptr(), ws.numel(), None, None, None, None) == -1
    assert lib.iron_neural_path_begin(C.byref(g), 0, 9, 8, 2, 64, ws.data_ptr(), ws.numel(), None) == -1   # 72 slots in a workspace of 64
