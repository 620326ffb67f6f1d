"""GPU: the path integrator for interreflections (csrc/envlight.hip: k_shade_env_indirect, MeshAsset.shade_env_indirect,
render_asset_env(max_depth > 1)) against the fp64 oracle of tests/_envpath_oracle.py, which runs on the device here.

Every vertex of every path is checked from the device's own upstream state: the ray that led to it (the camera ray, or the dumped
bounce ray of the vertex before) gives the oracle's surface record, the oracle evaluates the vertex in fp64 and the dumps are
compared with that.  Bounds described as measured are the oracle's own fp32 evaluation against its fp64 one on the same inputs,
times 4, with a floor of 1e-6 (test_gpu_envlight's convention): what fp32 can give, not what the kernel gives.  Discontinuous
steps (a texel boundary, a table step, a face's edge, a horizon) are compared only where the fp64 value lies clear of the step; the
share of excluded values is capped, and tests/test_envpath_oracle.py checks the caps from the oracle alone.
"""
import ctypes as C
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
import _meshrender_oracle as O
import test_gpu_envlight as EL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
dev, tables, measured, STEP_MARGIN, STEP_SHARE = EL.dev, EL.tables, EL.measured, EL.STEP_MARGIN, EL.STEP_SHARE
HORIZON = 1e-6  # a cosine smaller than this may have either sign in fp32


@functools.lru_cache(maxsize=None)
def scene_on_device(name):
    from iron_amd.envmap import EnvMap
    from iron_amd.mesh_render import MeshAsset
    sc = PO.scene(name)
    f = lambda x: x.float().to(dev())  # noqa: E731
    asset = MeshAsset(f(sc["V"]), sc["F"].to(dev()), f(sc["uvs"]), sc["face_uvs"].to(dev()), f(sc["material"]), normals=sc["normals"])
    o, d = EO.scene_rays(sc)
    o, d = f(o), f(d)
    t, face, bary = asset.bvh.raycast(o, d)
    hot = EO.hot_map().to(dev())
    return sc, asset, (o, d, t, face, bary), EnvMap(hot.float()), EO.EnvOracle(hot), EO.EnvOracle(hot, dtype=torch.float32)


def run_paths(asset, rays, env, n_paths, max_depth, seed=PO.SEED, **kw):
    o, d, t, face, bary = rays
    out = asset.shade_env_indirect(o, d, t, face, bary, env, tables(), n_paths=n_paths, max_depth=max_depth, seed=seed, **kw)
    torch.cuda.synchronize()
    return out


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def rel(a, ref):
    return (a - ref).abs() / ref.abs().clamp_min(1e-300)


def top(x):
    """the largest entry, 0 of none"""
    return float(x.max()) if x.numel() else 0.0


def few(mask, share):
    """a share of excused rows, or one row of a small population"""
    return int(mask.sum()) <= share * mask.numel() + 1


# ---- 1. every vertex through the dumps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", PO.SETTINGS)
@pytest.mark.parametrize("name", PO.DUMP_SCENES)
def test_paths_through_the_dumps(name, setting):
    sc, asset, rays, env, e64, e32 = scene_on_device(name)
    o, d, t, face, bary = rays
    P, D = setting
    out = run_paths(asset, rays, env, P, D, dump=True)
    hit = face >= 0
    H = int(hit.sum())
    assert 100 < H < hit.numel() - 100  # hits and misses interleaved
    for k, v in out.items():
        if v.dtype == torch.float32 and k != "dump_t":
            assert torch.isfinite(v).all(), k  # under the 1e4 texel
    assert torch.equal(out["indirect_color"], out["indirect_diffuse"] + out["indirect_specular"])
    # misses: nothing cast, zeros everywhere
    assert (out["dump_face"][~hit] == -2).all()
    for k, v in out.items():
        if k != "dump_face":
            assert (v[~hit] == 0).all(), k
    n = H * P
    pix = torch.nonzero(hit)[:, 0].repeat_interleave(P)
    path = torch.arange(P, device=dev()).repeat(H)
    V, F = sc["V"].to(dev()), sc["F"].to(dev())
    NG = EO.geometric_normals(sc["V"], sc["F"]).to(dev())
    up_o, up_d, up_f = (a[hit].repeat_interleave(P, 0) for a in (o, d, face.long()))  # the ray that leads to the vertex
    reached = torch.ones(n, dtype=torch.bool, device=dev())
    T_prev = torch.ones((n, 3), dtype=torch.float64, device=dev())
    gathered = torch.zeros((n, 3), dtype=torch.float64, device=dev())
    gathered_abs = torch.zeros_like(gathered)
    worst = {}

    def note(key, err, bound):
        worst[key] = (max(worst.get(key, (0.0, 0.0))[0], err), max(worst.get(key, (0.0, 0.0))[1], bound))
        assert err <= bound, (key, j, err, bound)

    for j in range(D):
        col = lambda key: out["dump_" + key][hit][:, :, j].reshape(n, *out["dump_" + key].shape[3:])  # noqa: E731
        wb, org, fr, tt, wl, lv = col("bounce_dir"), col("bounce_org"), col("face").long(), col("t"), col("light_dir"), col("light_vis").bool()
        dl, db, lt, et, tp = col("denom_light"), col("denom_brdf"), col("light_term"), col("escape_term"), col("throughput")
        gathered += lt.double() + et.double()
        gathered_abs += lt.double().abs() + et.double().abs()
        # a vertex no path reached: no ray, zeros
        assert (fr[~reached] == -2).all()
        for a in (wb, org, tt, wl, lv, dl, db, lt, et, tp):
            assert (a[~reached] == 0).all()
        idx = torch.nonzero(reached)[:, 0]
        if idx.numel() == 0:
            continue
        wb, org, fr, tt, wl, lv, dl, db, lt, et, tp = (a[idx] for a in (wb, org, fr, tt, wl, lv, dl, db, lt, et, tp))
        Tp = T_prev[idx]
        s64 = PO.vertex_state(sc, name, up_o[idx], up_d[idx], up_f[idx])
        s32 = PO.vertex_state(sc, name, up_o[idx], up_d[idx], up_f[idx], dtype=torch.float32)
        S64 = PO.vertex_samples(e64, s64, pix[idx], path[idx], j, PO.SEED)
        S32 = PO.vertex_samples(e32, s32, pix[idx], path[idx], j, PO.SEED, dtype=torch.float32)
        m = idx.numel()
        # (a) the BRDF sample's direction
        ok_dev = (wb != 0).any(-1)
        odd = S64["ok_b"] != ok_dev  # a GGX sample whose v.h changes sign between fp32 and fp64
        assert few(odd, 1e-4)
        same = ~odd & (S32["ok_b"] == S64["ok_b"])
        note("bounce direction", top((wb.double() - S64["wb"]).abs()[~odd]), measured(S32["wb"], S64["wb"], False, keep=same[:, None].expand(-1, 3)))
        # (b) does it count, and where does its ray start
        cast = fr != -2
        cnt64 = PO.counts(s64, wb.double(), ok_dev)
        grazing = torch.minimum(EO._dot(s64["n"], wb.double()).abs(), EO._dot(s64["ng"], wb.double()).abs()) < HORIZON
        assert (cast == cnt64)[~grazing].all() and few(grazing & ok_dev, 1e-3)
        assert (org[~cast] == 0).all() and (tt[~cast] == 0).all() and (db[~cast] == 0).all()
        c = torch.nonzero(cast)[:, 0]
        org64 = EO.shadow_origin(s64["x"][c], s64["ng"][c], wb[c].double(), sc["eps_d"])
        org32 = EO.shadow_origin(s32["x"][c], s32["ng"][c], wb[c], sc["eps_d"])
        note("bounce origin", top((org[c].double() - org64).abs()), measured(org32, org64, False))
        # (c) the face it reaches, and t, against the fp64 brute force on the device's own ray
        t64, f64, _, _ = O.closest_hit(org[c].double(), wb[c].double(), V, F)
        _, margin = EO.any_hit(org[c].double(), wb[c].double(), V, F, skip=up_f[idx][c])
        bad = fr[c] != f64
        assert int((bad & (margin >= PO.EDGE_MARGIN)).sum()) == 0 and few(bad, PO.EDGE_SHARE)
        on = ~bad & (f64 >= 0)
        # t under the ray cast's own contract: |t - t64| <= 2e-6 D / |d|, D the diagonal of the mesh's box, which
        # holds the origins here.  The ray-space test forms t from the vertices' depths along the ray, so its error scales with the
        # face's extent, not with t: relative to a short t next to the crease it is far above what Moeller-Trumbore in fp32 gives.
        note("t |d| (ray cast's contract)", top(((tt[c].double() - t64).abs() * wb[c].double().norm(dim=-1))[on]), 2e-6 * sc["eps_d"] / 1e-4)
        assert (tt[c][fr[c] == -1] == INF).all()
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
            # (e) V of the device's own light direction against the fp64 brute force
            v64, vmargin, _ = EO.visibility(s64["x"], s64["n"], s64["ng"], s64["v"], wl.double(), up_f[idx], V, F, sc["eps_d"])
            vbad = (lv != v64) & ~flipped
            assert int((vbad & (vmargin >= EO.VIS_MARGIN)).sum()) == 0 and few(vbad, EO.VIS_SHARE)
            assert j > 1 or int(lv.sum()) > 0
            # (f) the light term from the device's own direction, denominator, V and upstream throughput
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
        esc = (fr == -1) & (j >= 1)
        assert (et[~esc] == 0).all()
        if esc.any():
            tex_clear = e64.texel_margin(wb.double()) >= STEP_MARGIN
            keep = esc & step_b & tex_clear & (db > 0)
            ref = Tp * e64.lookup(wb.double()) * (fd64 + fs64) / db.double().clamp_min(1e-300)[:, None]
            note("escape term", top(rel(et.double(), ref)[keep]), measured(fd32 + fs32, fd64 + fs64, True, keep=keep[:, None].expand(-1, 3)) + 6e-7)
        goes_on = (tp != 0).any(-1)
        behind = EO._dot(NG[fr.clamp(min=0)], wb.double())  # the face met is seen from its front when this is negative
        assert (goes_on == ((fr >= 0) & (behind < 0)))[behind.abs() >= HORIZON].all()
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
        # hand the paths on
        reached = torch.zeros_like(reached)
        reached[idx[goes_on]] = True
        T_prev[idx] = tp.double()
        up_o[idx], up_d[idx], up_f[idx] = org, wb, fr.clamp(min=0)
    print("%s %s: hits %d, paths %d; largest error (measured bound): %s" % (name, setting, H, n, ", ".join("%s %.3e (%.3e)" % (k, *v) for k, v in worst.items())))
    # the pixel sums against the fp64 sum of the dumped terms
    lobe_d, lobe_s = (out["dump_lobe_" + k][hit].reshape(n, 3).double() for k in ("diffuse", "specular"))
    for key, lobe in (("indirect_diffuse", lobe_d), ("indirect_specular", lobe_s)):
        ref, mag = (lobe * gathered).reshape(H, P, 3).sum(1) / P, (lobe * gathered_abs).reshape(H, P, 3).sum(1) / P
        got = out[key][hit].double()
        e = float(((got - ref).abs() / mag.clamp_min(1e-300))[mag > 0].max()) if (mag > 0).any() else 0.0
        print("%s %s: %s against the fp64 sum of the dumped terms: %.3e of the sum of absolute terms (bound 1e-5)" % (name, setting, key, e))
        assert e <= 1e-5 and (got[mag == 0] == 0).all()
    if name != "floor":
        assert float(out["indirect_color"].max()) > 0 and float(out["indirect_color"].min()) >= 0


# ---- 2. the bounce ray is the cast ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner_face", "floor"])
def test_bounce_rays_are_the_ray_cast_without_their_own_face(name):
    from iron_amd.mesh_distance import MeshBVH
    sc, asset, rays, env, _, _ = scene_on_device(name)
    P, D = PO.SETTINGS[1]
    out = run_paths(asset, rays, env, P, D, dump=True)
    face = out["dump_face"]                                                              # [n, P, D]
    own = torch.cat([rays[3][:, None, None].expand(-1, P, 1), face[:, :, :-1]], 2)       # the face a vertex's bounce ray starts on
    nf = sc["F"].shape[0]
    total = 0
    for f in range(nf):
        rows = (face != -2) & (own == f)
        if not rows.any():
            continue
        keep = torch.arange(nf) != f
        rest = MeshBVH(sc["V"].float().to(dev()), sc["F"][keep].to(dev()))
        t, g, _ = rest.raycast(out["dump_bounce_org"][rows].contiguous(), out["dump_bounce_dir"][rows].contiguous())
        back = torch.nonzero(keep)[:, 0].to(dev()).int()                                   # positions in the smaller mesh -> faces
        g = torch.where(g >= 0, back[g.clamp(min=0).long()], g)
        assert torch.equal(g, face[rows]) and torch.equal(bits(t), bits(out["dump_t"][rows])), (name, f)
        total += int(rows.sum())
    assert total == int((face != -2).sum()) > 1000 and int((face >= 0).sum()) > 100


# ---- 3. exact zeros ------------------------------------------------------------------------------------------------------------------
def scene_camera(sc, W, H):
    """raytracer.Camera at the scene's camera looking at its target (x right, y down, z forward)"""
    from iron_amd.raytracer import Camera
    cam = torch.tensor(sc["cam"], dtype=torch.float64)
    z = torch.tensor(sc["target"], dtype=torch.float64) - cam
    z = z / z.norm()
    x = torch.cross(z, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), dim=0)
    x = x / x.norm()
    y = torch.cross(z, x, dim=0)
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, cam
    K = torch.tensor([[0.9 * W, 0, W / 2, 0], [0, 0.9 * W, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)
    return Camera(W, H, K.to(dev()), torch.inverse(c2w).float().to(dev()))


@pytest.mark.parametrize("name", PO.ZERO_SCENES)
def test_no_interreflection_is_exactly_zero(name):
    from iron_amd.mesh_render import render_asset_env
    sc, asset, rays, env, _, _ = scene_on_device(name)
    P, D = PO.SETTINGS[1]
    out = run_paths(asset, rays, env, P, D, dump=True)
    assert int((rays[3] >= 0).sum()) > 100
    for k in ("indirect_diffuse", "indirect_specular", "indirect_color", "dump_light_term", "dump_escape_term"):
        assert (out[k] == 0).all(), k
    face = out["dump_face"]
    assert int((face == -1).sum()) > 1000
    if name == "floor":  # bounce rays from the floor reach the occluder's underside, which faces away: absorbed
        assert int((face >= 2).sum()) > 50 and (out["dump_throughput"][face >= 0] == 0).all()
    else:
        assert (face < 0).all()
    cam = scene_camera(sc, 40, 30)
    deep, plain = render_asset_env(cam, asset, env, n_light=8, n_brdf=8, seed=2, max_depth=3, n_paths=8), render_asset_env(cam, asset, env, n_light=8, n_brdf=8, seed=2)
    assert int(plain["convergent_mask"].sum()) > 100 and float(plain["color"].max()) > 0
    assert torch.equal(bits(deep["color"]), bits(plain["color"])) and (deep["indirect_color"] == 0).all()


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner_vertex", "floor"])
def test_bitwise_reproducible(name):
    sc, asset, rays, env, _, _ = scene_on_device(name)
    P, D = 21, 4  # a ragged last round
    out = run_paths(asset, rays, env, P, D, dump=True)
    again = run_paths(asset, rays, env, P, D, dump=True)
    plain = run_paths(asset, rays, env, P, D)
    rect = (torch.arange(31)[:, None] * 33 + torch.arange(33)[None, :])[7:20, 5:23].reshape(-1).to(dev())
    part = run_paths(asset, tuple(a[rect] for a in rays), env, P, D, pixel_idx=rect.int(), dump=True)
    assert set(plain.keys()) == {"indirect_diffuse", "indirect_specular", "indirect_color"}
    for k in out:
        assert torch.equal(bits(out[k]), bits(again[k])), k
        assert torch.equal(bits(out[k][rect]), bits(part[k])), k
        if k in plain:
            assert torch.equal(bits(out[k]), bits(plain[k])), k
    # the first two vertices of a path do not depend on max_depth
    short = run_paths(asset, rays, env, P, 2, dump=True)
    for k in short:
        if k.startswith("dump_") and not k.startswith("dump_lobe_"):
            assert torch.equal(bits(out[k][:, :, :2]), bits(short[k])), k
    assert torch.equal(out["dump_lobe_diffuse"], short["dump_lobe_diffuse"]) and torch.equal(out["dump_lobe_specular"], short["dump_lobe_specular"])
    if name != "floor":
        assert not torch.equal(out["indirect_color"], short["indirect_color"])  # the longer paths do gather more
        assert not torch.equal(run_paths(asset, rays, env, P, D, seed=PO.SEED + 1)["indirect_color"], out["indirect_color"])


# ---- 5. unbiasedness at depth 2 --------------------------------------------------------------------------------------------------------
CELLS, SUB = 48, 4     # the nested quadrature's grids
N_UNBIASED = 2048     # paths per probe pixel


def test_estimate_against_the_nested_quadrature():
    sc, asset, _, env, e64, _ = scene_on_device("corner_face")
    q = PO.probe_quadrature(str(dev()), CELLS, SUB)
    quad = q["indirect_diffuse"] + q["indirect_specular"]
    o, d = (a.float().to(dev()) for a in PO.probe_rays())
    t, face, bary = asset.bvh.raycast(o, d)
    assert torch.equal(face.long(), q["face"]) and (face[:4] < 2).all() and (face[4:] >= 2).all()  # four on the floor, four on the wall
    N = N_UNBIASED
    out = run_paths(asset, (o, d, t, face, bary), env, N, 2, seed=9, dump=True)
    # a path's value once more in fp64, from the dumped directions, faces, V and denominators
    rep = lambda a: a.repeat_interleave(N, 0)  # noqa: E731
    g = lambda key, j: out["dump_" + key][:, :, j].reshape(8 * N, *out["dump_" + key].shape[3:])  # noqa: E731
    s0 = PO.vertex_state(sc, "corner_face", rep(o), rep(d), rep(face.long()))
    wb0, f0 = g("bounce_dir", 0).double(), g("face", 0).long()
    on = (g("throughput", 0) != 0).any(-1)
    fd, fs = PO.plastic(s0, wb0, tables())
    lobes = torch.where(on[:, None], (fd + fs) / EO.brdf_pdf(s0["n"], s0["v"], wb0, s0["alpha"]).clamp_min(1e-300)[:, None], torch.zeros_like(fd))
    i1 = torch.nonzero(on)[:, 0]
    s1 = PO.vertex_state(sc, "corner_face", g("bounce_org", 0)[i1], g("bounce_dir", 0)[i1], f0[i1])
    wl, lv, dl = g("light_dir", 1)[i1].double(), g("light_vis", 1)[i1].bool(), g("denom_light", 1)[i1].double()
    wb1, esc, db = g("bounce_dir", 1)[i1].double(), g("face", 1)[i1] == -1, g("denom_brdf", 1)[i1].double()
    fl = sum(PO.plastic(s1, wl, tables()))
    fb = sum(PO.plastic(s1, wb1, tables()))
    zero = torch.zeros_like(fl)
    C = torch.where((lv & (dl > 0))[:, None], e64.lookup(wl) * fl / dl.clamp_min(1e-300)[:, None], zero) \
        + torch.where((esc & (db > 0))[:, None], e64.lookup(wb1) * fb / db.clamp_min(1e-300)[:, None], zero)
    values = torch.zeros((8 * N, 3), dtype=torch.float64, device=dev())
    values[i1] = lobes[i1] * C
    values = values.reshape(8, N, 3)
    se = values.std(1, unbiased=True) / N ** 0.5
    got = out["indirect_color"].double()
    z = ((got - quad).abs() - q["change"]).clamp_min(0) / se.clamp_min(1e-300)
    power = float((se / quad).max(1).values.median())
    print("depth 2, %d paths: estimate / nested quadrature per pixel (channel 0) %s; largest |estimate - quadrature| beyond the refinement change "
          "%.2f standard errors; standard error / quadrature: median pixel %.3e; refinement change / standard error: max %.3f; indirect / direct "
          "%.3f .. %.3f" % (N, [round(float(a), 4) for a in got[:, 0] / quad[:, 0]], float(z.max()), power, float((q["change"] / se).max()),
                            float((quad / q["direct"]).min()), float((quad / q["direct"]).max())))
    assert float((values.mean(1) - got).abs().max()) <= 1e-4 * float(got.max())  # the re-evaluation is the device's estimate
    assert (se > 0).all() and power <= 0.05                    # the comparison has power ...
    assert float((q["change"] / se).max()) <= 1.0 / 3.0        # ... and the quadrature is finer than it
    assert float(z.max()) <= 5.0


# ---- 6. render_asset_env end to end -----------------------------------------------------------------------------------------------------
def test_render_asset_env_with_interreflections(tmp_path):
    from iron_amd import _lib
    from iron_amd.envmap import EnvMap
    from iron_amd.export_materials import write_obj
    from iron_amd.mesh_render import MeshAsset, render_asset_env, render_asset_uv, subpixel_uvs
    from iron_amd.raytracer import Camera
    sc, asset, _, env, _, _ = scene_on_device("corner_vertex")
    cam = scene_camera(sc, 40, 30)
    kw = dict(n_light=8, n_brdf=8, seed=3, samples_per_axis=2)
    res = render_asset_env(cam, asset, env, max_depth=3, n_paths=8, **kw)
    direct = render_asset_env(cam, asset, env, **kw)
    assert set(res.keys()) == set(direct.keys()) | {"indirect_color"}
    m = res["coverage"] >= 1.0
    assert 100 < int(m.sum()) < 40 * 30 - 50
    assert torch.isfinite(res["color"]).all() and float(res["indirect_color"].min()) >= 0 and float(res["indirect_color"][m].mean()) > 0
    assert torch.equal(bits(res["color"]), bits(res["diffuse_color"] + res["specular_color"]))
    for k in direct:
        if k not in ("color", "diffuse_color", "specular_color"):
            assert torch.equal(res[k], direct[k]), k  # the geometry and material maps are the direct run's
    # frame by frame: the direct run's lobes plus the indirect lobes, sample k with seed + k, averaged in the same order
    dsum, ssum, isum = None, None, None
    for k, uv in enumerate(subpixel_uvs(cam, 2)):
        fr = render_asset_uv(cam, asset, 0.0, uv, env=dict(envmap=env, n_light=8, n_brdf=8, seed=3 + k, shadow_eps=1e-4))
        o, d = fr["ray_o"].reshape(-1, 3), fr["ray_d"].reshape(-1, 3)
        ind = asset.shade_env_indirect(o, d, fr["t"].reshape(-1), fr["face_idx"].reshape(-1), fr["barycentric"].reshape(-1, 2), env, tables(),
                                       n_paths=8, max_depth=3, seed=3 + k)
        dk = fr["diffuse_color"] + ind["indirect_diffuse"].reshape(30, 40, 3)
        sk = fr["specular_color"] + ind["indirect_specular"].reshape(30, 40, 3)
        ik = ind["indirect_color"].reshape(30, 40, 3)
        dsum, ssum, isum = (dk, sk, ik) if dsum is None else (dsum + dk, ssum + sk, isum + ik)
    assert torch.equal(bits(res["diffuse_color"]), bits(dsum / 4.0)) and torch.equal(bits(res["specular_color"]), bits(ssum / 4.0))
    assert torch.equal(bits(res["indirect_color"]), bits(isum / 4.0))
    # the default arguments, and max_depth = 1 spelled out, are the direct render
    same = render_asset_env(cam, asset, env, max_depth=1, n_paths=5, **kw)
    assert set(same.keys()) == set(direct.keys()) and all(torch.equal(same[k], direct[k]) for k in direct)
    # background: the pixels whose rays all hit are untouched, the others hold the map
    bg = render_asset_env(cam, asset, env, max_depth=3, n_paths=8, background=True, **kw)
    assert torch.equal(bg["color"][m], res["color"][m]) and float(bg["color"][res["coverage"] == 0].min()) > 0
    # refusals
    for bad in (dict(max_depth=0), dict(max_depth=9), dict(max_depth=2, n_paths=0), dict(max_depth=2, n_paths=(1 << 16) + 1)):
        with pytest.raises(_lib.IronError):
            render_asset_env(cam, asset, env, **bad)
    rays = scene_on_device("corner_vertex")[2]
    for bad in (dict(max_depth=1), dict(max_depth=9), dict(n_paths=0)):
        with pytest.raises(_lib.IronError):
            asset.shade_env_indirect(*rays, env, tables(), **bad)
    lib, n = _lib.load(), rays[0].shape[0]
    mesh, cenv = asset._shade_buffers(1)[1], env.c_struct()
    for n_paths, depth in ((8, 1), (8, 9), (0, 2), ((1 << 16) + 1, 2)):  # the C entry itself: IRON_ERR_BAD_ARG
        assert lib.iron_asset_shade_env_indirect(C.byref(mesh), asset.bvh.workspace.data_ptr(), C.byref(cenv), tables()[0].data_ptr(),
                                                 tables()[1].data_ptr(), rays[0].data_ptr(), rays[1].data_ptr(), rays[2].data_ptr(),
                                                 rays[3].data_ptr(), rays[4].data_ptr(), None, n, n_paths, depth, 0, 1e-4, None, None, None,
                                                 None) == -1
    # the command line on the asset written to disk: bitwise the API
    adir = os.path.join(tmp_path, "asset")
    os.makedirs(adir)
    write_obj(os.path.join(adir, "model.obj"), sc["V"].float().numpy(), sc["uvs"].float().numpy(), sc["F"].numpy(), sc["face_uvs"].numpy())
    mm = sc["material"].float().numpy()
    np.save(os.path.join(adir, "diffuse_albedo.npy"), mm[..., :3])
    np.save(os.path.join(adir, "specular_albedo.npy"), mm[..., 3:6])
    np.save(os.path.join(adir, "roughness.npy"), mm[..., 6])
    np.save(os.path.join(adir, "probe.npy"), EO.hot_map().float().numpy())
    cams = {"7.png": {"K": cam.K.cpu().reshape(-1).tolist(), "W2C": cam.W2C.cpu().reshape(-1).tolist(), "img_size": [40, 30]}}
    with open(os.path.join(adir, "cam_dict_norm.json"), "w") as fp:
        json.dump(cams, fp)
    rdir = os.path.join(tmp_path, "render")
    r = subprocess.run([sys.executable, "-m", "iron_amd.render_asset", "--mesh", os.path.join(adir, "model.obj"), "--textures", adir,
                        "--cam_dict", os.path.join(adir, "cam_dict_norm.json"), "--out", rdir, "--envmap", os.path.join(adir, "probe.npy"),
                        "--n-light", "8", "--n-brdf", "8", "--seed", "3", "--spp-axis", "2", "--max-depth", "3", "--n-paths", "8"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if os.path.exists(os.path.join(rdir, "image", "7.npy")):
        img = np.load(os.path.join(rdir, "image", "7.npy"))
    else:
        import imageio
        img = np.asarray(imageio.imread(os.path.join(rdir, "image", "7.exr")), dtype=np.float32)
    cam_json = Camera(40, 30, torch.tensor(cams["7.png"]["K"], dtype=torch.float32).reshape(4, 4).to(dev()),
                      torch.tensor(cams["7.png"]["W2C"], dtype=torch.float32).reshape(4, 4).to(dev()))
    api = render_asset_env(cam_json, MeshAsset.load(os.path.join(adir, "model.obj"), adir), EnvMap(np.load(os.path.join(adir, "probe.npy"))),
                           max_depth=3, n_paths=8, **kw)["color"].cpu().numpy()
    assert img.dtype == np.float32 and np.array_equal(img.view(np.int32), api.view(np.int32))
    assert np.abs(api - direct["color"].cpu().numpy()).max() > 0
    from PIL import Image
    png = np.asarray(Image.open(os.path.join(rdir, "image", "7.png")))
    assert np.array_equal(png[..., :3], (np.clip(np.power(api, 1 / 2.2), 0, 1) * 255).astype(np.uint8))
