"""GPU: the environment render (csrc/envlight.hip, iron_amd/envmap.py, iron_amd/mesh_render.py) against the fp64
oracle of tests/_envlight_oracle.py, which runs on the device here.  No Mitsuba render exists: the feature is pinned to the oracle
and to closed forms.

Bounds described as measured are the oracle's own fp32 evaluation against its fp64 one on the same inputs, times 4, with a floor
of 1e-6: what fp32 can give, not what the kernel gives.  Discontinuous steps (a texel boundary, a table step, a face's edge) are
compared only where the oracle's fp64 value lies clear of the step; the share of excluded values is capped.
"""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _envlight_oracle as EO
import _meshdist_oracle as MO
import _meshrender_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
STEP_MARGIN = 1e-4  # texel / table-step coordinates closer than this to a step may resolve either way in fp32
STEP_SHARE = 5e-3


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def tables():
    from iron_amd.renderer_ggx import load_mts_tables
    return tuple(t.to(dev()) for t in load_mts_tables())


def measured(a32, a64, relative, keep=None):
    """4 x the largest error of the oracle's fp32 evaluation against its fp64 one, floor 1e-6"""
    e = (a32.double() - a64).abs()
    if relative:
        e = e / a64.abs().clamp_min(1e-300)
    if keep is not None:
        e = e[keep]
    return max(4 * float(e.max()) if e.numel() else 0.0, 1e-6)


# ---- 1. occlusion ------------------------------------------------------------------------------------------------------------------
def bvh_of(V, F):
    from iron_amd.mesh_distance import MeshBVH
    return MeshBVH(V.float().to(dev()), F.to(dev()))


def random_rays(n, seed, lo=-2.0, hi=3.0):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand((n, 3), generator=g, dtype=torch.float64) * (hi - lo) + lo).float()
    target = torch.rand((n, 3), generator=g, dtype=torch.float64) * 1.4 - 0.2
    d = target - o.double()
    d = d / d.norm(dim=1, keepdim=True) * (0.25 + 3.5 * torch.rand((n, 1), generator=g, dtype=torch.float64))  # not unit length
    return o.to(dev()), d.float().to(dev())


def occlusion_meshes():
    one = (torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, 0.5]], dtype=torch.float64), torch.tensor([[0, 1, 2]]))
    two = (torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.5]], dtype=torch.float64),
           torch.tensor([[0, 1, 2], [2, 1, 3]]))
    soup = MO.triangle_soup(2000)
    return {"triangle": one, "two_triangles": two, "cube": MO.unit_cube(), "tetrahedron": MO.regular_tetrahedron(),
            "soup": (soup[0].float().double(), soup[1])}


@pytest.mark.parametrize("name", ["triangle", "two_triangles", "cube", "tetrahedron", "soup", "sphere_edges"])
def test_occluded_is_the_closest_hit_casts_mask(name):
    if name == "sphere_edges":  # rays through the vertices and edges of the sphere
        V, F = O.uv_sphere(48, 96, 0.6)
        cam = torch.tensor((0.4, 0.3, 2.2), dtype=torch.float64).float().double()
        tg = O.edge_targets(V, F, cam, n=3000, min_cos=0.2, seed=1)
        d = (tg - cam[None]).float().to(dev())
        o = cam[None].expand(d.shape[0], 3).float().contiguous().to(dev())
        windows = ((0.0, INF), (0.0, 1.7), (1.7, INF))
    else:
        V, F = occlusion_meshes()[name]
        o, d = random_rays(4000, seed=3)
        special_o = torch.tensor([[-1, 0.5, 0.25], [float("nan"), 0.5, 0.25], [-1, 0.5, 0.25], [-1, float("inf"), 0.25], [-1, 0.5, 0.25]])
        special_d = torch.tensor([[0.0, 0, 0], [1, 0, 0], [float("inf"), 0, 0], [1, 0, 0], [float("nan"), 1, 0]])
        o, d = torch.cat([o, special_o.to(dev())]), torch.cat([d, special_d.to(dev())])
        windows = ((0.0, INF), (0.9, INF), (0.0, 1.1), (0.9, 1.6), (1.2, 1.2), (2.0, 1.0))
    bvh = bvh_of(V, F)
    t0, f0, _ = bvh.raycast(o, d)
    for t_min, t_max in windows:
        f = bvh.raycast(o, d, t_min=t_min, t_max=t_max)[1]
        occ = bvh.occluded(o, d, t_min=t_min, t_max=t_max)
        assert occ.dtype == torch.uint8 and torch.equal(occ.bool(), f >= 0), (name, t_min, t_max)
        assert torch.equal(occ, bvh.occluded(o, d, t_min=t_min, t_max=t_max, skip_face=torch.full_like(f0, -1)))
    if name != "sphere_edges":
        assert not bvh.occluded(o[-5:], d[-5:]).any()  # the zero and the non-finite rays
        assert 0 < int((f0 >= 0).sum()) < o.shape[0]
        # a finite window that cuts the nearer hit: where the closest hit lies beyond t_max nothing is reported
        cut = bvh.occluded(o, d, t_max=0.75)
        assert torch.equal(cut.bool(), (f0 >= 0) & (t0 <= 0.75))
    # skip_face = a ray's closest face: the answer of a closest-hit cast on the mesh without that face
    if F.shape[0] > 1:
        hit_faces = torch.unique(f0[f0 >= 0]).tolist()[:6]
        for g in hit_faces:
            rays = f0 == g
            keep = torch.arange(F.shape[0]) != g
            rest = bvh_of(V, F[keep]).raycast(o[rays], d[rays])[1]
            got = bvh.occluded(o[rays], d[rays], skip_face=f0[rays])
            assert torch.equal(got.bool(), rest >= 0), (name, g)
    else:
        assert not bvh.occluded(o, d, skip_face=torch.zeros_like(f0)).any()


# ---- 2. the environment map --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1", "2x3", "16x32", "holes", "rotated"])
def test_envmap_sample_pdf_lookup_against_the_oracle(name):
    from iron_amd.envmap import EnvMap
    R = None
    if name == "rotated":
        c, s = math.cos(0.7), math.sin(0.7)
        R = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64) @ torch.tensor([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=torch.float64)
        R = R.float().double()
    img = EO.env_maps()["16x32" if name == "rotated" else name].to(dev())
    env = EnvMap(img.float(), to_world=None if R is None else R.numpy())
    e64 = EO.EnvOracle(img, None if R is None else R.to(dev()))
    e32 = EO.EnvOracle(img, None if R is None else R.to(dev()), dtype=torch.float32)
    u = EO.sample_inputs().to(dev())
    tx, d, p = env.sample(u.float())
    t64, d64, p64 = e64.sample(u)
    gap = e64.boundary_gap
    t32, d32, p32 = e32.sample(u)
    flip = (tx.long() != t64).any(-1)
    same = ~flip
    bd, bp = measured(d32, d64, False), measured(p32, p64, True)
    ed = float((d.double() - d64)[same].abs().max())
    ep = float(((p.double() - p64).abs() / p64)[same].max())
    print("%s: sample: texel flips %d of %d (all within 4 ulps of a boundary: %s), |dir error| %.3e (measured bound %.3e), pdf rel error %.3e "
          "(measured bound %.3e)" % (name, int(flip.sum()), u.shape[0], bool((gap[flip] <= 4).all()), ed, bd, ep, bp))
    assert (gap[flip] <= 4).all() and float(flip.double().mean()) <= EO.FLIP_SHARE
    assert ed <= bd and ep <= bp
    assert (e64.weight[tx[:, 0].long(), tx[:, 1].long()] > 0).all()  # a texel of weight 0 is never returned
    assert float((d.norm(dim=1) - 1).abs().max()) <= 1e-6
    # pdf and lookup at arbitrary directions (not unit length), away from texel boundaries
    g = torch.Generator().manual_seed(41)
    q = (EO._unit(torch.randn((100000, 3), generator=g, dtype=torch.float64)) * (0.5 + torch.rand((100000, 1), generator=g, dtype=torch.float64)))
    q = q.float().to(dev())
    clear = e64.texel_margin(q.double()) >= STEP_MARGIN
    pq, lq = env.pdf(q), env.lookup(q)
    pq64, pq32 = e64.pdf(q.double()), e32.pdf(q.double())
    bq = measured(pq32, pq64, True, keep=clear & (pq64 > 0))
    eq = float(((pq.double() - pq64).abs() / pq64.clamp_min(1e-300))[clear & (pq64 > 0)].max()) if bool((pq64 > 0).any()) else 0.0
    print("%s: pdf(dir) rel error %.3e (measured bound %.3e), share of directions within %g texel of a boundary %.2e"
          % (name, eq, bq, STEP_MARGIN, 1 - float(clear.double().mean())))
    assert float((~clear).double().mean()) <= STEP_SHARE
    assert eq <= bq
    assert (pq[clear & (pq64 == 0)] == 0).all()
    assert torch.equal(lq[clear], e64.lookup(q.double())[clear].float())
    # the density of a sampled direction is the sample's own
    again = env.pdf(d)
    ok = e64.texel_margin(d.double()) >= STEP_MARGIN
    assert float(((again - p).abs() / p)[ok].max()) <= 4 * bp + 1e-5


def test_envmap_black_and_refusals():
    from iron_amd._lib import IronError
    from iron_amd.envmap import EnvMap
    env = EnvMap(np.zeros((4, 8, 3), dtype=np.float32))
    u = EO.sample_inputs(1000).float().to(dev())
    tx, d, p = env.sample(u)
    assert (p == 0).all() and torch.isfinite(d).all() and (tx == 0).all()
    assert (env.pdf(d) == 0).all() and (env.lookup(d) == 0).all()
    for bad in (-1.0, float("nan"), float("inf")):
        img = np.ones((2, 2, 3), dtype=np.float32)
        img[1, 0, 2] = bad
        with pytest.raises(IronError):
            EnvMap(img)
    with pytest.raises(IronError):
        EnvMap(torch.ones((2, 2, 3)))  # a CPU tensor


# ---- 3. the BRDF -------------------------------------------------------------------------------------------------------------------
def brdf_inputs(m, seed, extreme):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)  # noqa: E731
    n = EO._unit(torch.randn((m, 3), generator=g, dtype=torch.float64))

    def about(cos_lo, cos_hi):
        c = cos_lo + (cos_hi - cos_lo) * r(m)
        t = EO._unit(torch.cross(n, torch.randn((m, 3), generator=g, dtype=torch.float64), dim=-1))
        return c[:, None] * n + torch.sqrt(1 - c * c)[:, None] * t
    if not extreme:
        v, l = about(0.05, 0.999), about(0.05, 0.999)
        rough = 0.02 + 0.98 * r(m)
    else:
        v, l = about(-0.2, 1.0), about(-0.3, 1.0)
        k = m // 5
        v[:k] = about(1e-6, 1e-3)[:k]            # grazing view
        l[k:2 * k] = about(1e-6, 1e-3)[k:2 * k]  # grazing light
        rough = r(m)
        rough[2 * k:3 * k] = 1e-4                 # at the clamp
        rough[3 * k:4 * k] = 1e-4 * r(k)          # below it
    f = lambda x: x.float().to(dev())  # noqa: E731
    return f(n), f(v), f(l), f(r(m, 3)), f(r(m, 3)), f(rough)


@pytest.mark.parametrize("extreme", [False, True])
def test_roughplastic_point_against_the_oracle(extreme):
    from iron_amd import _lib
    m = 10000
    n, v, l, kd, ks, rough = brdf_inputs(m, 51, extreme)
    d = torch.empty((m, 3), device=dev())
    s = torch.empty((m, 3), device=dev())
    tt, td = tables()
    _lib.check(_lib.load().iron_roughplastic(n.data_ptr(), v.data_ptr(), l.data_ptr(), kd.data_ptr(), ks.data_ptr(), rough.data_ptr(),
                                             tt.data_ptr(), td.data_ptr(), m, d.data_ptr(), s.data_ptr(), _lib.stream_ptr(dev())))
    d64, s64 = EO.roughplastic_point(n, v, l, kd, ks, rough, (tt, td))
    d32, s32 = EO.roughplastic_point(n, v, l, kd, ks, rough, (tt, td), dtype=torch.float32)
    clear = EO.table_margin(n, v, l, rough) >= STEP_MARGIN
    lit = EO._dot(n.double(), l.double()) > 1e-7
    dark = EO._dot(n.double(), l.double()) < -1e-7
    keep = (clear & lit)[:, None].expand(m, 3)
    bd, bs = measured(d32, d64, True, keep=keep), measured(s32, s64, True, keep=keep)
    ed = float(((d.double() - d64).abs() / d64.abs().clamp_min(1e-300))[keep].max())
    es = float(((s.double() - s64).abs() / s64.abs().clamp_min(1e-300))[keep].max())
    print("roughplastic_point (%s): lit %d, dark %d, near a table step %d; diffuse rel error %.3e (measured bound %.3e), specular rel error "
          "%.3e (measured bound %.3e)" % ("clamps and grazing" if extreme else "moderate", int(lit.sum()), int(dark.sum()), int((~clear).sum()),
                                         ed, bd, es, bs))
    assert float((~clear).double().mean()) <= STEP_SHARE
    assert ed <= bd and es <= bs
    assert (d[dark] == 0).all() and (s[dark] == 0).all()
    assert torch.isfinite(d).all() and torch.isfinite(s).all()
    if extreme:
        assert int(dark.sum()) > 500
    else:  # l = v: the co-located head with intensity 1 (kFr is the 4-digit rounding of the computed Fresnel term)
        from iron_amd.renderer_ggx import GGXColocatedRenderer
        _lib.check(_lib.load().iron_roughplastic(n.data_ptr(), v.data_ptr(), v.data_ptr(), kd.data_ptr(), ks.data_ptr(), rough.data_ptr(),
                                                 tt.data_ptr(), td.data_ptr(), m, d.data_ptr(), s.data_ptr(), _lib.stream_ptr(dev())))
        out = GGXColocatedRenderer(use_cuda=True)(1.0, torch.ones((m, 1), device=dev()), n, v,
                                                  {"diffuse_albedo": kd, "specular_albedo": ks, "specular_roughness": rough[:, None]})
        rs = float(((s - out["specular_rgb"]).abs() / out["specular_rgb"]).max())
        rd = float(((d - out["diffuse_rgb"]).abs() / out["diffuse_rgb"]).max())
        print("l = v against the co-located head: specular rel %.3e, diffuse rel %.3e" % (rs, rd))
        assert rs <= 2e-4 and rd <= 1e-6


# ---- 4. the integrator, through the dumps --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_on_device(name, below=False):
    from iron_amd.envmap import EnvMap
    from iron_amd.mesh_render import MeshAsset
    sc = EO.scene(name)
    f = lambda x: x.float().to(dev())  # noqa: E731
    asset = MeshAsset(f(sc["V"]), sc["F"].to(dev()), f(sc["uvs"]), sc["face_uvs"].to(dev()), f(sc["material"]), normals=sc["normals"])
    if below:
        sc = dict(sc, cam=(sc["cam"][0], -sc["cam"][1], sc["cam"][2]))
    o, d = EO.scene_rays(sc)
    o, d = f(o), f(d)
    t, face, bary = asset.bvh.raycast(o, d)
    hot = EO.hot_map().to(dev())
    return sc, asset, (o, d, t, face, bary), EnvMap(hot.float()), EO.EnvOracle(hot), EO.EnvOracle(hot, dtype=torch.float32)


def run_env(asset, rays, env, n_light, n_brdf, seed=5, **kw):
    o, d, t, face, bary = rays
    out = asset.shade_env(o, d, t, face, bary, env, tables(), n_light=n_light, n_brdf=n_brdf, seed=seed, **kw)
    torch.cuda.synchronize()
    return out


def per_sample(x, N):
    return x[:, None].expand(x.shape[0], N, *x.shape[1:]).reshape(-1, *x.shape[1:])


@pytest.mark.parametrize("counts", [(5, 3), (8, 0), (0, 8), (64, 64), (100, 30)])
@pytest.mark.parametrize("name", ["floor", "cube"])
def test_integrator_through_the_dumps(name, counts):
    from iron_amd import _lib
    sc, asset, rays, env, e64, e32 = scene_on_device(name)
    o, d, t, face, bary = rays
    n_light, n_brdf = counts
    N = n_light + n_brdf
    out = run_env(asset, rays, env, n_light, n_brdf, dump=True)
    hit = face >= 0
    P = int(hit.sum())
    assert 100 < P < hit.numel() - 100  # hits and misses interleaved
    pix = torch.nonzero(hit)[:, 0]
    nrm, x, v = out["normal"][hit].double(), out["points"][hit].double(), -d[hit].double()
    kd, ks, rough = out["diffuse_albedo"][hit].double(), out["specular_albedo"][hit].double(), out["specular_roughness"][hit].double()
    alpha = rough.clamp(min=1e-4)
    ng = EO.geometric_normals(sc["V"], sc["F"]).to(dev())[face[hit].long()]
    w = out["dump_dir"][hit].reshape(-1, 3).double()
    den = out["dump_denom"][hit].reshape(-1).double()
    vis = out["dump_vis"][hit].reshape(-1).bool()
    con = out["dump_contrib"][hit].reshape(-1, 3).double()
    # (a) directions and denominators against the oracle's, from the restated random numbers
    S64 = EO.pixel_samples(e64, nrm, v, alpha, pix, n_light, n_brdf, 5)
    S32 = EO.pixel_samples(e32, nrm, v, alpha, pix, n_light, n_brdf, 5, dtype=torch.float32)
    flipped = S64["gap"] <= 4
    odd = S64["ok"] != (w != 0).any(-1)  # a GGX sample whose v.h changes sign between fp32 and fp64
    # a BRDF sample's direction is looked up in the map: clear of a texel boundary, or no sample at all (nothing is looked up)
    anywhere = torch.tensor([0.3, 0.5, 0.8], dtype=torch.float64, device=dev())
    clear = (e64.texel_margin(torch.where(S64["ok"][:, None], S64["dir"], anywhere[None])) >= STEP_MARGIN) | ~S64["ok"]
    is_light = (torch.arange(N, device=dev()) < n_light)[None].expand(P, N).reshape(-1)
    good = ~flipped & ~odd & (clear | is_light)
    bdir = measured(S32["dir"], S64["dir"], False, keep=(good & (S32["ok"] == S64["ok"]))[:, None].expand(-1, 3))
    # denominators are compared where the sample can count at all: above the shading horizon and on the viewer's side of the face
    # (opposite the viewer, v + w cancels and the half vector of the GGX density is rounding noise in fp32; V is 0 there anyway)
    n_s, ng_s, v_s = per_sample(nrm, N), per_sample(ng, N), per_sample(v, N)
    side = (EO._dot(n_s, S64["dir"]) > 0) & (EO._dot(ng_s, S64["dir"]) * EO._dot(ng_s, v_s) > 0)
    pos = good & side & (S64["denom"] > 0) & torch.isfinite(S64["denom"])
    bden = measured(S32["denom"], S64["denom"], True, keep=pos & (S32["ok"] == S64["ok"]))
    edir = float((w - S64["dir"]).abs()[good].max())
    eden = float(((den - S64["denom"]).abs() / S64["denom"].clamp_min(1e-300))[pos].max())
    print("%s %s: hits %d, samples %d; near a CDF boundary %d, v.h sign changes %d, near a texel boundary %d; |dir error| %.3e (measured "
          "bound %.3e), denominator rel error %.3e (measured bound %.3e)"
          % (name, counts, P, P * N, int(flipped.sum()), int(odd.sum()), int((~clear & ~is_light).sum()), edir, bdir, eden, bden))
    assert float(flipped.double().mean()) <= EO.FLIP_SHARE and float(odd.double().mean()) <= 1e-4
    assert float((~clear & ~is_light).double().mean()) <= STEP_SHARE
    assert edir <= bdir and eden <= bden
    assert (den[good & (S64["denom"] == 0)] == 0).all()
    # (f) one technique alone: the denominator is its own density times its count
    if n_brdf == 0:
        assert float(((den - n_light * S64["p_light"]).abs() / S64["denom"].clamp_min(1e-300))[pos].max()) <= bden
    if n_light == 0:
        assert float(((den - n_brdf * S64["p_brdf"]).abs() / S64["denom"].clamp_min(1e-300))[pos].max()) <= bden
    # (b) visibility of the device's own directions against the fp64 brute force
    xs, ns, ngs, vs = per_sample(x, N), n_s, ng_s, v_s
    fs = per_sample(face[hit].long(), N)
    v64, margin, front = EO.visibility(xs, ns, ngs, vs, w, fs, sc["V"], sc["F"], sc["eps_d"])
    bad = (vis != v64) & ~flipped
    print("%s %s: visible %d of %d, visibility mismatches %d, of which margin >= %g: %d"
          % (name, counts, int(vis.sum()), vis.numel(), int(bad.sum()), EO.VIS_MARGIN, int((bad & (margin >= EO.VIS_MARGIN)).sum())))
    assert int((bad & (margin >= EO.VIS_MARGIN)).sum()) == 0
    assert float(bad.double().mean()) <= EO.VIS_SHARE
    assert 0 < int(vis.sum()) < vis.numel()
    # (c) every sample's term, and the sums, from the device's own directions, denominators and visibility in fp64
    kds, kss, rs = per_sample(kd, N), per_sample(ks, N), per_sample(rough, N)
    td64, ts64 = EO.sample_terms(e64, ns, vs, kds, kss, rs, w, den, vis, tables(), texel=S64["texel"])
    f32d, f32s = EO.roughplastic_point(ns, vs, w, kds, kss, rs, tables(), dtype=torch.float32)
    f64d, f64s = EO.roughplastic_point(ns, vs, w, kds, kss, rs, tables())
    step_clear = (EO.table_margin(ns, vs, w, rs) >= STEP_MARGIN) & (clear | is_light) & ~flipped
    lit = (vis & (den > 0) & step_clear)[:, None].expand(-1, 3)
    bf = measured(f32d + f32s, f64d + f64s, True, keep=lit) + 4e-7  # and the product with L and the division, one rounding each
    tot = td64 + ts64
    eterm = float(((con - tot).abs() / tot.abs().clamp_min(1e-300))[lit].max())
    print("%s %s: per-sample term rel error %.3e (measured bound %.3e); near a table step %d" % (name, counts, eterm, bf, int((~step_clear).sum())))
    assert float((~step_clear).double().mean()) <= 2 * STEP_SHARE
    assert eterm <= bf
    assert (con[~vis] == 0).all()
    col = out["color"][hit].double()
    s_abs = con.abs().reshape(P, N, 3).sum(1)
    esum = float(((col - con.reshape(P, N, 3).sum(1)).abs() / s_abs.clamp_min(1e-300))[s_abs > 0].max())
    print("%s %s: colour against the fp64 sum of the dumped terms: %.3e of the sum of absolute terms (bound 1e-5)" % (name, counts, esum))
    assert esum <= 1e-5
    assert (col[s_abs == 0] == 0).all()
    pixel_clear = step_clear.reshape(P, N).all(1)
    for key, terms in (("diffuse_color", td64), ("specular_color", ts64)):
        ref, mag = terms.reshape(P, N, 3).sum(1), terms.abs().reshape(P, N, 3).sum(1)
        e = float(((out[key][hit].double() - ref).abs() / mag.clamp_min(1e-300))[pixel_clear & (mag > 0).all(-1)].max())
        print("%s %s: %s against the oracle's fp64 sum: %.3e of the sum of absolute terms (bound %.3e)" % (name, counts, key, e, bf + 1e-5))
        assert e <= bf + 1e-5
    assert torch.equal(out["color"], out["diffuse_color"] + out["specular_color"])
    # (e) misses write zeros everywhere
    for key in ("color", "diffuse_color", "specular_color", "normal", "dump_dir", "dump_denom", "dump_vis", "dump_contrib"):
        assert (out[key][~hit] == 0).all(), key
    # (d) bitwise: a second run, without the dump pointers, and a sub-rectangle of the rays with their own pixel indices
    plain = run_env(asset, rays, env, n_light, n_brdf)
    again = run_env(asset, rays, env, n_light, n_brdf, dump=True)
    rect = (torch.arange(31)[:, None] * 33 + torch.arange(33)[None, :])[7:20, 5:23].reshape(-1).to(dev())
    part = run_env(asset, tuple(a[rect] for a in rays), env, n_light, n_brdf, pixel_idx=rect.int())
    for key in _lib.ASSET_OUT_FIELDS:
        a = out[key].view(torch.int32) if out[key].dtype == torch.float32 else out[key]
        for other, idx in ((plain, None), (again, None), (part, rect)):
            b = other[key].view(torch.int32) if other[key].dtype == torch.float32 else other[key]
            assert torch.equal(a if idx is None else a[idx], b), key
    for key in ("dump_dir", "dump_denom", "dump_vis", "dump_contrib"):
        assert torch.equal(out[key], again[key]), key
    other_seed = run_env(asset, rays, env, n_light, n_brdf, seed=6)
    assert not torch.equal(other_seed["color"], out["color"])


def test_back_facing_hits_are_black():
    """The floor seen from below: its face normal is never flipped towards the viewer, so n.w > 0 and (n_g.w)(n_g.v) > 0 exclude each
    other and every sample is invisible."""
    sc, asset, rays, env, e64, e32 = scene_on_device("floor", below=True)
    out = run_env(asset, rays, env, 16, 16, dump=True)
    hit = rays[3] >= 0
    assert int(hit.sum()) > 100
    assert float((out["normal"][hit] * -rays[1][hit]).sum(-1).max()) < 0
    assert (out["color"] == 0).all() and (out["dump_vis"] == 0).all()
    assert (out["dump_denom"][hit] > 0).any()


# ---- 5. unbiasedness against quadrature ---------------------------------------------------------------------------------------------
def test_estimate_against_quadrature():
    sc, asset, _, env, e64, _ = scene_on_device("floor")
    hot = EO.uv_to_dir(torch.tensor([(EO.HOT[1] + 0.5) / 32]), torch.tensor([(EO.HOT[0] + 0.5) / 16]))[0].double()
    shadow = torch.tensor([0.0, 0.5, 0.0], dtype=torch.float64) - hot * (0.5 / float(hot[1]))  # the occluder's centre along the hot texel
    targets = torch.tensor([[0.6, 0, 0.5], [0.7, 0, -0.6], [-0.8, 0, 0.7], [0.2, 0, 0.8], [-0.9, 0, -0.8], [0.85, 0, 0.1], [0.45, 0, 0.85]],
                           dtype=torch.float64)
    targets = torch.cat([targets, shadow[None]])
    cam = torch.tensor(sc["cam"], dtype=torch.float64)
    d = EO._unit(targets - cam[None]).float().to(dev())
    o = cam[None].expand(8, 3).float().contiguous().to(dev())
    t, face, bary = asset.bvh.raycast(o, d)
    assert (face >= 0).all() and (face < 2).all()  # the floor itself
    rays = (o, d, t, face, bary)
    first = run_env(asset, rays, env, 1, 0)
    x, nrm, v = first["points"].double(), first["normal"].double(), -d.double()
    kd, ks, rough = first["diffuse_albedo"].double(), first["specular_albedo"].double(), first["specular_roughness"].double()
    ng = EO.geometric_normals(sc["V"], sc["F"]).to(dev())[face.long()]
    quad, qerr = [], []
    for p in range(8):
        fine, coarse = (sum(EO.quadrature(e64, x[p], nrm[p], ng[p], v[p], kd[p], ks[p], rough[p], int(face[p]), sc["V"], sc["F"], sc["eps_d"],
                                          tables(), sub=sub)) for sub in (16, 8))
        quad.append(fine)
        qerr.append((fine - coarse).abs())  # the midpoint rule's own error at 16 x 16 cells per texel is below its change from 8 x 8
    quad, qerr = torch.stack(quad), torch.stack(qerr)
    assert float(quad[7].max()) < 0.05 * float(quad[:7].min())  # the eighth pixel lies in the occluder's shadow of the hot texel
    for n_light, n_brdf in ((2048, 2048), (4096, 0), (0, 4096)):
        N = n_light + n_brdf
        out = run_env(asset, rays, env, n_light, n_brdf, seed=9, dump=True)
        w = out["dump_dir"].reshape(-1, 3).double()
        den, vis = out["dump_denom"].reshape(-1).double(), out["dump_vis"].reshape(-1).bool()
        e = lambda a: per_sample(a, N)  # noqa: E731
        td, ts = EO.sample_terms(e64, e(nrm), e(v), e(kd), e(ks), e(rough), w, den, vis, tables())
        terms = (td + ts).reshape(8, N, 3)
        var = torch.zeros((8, 3), dtype=torch.float64, device=dev())
        if n_light > 1:
            var += n_light * terms[:, :n_light].var(1, unbiased=True)
        if n_brdf > 1:
            var += n_brdf * terms[:, n_light:].var(1, unbiased=True)
        se = var.sqrt()
        dev_ = (out["color"].double() - quad).abs()
        z = (dev_ - qerr).clamp_min(0) / se.clamp_min(1e-300)
        print("(%d, %d): estimate / quadrature per pixel (channel 0) %s; largest |estimate - quadrature| in standard errors %.2f; "
              "standard error / quadrature: median %.3e, shadowed pixel %.3e"
              % (n_light, n_brdf, [round(float(a), 4) for a in (out["color"][:, 0].double() / quad[:, 0])], float(z.max()),
                 float((se / quad).median()), float((se / quad)[7].max())))
        assert (se > 0).all()
        assert float(z.max()) <= 5.0


# ---- 6. render_asset_env end to end --------------------------------------------------------------------------------------------------
def diffuse_closed_form(cos_o, rough):
    """radiance of a diffuse-only white plane under a constant map of radiance 1, per cos_o: 2 pi int f_d cos sin dtheta"""
    k = 20000
    th = (torch.arange(k, dtype=torch.float64, device=dev()) + 0.5) / k * (math.pi / 2)
    l = torch.stack([torch.sin(th), torch.cos(th), torch.zeros_like(th)], -1)
    n = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=dev())[None].expand(k, 3)
    one = torch.ones((k, 3), dtype=torch.float64, device=dev())
    out = []
    for c in cos_o.tolist():
        v = torch.tensor([math.sqrt(max(1 - c * c, 0.0)), c, 0.0], dtype=torch.float64, device=dev())[None].expand(k, 3)
        fd, _ = EO.roughplastic_point(n, v, l, one, 0 * one, torch.full((k,), rough, dtype=torch.float64, device=dev()), tables())
        out.append(2 * math.pi * float((fd[:, 0] * torch.sin(th)).sum()) * (math.pi / 2 / k))
    return torch.tensor(out, dtype=torch.float64, device=dev())


def test_render_asset_env_end_to_end(tmp_path):
    import test_gpu_meshrender as MR
    from iron_amd.envmap import EnvMap
    from iron_amd.export_materials import write_obj
    from iron_amd.mesh_render import MeshAsset, render_asset_camera, render_asset_env, render_asset_uv, subpixel_uvs
    from iron_amd.raytracer import Camera
    v, f, uvs, fuv, xyz, mat, weight = MR.exported_asset()
    asset = MeshAsset(v, f, uvs, fuv, mat, weight=weight)
    cam = MR.fixture_camera(64, 64)
    hot = EO.hot_map().float().to(dev())
    env = EnvMap(hot)
    kw = dict(n_light=16, n_brdf=16, seed=3)
    res = render_asset_env(cam, asset, env, **kw)
    flash = render_asset_camera(cam, asset, 20.0)
    assert set(res.keys()) == set(flash.keys())
    for k in flash:
        assert res[k].shape == flash[k].shape and res[k].dtype == flash[k].dtype, k
    for k in ("normal", "points", "distance", "depth", "diffuse_albedo", "specular_roughness", "face_idx", "t", "convergent_mask", "tex_uv"):
        assert torch.equal(res[k], flash[k]), k  # the geometry and material maps are the flash render's
    m = res["convergent_mask"]
    assert 1000 < int(m.sum()) < 64 * 64 - 500
    assert (res["color"][~m] == 0).all() and float(res["color"][m].min()) >= 0 and float(res["color"][m].max()) > 0
    assert torch.isfinite(res["color"]).all()
    # background=True changes the miss pixels of `color` and nothing else
    bg = render_asset_env(cam, asset, env, background=True, **kw)
    for k in res:
        if k != "color":
            assert torch.equal(res[k], bg[k]), k
    assert torch.equal(bg["color"][m], res["color"][m])
    assert torch.equal(bg["color"][~m], env.lookup(res["ray_d"][~m]))
    assert float(bg["color"][~m].min()) > 0
    # samples_per_axis = 2: the mean of the four sub-frames, sample k with seed + k
    ss = render_asset_env(cam, asset, env, samples_per_axis=2, **kw)
    frames = [render_asset_uv(cam, asset, 0.0, uv, env=dict(envmap=env, n_light=16, n_brdf=16, seed=3 + k, shadow_eps=1e-4))
              for k, uv in enumerate(subpixel_uvs(cam, 2))]
    mean = (((frames[0]["color"] + frames[1]["color"]) + frames[2]["color"]) + frames[3]["color"]) / 4.0
    assert torch.equal(ss["color"].view(torch.int32), mean.view(torch.int32))
    assert not torch.equal(frames[0]["color"], render_asset_uv(cam, asset, 0.0, subpixel_uvs(cam, 2)[0],
                                                               env=dict(envmap=env, n_light=16, n_brdf=16, seed=4, shadow_eps=1e-4))["color"])
    # a diffuse-only white material under a constant map of radiance 1: the plane's closed form within 5 standard errors
    white = torch.zeros((8, 8, 7), device=dev())
    white[..., :3] = 1.0
    white[..., 6] = 0.3
    plain = MeshAsset(v, f, uvs, fuv, white)
    one = EnvMap(torch.ones((16, 32, 3), device=dev()))
    e64 = EO.EnvOracle(torch.ones((16, 32, 3), dtype=torch.float64, device=dev()))
    ray_o, ray_d, _ = cam.get_rays(cam.get_uv())
    o, d = ray_o.reshape(-1, 3).contiguous(), ray_d.reshape(-1, 3).contiguous()
    t, face, bary = plain.bvh.raycast(o, d)
    N = 128
    out = plain.shade_env(o, d, t, face, bary, one, tables(), n_light=64, n_brdf=64, seed=1, dump=True)
    hit = face >= 0
    nrm, vv = out["normal"][hit].double(), -d[hit].double()
    cos_o = EO._dot(nrm, vv)
    front = cos_o > 0.05
    P = int(hit.sum())
    e = lambda a: per_sample(a, N)  # noqa: E731
    td, _ = EO.sample_terms(e64, e(nrm), e(vv), e(out["diffuse_albedo"][hit]), e(out["specular_albedo"][hit]), e(out["specular_roughness"][hit]),
                            out["dump_dir"][hit].reshape(-1, 3), out["dump_denom"][hit].reshape(-1), out["dump_vis"][hit].reshape(-1), tables())
    terms = td[:, 0].reshape(P, N)
    se = (64 * terms[:, :64].var(1, unbiased=True) + 64 * terms[:, 64:].var(1, unbiased=True)).sqrt()
    grid = torch.linspace(0.0, 1.0, 401, dtype=torch.float64, device=dev())
    closed_grid = diffuse_closed_form(grid, 0.3)
    # the closed form is a step function of cos_o (the table): evaluate it at each pixel's own table entry through the nearest grid
    # points on both sides and take the closer value
    lo = (cos_o.clamp(0, 1) * 400).floor().long().clamp(0, 399)
    cands = torch.stack([closed_grid[lo], closed_grid[lo + 1]], -1)
    got = out["diffuse_color"][hit][:, 0].double()
    z = ((got[:, None] - cands).abs().min(-1).values / se.clamp_min(1e-300))[front]
    print("white sphere under a constant map: front-facing pixels %d, diffuse radiance %.4f .. %.4f, largest deviation from the plane's closed "
          "form %.2f standard errors (median standard error %.2e)" % (int(front.sum()), float(got[front].min()), float(got[front].max()),
                                                                      float(z.max()), float(se[front].median())))
    assert int(front.sum()) > 1000 and float(z.max()) <= 5.0
    assert (out["specular_color"] == 0).all()
    # the command line on the asset written to disk: bitwise the API
    adir = os.path.join(tmp_path, "asset")
    os.makedirs(adir)
    write_obj(os.path.join(adir, "model.obj"), v.cpu().numpy(), uvs.cpu().numpy(), f.cpu().numpy(), fuv.cpu().numpy())
    mm = mat.cpu().numpy()
    np.save(os.path.join(adir, "diffuse_albedo.npy"), mm[..., :3])
    np.save(os.path.join(adir, "specular_albedo.npy"), mm[..., 3:6])
    np.save(os.path.join(adir, "roughness.npy"), mm[..., 6])
    np.save(os.path.join(adir, "weight.npy"), weight.cpu().numpy())
    np.save(os.path.join(adir, "probe.npy"), hot.cpu().numpy())
    cams = {"7.png": {"K": cam.K.cpu().reshape(-1).tolist(), "W2C": cam.W2C.cpu().reshape(-1).tolist(), "img_size": [64, 64]}}
    with open(os.path.join(adir, "cam_dict_norm.json"), "w") as fp:
        json.dump(cams, fp)
    rdir = os.path.join(tmp_path, "render")
    r = subprocess.run([sys.executable, "-m", "iron_amd.render_asset", "--mesh", os.path.join(adir, "model.obj"), "--textures", adir,
                        "--cam_dict", os.path.join(adir, "cam_dict_norm.json"), "--out", rdir, "--envmap", os.path.join(adir, "probe.npy"),
                        "--n-light", "16", "--n-brdf", "16", "--seed", "3", "--background"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if os.path.exists(os.path.join(rdir, "image", "7.npy")):
        img = np.load(os.path.join(rdir, "image", "7.npy"))
    else:
        import imageio
        img = np.asarray(imageio.imread(os.path.join(rdir, "image", "7.exr")), dtype=np.float32)
    cam_json = Camera(64, 64, torch.tensor(cams["7.png"]["K"], dtype=torch.float32).reshape(4, 4).to(dev()),
                      torch.tensor(cams["7.png"]["W2C"], dtype=torch.float32).reshape(4, 4).to(dev()))
    api = render_asset_env(cam_json, MeshAsset.load(os.path.join(adir, "model.obj"), adir), EnvMap(np.load(os.path.join(adir, "probe.npy"))),
                           background=True, **kw)["color"].cpu().numpy()
    assert img.dtype == np.float32 and np.array_equal(img.view(np.int32), api.view(np.int32))
    from PIL import Image
    png = np.asarray(Image.open(os.path.join(rdir, "image", "7.png")))
    assert np.array_equal(png[..., :3], (np.clip(np.power(api, 1 / 2.2), 0, 1) * 255).astype(np.uint8))
    assert not os.path.exists(os.path.join(rdir, "light.txt"))
