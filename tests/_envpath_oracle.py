"""fp64 restatement of the path integrator for interreflections (csrc/envlight.hip: k_shade_env_indirect), in torch
and device-agnostic: CPU for the CPU tests, the GPU for the larger checks.  Test infrastructure: never uses the HIP library.

Everything the direct integrator already has (the map and its sampler, the BRDF and its sampler, the random numbers, the
brute-force casts, the direct quadrature) is _envlight_oracle's and _meshrender_oracle's; this module adds the surface record of a
ray that is not a camera ray, the walk along a path, the scenes `corner` and `sphere`, and a nested quadrature of the one-bounce
integral that shares nothing with the sampler.  `dtype=torch.float32` runs the same formulas in fp32: the measure of what fp32 can
give, from which the GPU tests take their bounds.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import _envlight_oracle as EO
import _meshrender_oracle as O

EDGE_MARGIN = 1e-4  # a bounce ray whose fp64 hit lies closer than this to a face edge (barycentric) may reach either face in fp32
EDGE_SHARE = 1e-3


# ---- scenes ----
def scene(name):
    """EO.scene's dictionary for `floor` and `cube`, and for
    corner_face / corner_vertex: the floor y = 0 on [-1, 1]^2 with the wall x = -1, y in [0, 2], both wound to face into the corner
        and sharing the two crease vertices; face normals, or area-weighted vertex normals that are smooth across the crease (the
        shading normal then leaves the geometric one by up to 45 degrees);
    sphere: O.uv_sphere(16, 32), convex, smooth normals."""
    if name in ("floor", "cube"):
        return EO.scene(name)
    g = torch.Generator().manual_seed(35)
    if name == "sphere":
        V, F = O.uv_sphere(16, 32, 0.6)
        r = V.norm(dim=1, keepdim=True)
        uvs = torch.stack([torch.atan2(V[:, 1], V[:, 0]) / (2 * math.pi) + 0.5, torch.acos((V[:, 2:3] / r)[:, 0].clamp(-1, 1)) / math.pi], -1)
        cam, target, normals = (0.4, 0.3, 2.2), (0.0, 0.0, 0.0), "vertex"
    else:
        V = torch.tensor([[-1.0, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1], [-1, 2, -1], [-1, 2, 1]], dtype=torch.float64)
        F = torch.tensor([[0, 2, 1], [0, 3, 2], [0, 4, 5], [0, 5, 3]])
        uvs = torch.stack([((V[:, 0] + 1) - V[:, 1] + 2) / 4, (V[:, 2] + 1) / 2], -1)  # the wall unfolded beside the floor
        cam, target, normals = (1.7, 1.9, 2.1), (-0.35, 0.45, 0.0), name.split("_")[1]
    mat = torch.rand((4, 4, 7), generator=g, dtype=torch.float64) * 0.6 + 0.2
    mat[..., 6] = 0.2 + 0.4 * torch.rand((4, 4), generator=g, dtype=torch.float64)
    V = EO.f32(V)
    return {"V": V, "F": F, "uvs": EO.f32(uvs), "face_uvs": F, "material": EO.f32(mat), "normals": normals, "cam": cam, "target": target,
            "eps_d": 1e-4 * float((V.max(0).values - V.min(0).values).norm())}


def probe_rays():
    """The eight probe pixels of `corner`: camera rays to four points of the floor and four of the wall, 0.2 .. 0.5 from the crease."""
    sc = scene("corner_face")
    targets = torch.tensor([[-0.8, 0, 0.3], [-0.7, 0, -0.4], [-0.6, 0, 0.6], [-0.5, 0, -0.1],
                            [-1, 0.2, -0.3], [-1, 0.3, 0.5], [-1, 0.4, 0.1], [-1, 0.5, -0.2]], dtype=torch.float64)
    cam = torch.tensor(sc["cam"], dtype=torch.float64)
    d = EO._unit(targets - cam[None])
    return EO.f32(cam[None].expand(8, 3).contiguous()), EO.f32(d)


# ---- the surface record of any ray that is known to meet a face ----
@functools.lru_cache(maxsize=None)
def _vertex_normals(name):
    sc = scene(name)
    return O.vertex_normals(sc["V"], sc["F"])[0]


def vertex_state(sc, name, org, d, face, dtype=torch.float64):
    """The path vertex where the ray (org, d) [m, 3] meets face [m] (>= 0) of the scene `name`: Moeller-Trumbore on that face alone
    for t and the barycentric weights, then the asset's surface record (point, interpolated or face normal, bilinear material) ->
    {x, n, ng, v = -d, kd, ks, rough, alpha, face, t}.  Geometry and weights in `dtype`; the texture fetch itself is O.texture_fetch."""
    dev = org.device
    V, F = sc["V"].to(dev).to(dtype), sc["F"].long().to(dev)
    o, dd = org.to(dtype), d.to(dtype)
    fv = F[face]
    a, e1, e2 = V[fv[:, 0]], V[fv[:, 1]] - V[fv[:, 0]], V[fv[:, 2]] - V[fv[:, 0]]
    p = torch.cross(dd, e2, dim=-1)
    det = EO._dot(e1, p)
    s = o - a
    b1 = EO._dot(s, p) / det
    q = torch.cross(s, e1, dim=-1)
    b2 = EO._dot(dd, q) / det
    t = EO._dot(e2, q) / det
    b1, b2 = b1.clamp(0, 1), b2.clamp(0, 1)
    b0 = (1 - b1) - b2
    ng = EO._unit(torch.cross(e1, e2, dim=-1))
    if sc["normals"] == "vertex":
        VN = _vertex_normals(name).to(dev).to(dtype)
        n = EO._unit(b0[:, None] * VN[fv[:, 0]] + b1[:, None] * VN[fv[:, 1]] + b2[:, None] * VN[fv[:, 2]])
    else:
        n = ng
    UV = sc["uvs"].to(dev).to(dtype)
    ft = sc["face_uvs"].long().to(dev)[face]
    uv = b0[:, None] * UV[ft[:, 0]] + b1[:, None] * UV[ft[:, 1]] + b2[:, None] * UV[ft[:, 2]]
    mat = O.texture_fetch(sc["material"].to(dev), uv.double())[0].to(dtype)
    return {"x": o + t[:, None] * dd, "n": n, "ng": ng, "v": -dd, "kd": mat[:, :3], "ks": mat[:, 3:6], "rough": mat[:, 6],
            "alpha": mat[:, 6].clamp(min=1e-4), "face": face, "t": t}


def take(st, keep):
    return {k: v[keep] for k, v in st.items()}


def counts(st, w, ok):
    """may the sample direction w count at the vertex: a sample, above the shading horizon, on the viewer's side of the face"""
    ngw = EO._dot(st["ng"], w)
    return ok & (EO._dot(st["n"], w) > 0) & (ngw * EO._dot(st["ng"], st["v"]) > 0) & torch.isfinite(w).all(-1)


def vertex_samples(env, st, pixel, path, j, seed, dtype=torch.float64):
    """The two samples of vertex j of path `path` [m] of pixel `pixel` [m] (env in the same dtype): the BRDF sample wb (ok_b: a
    sample at all) with p_light and p_brdf at it, the environment sample wl with its texel, both densities and the distance of its
    random numbers to the nearest CDF boundary (fp32 ulps)."""
    dev = st["x"].device
    pix, pth = (np.asarray(torch.as_tensor(a).cpu()).astype(np.int64) for a in (pixel, path))
    u = [torch.from_numpy(EO.env_rand(seed, pix, pth, 8 * (j + 1) + c)).to(dev).to(dtype) for c in range(5)]
    n, v, alpha = st["n"].to(dtype), st["v"].to(dtype), st["alpha"].to(dtype)
    wb, okb = EO.brdf_sample(n, v, alpha, u[0], u[1], u[2])
    texel, wl, pl_l = env.sample(torch.stack([u[3], u[4]], -1))
    zero = torch.zeros_like(alpha)
    return {"wb": wb, "ok_b": okb, "pl_b": env.pdf(wb).to(dtype), "pb_b": torch.where(okb, EO.brdf_pdf(n, v, wb, alpha), zero),
            "wl": wl.to(dtype), "texel": texel, "pl_l": pl_l.to(dtype), "pb_l": EO.brdf_pdf(n, v, wl.to(dtype), alpha), "gap": env.boundary_gap}


def plastic(st, w, tables, dtype=torch.float64):
    return EO.roughplastic_point(st["n"], st["v"], w, st["kd"], st["ks"], st["rough"], tables, dtype=dtype)


def bounce_cast(sc, st, w):
    """the bounce ray of a vertex along w in fp64: origin, t, face (-1: it escapes), the brute-force edge margin of EO.any_hit (over
    every face whose plane the ray crosses), and whether the face met is seen from its front"""
    org = EO.shadow_origin(st["x"].double(), st["ng"].double(), w.double(), sc["eps_d"])
    t, f, _, _ = O.closest_hit(org, w.double(), sc["V"], sc["F"])  # the vertex's own face lies behind the origin: nothing to skip
    _, margin = EO.any_hit(org, w.double(), sc["V"], sc["F"], skip=st["face"])
    ng2 = EO.geometric_normals(sc["V"], sc["F"]).to(org.device)[f.clamp(min=0)]
    return org, t, f, margin, (f >= 0) & (EO._dot(ng2, -w.double()) > 0)


# ---- the estimator ----
def estimate(env, sc, name, tables, ray_o, ray_d, pixel, n_paths, max_depth, seed):
    """fp64 path estimator for the camera rays (ray_o, ray_d) [n, 3] with pixel indices `pixel` [n], vectorised over rays and paths
    -> {hit [n], indirect_diffuse, indirect_specular [n, 3], values [n, n_paths, 3] (a path's lobe weights times what it gathered),
    bounce_margin, shadow_margin (one entry per ray cast), reached (the face of every bounce ray)}."""
    dev = ray_o.device
    n, P = ray_o.shape[0], int(n_paths)
    t0, f0, _, _ = O.closest_hit(ray_o.double(), ray_d.double(), sc["V"], sc["F"])
    hit = f0 >= 0
    rows = torch.nonzero(hit)[:, 0].repeat_interleave(P)         # the ray of every (ray, path) row
    path = torch.arange(P, device=dev).repeat(int(hit.sum()))
    pix = torch.as_tensor(pixel).to(dev).long()[rows]
    m = rows.shape[0]
    st = vertex_state(sc, name, ray_o[rows], ray_d[rows], f0[rows])
    live = torch.arange(m, device=dev)                           # the rows whose path is still under way
    T = torch.ones((m, 3), dtype=torch.float64, device=dev)
    C = torch.zeros_like(T)
    bd, bs = torch.zeros_like(T), torch.zeros_like(T)
    bm, sm, reached = [], [], []
    for j in range(max_depth):
        if live.numel() == 0:
            break
        S = vertex_samples(env, st, pix[live], path[live], j, seed)
        if j >= 1:
            vis, margin, front = EO.visibility(st["x"], st["n"], st["ng"], st["v"], S["wl"], st["face"], sc["V"], sc["F"], sc["eps_d"])
            sm.append(margin[front])
            fd, fs = plastic(st, S["wl"], tables)
            dl = S["pl_l"] + S["pb_l"]
            L = env.image[S["texel"][:, 0], S["texel"][:, 1]]
            good = (vis & (dl > 0))[:, None]
            C[live] += torch.where(good, T[live] * L * (fd + fs) / torch.where(dl > 0, dl, torch.ones_like(dl))[:, None], torch.zeros_like(L))
        go = counts(st, S["wb"], S["ok_b"])
        live, st, S = live[go], take(st, go), take(S, go)
        org, t, f, margin, front = bounce_cast(sc, st, S["wb"])
        bm.append(margin)
        reached.append(f)
        fd, fs = plastic(st, S["wb"], tables)
        esc = f < 0
        if j >= 1:
            db = (S["pl_b"] + S["pb_b"])[esc]
            C[live[esc]] += torch.where((db > 0)[:, None], T[live[esc]] * env.lookup(S["wb"][esc]) * (fd + fs)[esc]
                                        / torch.where(db > 0, db, torch.ones_like(db))[:, None], torch.zeros_like(fd[esc]))
        on = front & (S["pb_b"] > 0)
        if j == 0:
            bd[live[on]], bs[live[on]] = (fd / S["pb_b"][:, None])[on], (fs / S["pb_b"][:, None])[on]
        else:
            T[live[on]] = T[live[on]] * ((fd + fs) / S["pb_b"][:, None])[on]
        live = live[on]
        st = vertex_state(sc, name, org[on], S["wb"][on], f[on])
    P_hit = int(hit.sum())
    out_d = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    out_s = torch.zeros_like(out_d)
    out_d[hit], out_s[hit] = (bd * C).reshape(P_hit, P, 3).mean(1), (bs * C).reshape(P_hit, P, 3).mean(1)
    values = torch.zeros((n, P, 3), dtype=torch.float64, device=dev)
    values[hit] = ((bd + bs) * C).reshape(P_hit, P, 3)
    cat = lambda a: torch.cat(a) if a else torch.zeros(0, device=dev)  # noqa: E731
    return {"hit": hit, "indirect_diffuse": out_d, "indirect_specular": out_s, "values": values, "bounce_margin": cat(bm),
            "shadow_margin": cat(sm), "reached": cat(reached)}


# ---- nested quadrature of the one-bounce integral (max_depth = 2), independent of the sampler ----
def inner_direct(env, sc, st, tables, sub, chunk=1 << 20):
    """The direct radiance (diffuse + specular) [m, 3] that leaves the vertices `st` along their v: EO.quadrature's rule (every texel
    split into sub x sub cells in (u, v), midpoints, solid angle 2 pi^2 sin(theta) du dv, brute-force visibility), for many vertices
    at once; only directions above a vertex's shading horizon are cast."""
    dev = env.dev
    He, We = env.He, env.We
    vv = (torch.arange(He * sub, dtype=torch.float64, device=dev) + 0.5) / (He * sub)
    uu = (torch.arange(We * sub, dtype=torch.float64, device=dev) + 0.5) / (We * sub)
    U, Vv = torch.meshgrid(uu, vv, indexing="xy")
    w = EO.uv_to_dir(U.reshape(-1), Vv.reshape(-1)) @ env.R.T
    dom = (2 * math.pi ** 2 / (He * We * sub * sub)) * torch.sin(math.pi * Vv.reshape(-1))
    L = env.image[(torch.arange(He * sub, device=dev) // sub)[:, None], (torch.arange(We * sub, device=dev) // sub)[None, :]].reshape(-1, 3)
    m, M = st["x"].shape[0], w.shape[0]
    out = torch.zeros((m, 3), dtype=torch.float64, device=dev)
    step = max(1, chunk // M)
    for i0 in range(0, m, step):
        part = {k: v[i0:i0 + step] for k, v in st.items()}
        k = part["x"].shape[0]
        up = torch.nonzero(part["n"] @ w.T > 0)  # (vertex, direction) pairs above the horizon
        vi, wi = up[:, 0], up[:, 1]
        rows = take(part, vi)
        vis, _, _ = EO.visibility(rows["x"], rows["n"], rows["ng"], rows["v"], w[wi], rows["face"], sc["V"], sc["F"], sc["eps_d"])
        fd, fs = plastic(rows, w[wi], tables)
        acc = torch.zeros((k, 3), dtype=torch.float64, device=dev)
        acc.index_add_(0, vi, (dom[wi] * vis.double())[:, None] * L[wi] * (fd + fs))
        out[i0:i0 + k] = acc
    return out


def nested_quadrature(env, sc, name, tables, st0, cells, sub):
    """(indirect_diffuse, indirect_specular) [m, 3] of the primary vertices st0 at max_depth = 2: a midpoint grid over the part of
    each primary's hemisphere that sees a face, in the coordinates of that face.  Face (A, B, C) is the image of the unit square
    under (s, t) -> A + s ((1 - t) (B - A) + t (C - A)) (area element s |(B - A) x (C - A)|), cells x cells midpoints each; a
    point x' is the direction w = (x' - x) / r with solid angle n_g'.(-w) / r^2 times its area.  Per cell: the primary's two lobes
    at w times the direct radiance (inner_direct) that x' sends back, nothing where w does not count at the primary, where the face
    is met from behind or where the bounce ray's closest hit is another face.  (A grid in the direction itself cuts its cells along
    the silhouette of every face and converges like 1 / cells: 1.3 % between 64 and 128 cells here; this one has no cut cells.)"""
    dev = st0["x"].device
    A = int(cells)
    mid = (torch.arange(A, dtype=torch.float64, device=dev) + 0.5) / A
    s, t = mid[:, None].expand(A, A).reshape(-1), mid[None, :].expand(A, A).reshape(-1)
    V, F = sc["V"].to(dev), sc["F"].long().to(dev)
    NG = EO.geometric_normals(sc["V"], sc["F"]).to(dev)
    out_d, out_s = [], []
    for p in range(st0["x"].shape[0]):
        acc_d = torch.zeros(3, dtype=torch.float64, device=dev)
        acc_s = torch.zeros_like(acc_d)
        for g in range(F.shape[0]):
            a, e1, e2 = V[F[g, 0]], V[F[g, 1]] - V[F[g, 0]], V[F[g, 2]] - V[F[g, 0]]
            pts = a[None] + s[:, None] * ((1 - t)[:, None] * e1[None] + t[:, None] * e2[None])
            area = s * torch.cross(e1, e2, dim=0).norm() / (A * A)
            one = {k: v[p:p + 1].expand(A * A, *v.shape[1:]) for k, v in st0.items()}
            to = pts - one["x"]
            r2 = EO._dot(to, to)
            w = to / r2.sqrt()[:, None]
            cos1 = -EO._dot(NG[g][None], w)
            go = counts(one, w, torch.ones_like(s, dtype=torch.bool)) & (cos1 > 0)
            if not go.any():
                continue
            one, w, dom = take(one, go), w[go], (area * cos1 / r2)[go]
            org, _, f, _, _ = bounce_cast(sc, one, w)
            seen = f == g
            one, w, dom, org = take(one, seen), w[seen], dom[seen], org[seen]
            fd, fs = plastic(one, w, tables)
            back = inner_direct(env, sc, vertex_state(sc, name, org, w, torch.full((w.shape[0],), g, device=dev)), tables, sub)
            acc_d += (dom[:, None] * fd * back).sum(0)
            acc_s += (dom[:, None] * fs * back).sum(0)
        out_d.append(acc_d)
        out_s.append(acc_s)
    return torch.stack(out_d), torch.stack(out_s)


@functools.lru_cache(maxsize=None)
def probe_quadrature(device, cells, sub):
    """Once per session and device: the eight probe pixels of corner_face under EO.hot_map() -> {st0, direct [8, 3], indirect_diffuse,
    indirect_specular [8, 3] at (cells, sub), change [8, 3]: |indirect - indirect at (cells / 2, sub)| + |indirect at (cells / 2, sub)
    - indirect at (cells / 2, sub / 2)|, the refinement change of the outer and of the inner grid}."""
    from iron_amd.renderer_ggx import load_mts_tables
    dev = torch.device(device)
    tables = tuple(t.to(dev) for t in load_mts_tables())
    sc = scene("corner_face")
    env = EO.EnvOracle(EO.hot_map().to(dev))
    o, d = (a.to(dev) for a in probe_rays())
    _, f, _, _ = O.closest_hit(o, d, sc["V"], sc["F"])
    st0 = vertex_state(sc, "corner_face", o, d, f)
    fine = nested_quadrature(env, sc, "corner_face", tables, st0, cells, sub)
    outer = nested_quadrature(env, sc, "corner_face", tables, st0, cells // 2, sub)
    inner = nested_quadrature(env, sc, "corner_face", tables, st0, cells // 2, sub // 2)
    change = (fine[0] + fine[1] - outer[0] - outer[1]).abs() + (outer[0] + outer[1] - inner[0] - inner[1]).abs()
    direct = torch.stack([sum(EO.quadrature(env, st0["x"][p], st0["n"][p], st0["ng"][p], st0["v"][p], st0["kd"][p], st0["ks"][p],
                                            st0["rough"][p], int(f[p]), sc["V"], sc["F"], sc["eps_d"], tables, sub=2 * sub)) for p in range(8)])
    return {"st0": st0, "face": f, "direct": direct, "indirect_diffuse": fine[0], "indirect_specular": fine[1], "change": change}


# ---- what the CPU checks of the preconditions and the GPU tests share ----
SETTINGS = ((5, 2), (16, 3), (48, 4))  # (n_paths, max_depth) of the GPU test through the dumps
SEED = 5
DUMP_SCENES = ("corner_face", "corner_vertex", "floor")
ZERO_SCENES = ("cube", "sphere", "floor")  # no interreflection: convex, or the only other face is met from behind
