"""The oracle's side of the checks of the neural relight's interreflections (iron_amd/neural_relight.py with max_depth > 1,
csrc/envlight.hip k_npath_*), in torch and device-agnostic.  Test infrastructure: never uses the HIP library.

The path rules are tests/_envpath_oracle.py's with the neural scene's in the mesh's place: the shading normal stands where the
geometric normal stood, both rays of a vertex leave x + eps n, and the closest hit and the surface record are the reference
tracer's and the reference shading's (oracle/iron_ref.py).  What is shared:
    vertex(...)          a path vertex from a surface record (the device's dumped one, in the GPU tests) in fp64 or fp32;
    origin(...)          the origin of both rays of a vertex;
    PO.vertex_samples, PO.counts, PO.plastic on such a vertex: the two samples, the counting rule and the BRDF;
    Field                a field's fp64 / fp32 SDF, surface record and tracer;
    estimate(...)        the fp64 path estimator on the fixture view of a field (tests/test_neural_path_oracle.py);
    crease(...)          the scene of the two-integrator test: two overlapping boxes as a mesh and as a distance function.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import iron_ref as R
from iron_amd import scenes

import _envlight_oracle as EO
import _envpath_oracle as PO
import _hard_fields as H
import _nets as N
import _neuralenv_oracle as NO

SETTINGS = PO.SETTINGS   # (n_paths, max_depth) of the GPU test through the dumps: §17's
SEED = PO.SEED
EPS = NO.EPS             # the relight's default shadow_eps
RES = NO.RES             # the fixture view of the oracle estimator
SIDE = 1e-6              # a cosine smaller than this may have either sign in fp32


# ---- a vertex from a surface record ----
def vertex(x, n, d, kd, ks, rough, dtype=torch.float64):
    """The path vertex at point x with shading normal n, reached along d (v = -d), material (kd, ks, rough) -> the dictionary
    PO.vertex_samples, PO.counts and PO.plastic take.  There is no geometric normal: n takes its place."""
    x, n, d, kd, ks, rough = (a.to(dtype) for a in (x, n, d, kd, ks, rough))
    return {"x": x, "n": n, "ng": n, "v": -d, "kd": kd, "ks": ks, "rough": rough, "alpha": rough.clamp(min=1e-4),
            "face": torch.zeros(x.shape[0], dtype=torch.long, device=x.device)}


def origin(st, eps, dtype=torch.float64):
    """x + eps n, each product and sum rounded on its own in `dtype`"""
    return st["x"].to(dtype) + torch.as_tensor(eps, dtype=dtype, device=st["x"].device) * st["n"].to(dtype)


# ---- a field: the SDF, the surface record and the tracer of the oracle, in two precisions ----
class Field:
    def __init__(self, name):
        self.name = name
        self.net = NO.build(name)
        self.f64, self.f32 = H.oracle_fns(self.net)
        self.spec = N.sdf_spec(N.sdf_kw("prod"))
        self.sd64 = N.sd64(self.net)
        mats = {k: v for k, v in scenes.build_networks("S0").items() if k != "sdf_network"}
        self.mat64 = {k: ({a: b.detach().double() for a, b in mats[k].state_dict().items()}, R.GGX_SPECS[k]) for k in R.GGX_SPECS}

    @torch.no_grad()
    def trace(self, o, d, precision="fp64"):
        """the reference tracer on the fp32 rays (o, d), cut to the unit sphere -> convergent_mask, points, distance"""
        dtype = torch.float64 if precision == "fp64" else torch.float32
        work, near, far = R.intersect_sphere(o.float(), d.float(), 1.0)
        r = R.raytracer_forward(self.f64 if precision == "fp64" else self.f32, o.to(dtype), d.to(dtype), near.to(dtype), far.to(dtype),
                                work, R.TracerParams(n_steps=H.N_STEPS))
        return r["convergent_mask"], r["points"], r["distance"]

    @torch.no_grad()
    def surface(self, x):
        """the reference's surface record at x [m, 3] in fp64: normalised gradient and the three material heads"""
        x = x.double()
        _, feat, grad = R.sdf_get_all(self.sd64, self.spec, x)
        n = grad / (grad.norm(dim=-1, keepdim=True) + 1e-10)
        m = R.get_materials(self.mat64, x, n, feat)
        return n, m["diffuse_albedo"], m["specular_albedo"], m["specular_roughness"].reshape(-1)


@functools.lru_cache(maxsize=None)
def field(name):
    return Field(name)


@functools.lru_cache(maxsize=None)
def cpu_tables():
    from iron_amd.renderer_ggx import load_mts_tables
    return tuple(t.double() for t in load_mts_tables())


# ---- the estimator ----
@functools.lru_cache(maxsize=None)
@torch.no_grad()
def estimate(name, n_paths, max_depth, seed=SEED, res=RES, eps=EPS):
    """fp64 path estimator on the res x res fixture view of field `name` under EO.hot_map(): PO.estimate with the neural scene's
    rules -> {hits, vertices [max_depth + 1] (paths that reach vertex j; vertices[0] = hits * n_paths), bounce_rays, bounce_hits,
    front (bounce hits seen from the front), shadow_rays, occluded, indirect_diffuse, indirect_specular [hits, 3], values
    [hits, n_paths, 3], fp32_flips (bounce rays whose hit / miss differs between the oracle's fp32 and fp64 tracer)}."""
    F = field(name)
    env = EO.EnvOracle(EO.hot_map())
    tables = cpu_tables()
    ro, rd, near, far, work = H.fixture_rays(res, NO.yaw_of(name))
    r = R.raytracer_forward(F.f64, ro.double(), rd.double(), near.double(), far.double(), work, R.TracerParams(n_steps=H.N_STEPS))
    hit = r["convergent_mask"]
    Hn, P = int(hit.sum()), int(n_paths)
    pix = torch.nonzero(hit)[:, 0].repeat_interleave(P)
    path = torch.arange(P).repeat(Hn)
    x0 = r["points"][hit]
    n0, kd0, ks0, r0 = F.surface(x0)
    rep = lambda a: a.repeat_interleave(P, 0)  # noqa: E731
    st = vertex(rep(x0), rep(n0), rep(rd[hit].double()), rep(kd0), rep(ks0), rep(r0))
    m = Hn * P
    live = torch.arange(m)
    T = torch.ones((m, 3), dtype=torch.float64)
    C, bd, bs = torch.zeros_like(T), torch.zeros_like(T), torch.zeros_like(T)
    out = {"hits": Hn, "vertices": [m], "bounce_rays": 0, "bounce_hits": 0, "front": 0, "shadow_rays": 0, "occluded": 0, "fp32_flips": 0}
    for j in range(max_depth):
        if live.numel() == 0:
            out["vertices"].append(0)
            continue
        S = PO.vertex_samples(env, st, pix[live], path[live], j, seed)
        org = EO.f32(origin(st, eps))   # the rays are fp32 numbers on both sides
        if j >= 1:
            dl = S["pl_l"] + S["pb_l"]
            cast = PO.counts(st, S["wl"], torch.ones_like(dl, dtype=torch.bool)) & (dl > 0)
            occ, _, _ = F.trace(org[cast], EO.f32(S["wl"][cast]))
            vis = cast.clone()
            vis[cast] = ~occ
            out["shadow_rays"] += int(cast.sum())
            out["occluded"] += int(occ.sum())
            fd, fs = PO.plastic(st, S["wl"], tables)
            L = env.image[S["texel"][:, 0], S["texel"][:, 1]]
            C[live] += torch.where(vis[:, None], T[live] * L * (fd + fs) / torch.where(dl > 0, dl, torch.ones_like(dl))[:, None], torch.zeros_like(L))
        go = PO.counts(st, S["wb"], S["ok_b"])
        live, st, S, org = live[go], PO.take(st, go), PO.take(S, go), org[go]
        wb32 = EO.f32(S["wb"])
        got, pts, _ = F.trace(org, wb32)
        got32, _, _ = F.trace(org, wb32, "fp32")
        out["bounce_rays"] += int(got.numel())
        out["bounce_hits"] += int(got.sum())
        out["fp32_flips"] += int((got != got32).sum())
        fd, fs = PO.plastic(st, S["wb"], tables)
        esc = ~got
        if j >= 1:
            db = (S["pl_b"] + S["pb_b"])[esc]
            C[live[esc]] += torch.where((db > 0)[:, None], T[live[esc]] * env.lookup(S["wb"][esc]) * (fd + fs)[esc]
                                        / torch.where(db > 0, db, torch.ones_like(db))[:, None], torch.zeros_like(fd[esc]))
        n2, kd2, ks2, r2 = F.surface(pts[got])
        front = torch.zeros_like(got)
        front[got] = EO._dot(n2, -S["wb"][got]) > 0
        out["front"] += int(front.sum())
        on = front & (S["pb_b"] > 0)
        if j == 0:
            bd[live[on]], bs[live[on]] = (fd / S["pb_b"][:, None])[on], (fs / S["pb_b"][:, None])[on]
        else:
            T[live[on]] = T[live[on]] * ((fd + fs) / S["pb_b"][:, None])[on]
        keep = on[got]
        st = vertex(pts[got][keep], n2[keep], S["wb"][on], kd2[keep], ks2[keep], r2[keep])
        live = live[on]
        out["vertices"].append(int(live.numel()))
    out["indirect_diffuse"], out["indirect_specular"] = (bd * C).reshape(Hn, P, 3).mean(1), (bs * C).reshape(Hn, P, 3).mean(1)
    out["values"] = ((bd + bs) * C).reshape(Hn, P, 3)
    return out


# ---- one estimator, two scenes: a crease of two boxes ----
FLOOR = ((-0.6, -0.3, -0.5), (0.5, -0.1, 0.5))   # a slab, top face y = -0.1
WALL = ((-0.6, -0.3, -0.5), (-0.4, 0.5, 0.5))    # a slab, inner face x = -0.4; the crease is the line x = -0.4, y = -0.1
MATERIAL = (0.55, 0.45, 0.35, 0.3, 0.3, 0.3, 0.35)   # kd, ks, roughness: constant


def _box_mesh(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    V = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    # vertex index = 4 i + 2 j + k; outward faces, counter-clockwise seen from outside
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    F = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    return V, F


def crease():
    """The union of the two boxes as EO.scene's dictionary (24 faces: the two closed boxes, overlapping -- faces inside the solid are
    never seen from outside it; a 1 x 1 texture; face normals) with the slab length, the crease and the probe targets."""
    Va, Fa = _box_mesh(*FLOOR)
    Vb, Fb = _box_mesh(*WALL)
    V = torch.from_numpy(np.concatenate([Va, Vb]))
    F = torch.from_numpy(np.concatenate([Fa, Fb + 8]))
    # outward?  the normal of a face must point away from its box's centre
    for k in range(F.shape[0]):
        c = V[:8].mean(0) if k < 12 else V[8:].mean(0)
        a, b, d = V[F[k, 0]], V[F[k, 1]], V[F[k, 2]]
        if torch.dot(torch.cross(b - a, d - a, dim=0), a - c) < 0:
            F[k] = F[k][[0, 2, 1]]
    uvs = torch.full((V.shape[0], 2), 0.5, dtype=torch.float64)
    mat = torch.tensor(MATERIAL, dtype=torch.float64).reshape(1, 1, 7)
    length = 0.9   # of either slab, away from the crease
    s = torch.tensor([0.2, 0.3, 0.4, 0.5], dtype=torch.float64) * length
    z = torch.tensor([0.15, -0.2, 0.3, -0.05], dtype=torch.float64)
    on_floor = torch.stack([-0.4 + s, torch.full_like(s, -0.1), z], -1)
    on_wall = torch.stack([torch.full_like(s, -0.4), -0.1 + s * (0.6 / 0.9), z.flip(0)], -1)   # the wall is 0.6 high above the floor
    cam = torch.tensor([0.75, 0.8, 0.55], dtype=torch.float64)   # outside the unit sphere: the primary rays are the mesh's ray cast
    targets = torch.cat([on_floor, on_wall])
    d = EO._unit(targets - cam[None])
    V = EO.f32(V)
    return {"V": V, "F": F, "uvs": EO.f32(uvs), "face_uvs": F.clone(), "material": EO.f32(mat), "normals": "face",
            "ray_o": EO.f32(cam[None].expand(8, 3).contiguous()), "ray_d": EO.f32(d), "targets": targets,
            "diag": float((V.max(0).values - V.min(0).values).norm())}


def _box_sdf(x, lo, hi):
    c = (torch.as_tensor(lo, dtype=x.dtype, device=x.device) + torch.as_tensor(hi, dtype=x.dtype, device=x.device)) / 2
    h = (torch.as_tensor(hi, dtype=x.dtype, device=x.device) - torch.as_tensor(lo, dtype=x.dtype, device=x.device)) / 2
    q = (x - c).abs() - h
    return q.clamp(min=0).norm(dim=-1) + q.max(dim=-1).values.clamp(max=0)


def crease_sdf(x):
    """the union's distance function: min of the two boxes' exact distances (x [m, 3] -> [m], in x's dtype)"""
    return torch.minimum(_box_sdf(x, *FLOOR), _box_sdf(x, *WALL))


def crease_surface(points, ray_d):
    """the surface record of the union at points on it: the normal of the nearest box's nearest face, the constant material"""
    da, db = _box_sdf(points, *FLOOR), _box_sdf(points, *WALL)
    n = torch.zeros_like(points)
    for lo, hi, mine in ((FLOOR[0], FLOOR[1], da <= db), (WALL[0], WALL[1], db < da)):
        c = (torch.as_tensor(lo, dtype=points.dtype, device=points.device) + torch.as_tensor(hi, dtype=points.dtype, device=points.device)) / 2
        h = (torch.as_tensor(hi, dtype=points.dtype, device=points.device) - torch.as_tensor(lo, dtype=points.dtype, device=points.device)) / 2
        q = (points - c).abs() - h
        axis = q.argmax(dim=-1)
        nn = torch.zeros_like(points)
        nn.scatter_(1, axis[:, None], torch.sign(points - c).gather(1, axis[:, None]))
        n = torch.where(mine[:, None], nn, n)
    m = torch.tensor(MATERIAL, dtype=points.dtype, device=points.device)
    k = points.shape[0]
    return {"normal": n, "diffuse_albedo": m[None, :3].expand(k, 3).contiguous(), "specular_albedo": m[None, 3:6].expand(k, 3).contiguous(),
            "specular_roughness": m[6].expand(k).contiguous()}
