"""fp64 restatement of the asset renderer's building blocks (csrc/meshrender.hip), in torch and device-agnostic: CPU for the CPU
tests, the GPU for the larger checks.  Test infrastructure: never uses the HIP library.

The ray-triangle test is Moeller-Trumbore over every face (a formulation independent of the kernel's ray-space edge functions),
with inclusive edge tests (u >= 0, v >= 0, u + v <= 1), faces two-sided, hits with t in (t_min, t_max], the smallest face index
among equal t.  `dtype=torch.float32` runs the same formulas in fp32: the textbook formulation the kernel is measured against.
"""
from __future__ import annotations

import math

import torch

INF = float("inf")


def _dot(a, b):
    return (a * b).sum(-1)


def closest_hit(ray_o, ray_d, V, F, t_min=0.0, t_max=INF, dtype=torch.float64, pair_chunk=1 << 21):
    """-> (t [n], face [n] int64 (-1: miss), bary [n, 2] (weights of the face's second and third vertex), margin [n]: the hit's
    smallest barycentric weight min(u, v, 1 - u - v)), in `dtype`, on ray_o's device.  Non-finite or zero rays miss."""
    dev = ray_o.device
    o, d = ray_o.to(dtype), ray_d.to(dtype)
    V = torch.as_tensor(V).to(device=dev, dtype=dtype)
    F = torch.as_tensor(F).long().to(dev)
    n, nf = o.shape[0], F.shape[0]
    a, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    t_out = torch.full((n,), INF, dtype=dtype, device=dev)
    f_out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    b_out = torch.zeros((n, 2), dtype=dtype, device=dev)
    m_out = torch.zeros((n,), dtype=dtype, device=dev)
    valid = torch.isfinite(o).all(-1) & torch.isfinite(d).all(-1) & (d != 0).any(-1)
    rc = max(1, pair_chunk // max(nf, 1))
    big = torch.iinfo(torch.int64).max
    ar = torch.arange(nf, device=dev)
    for i0 in range(0, n, rc):
        oo, dd = o[i0:i0 + rc, None, :], d[i0:i0 + rc, None, :]
        k = oo.shape[0]
        p = torch.cross(dd.expand(k, nf, 3), e2[None].expand(k, nf, 3), dim=-1)
        det = _dot(e1[None], p)
        s = oo - a[None]
        u = _dot(s, p) / det
        q = torch.cross(s, e1[None].expand(k, nf, 3), dim=-1)
        v = _dot(dd, q) / det
        t = _dot(e2[None], q) / det
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_min) & (t <= t_max) & valid[i0:i0 + k, None]
        tt = torch.where(ok, t, torch.full_like(t, INF))
        tm = tt.min(1).values
        fi = torch.where(ok & (tt == tm[:, None]), ar[None], torch.full((1, 1), big, device=dev)).min(1).values
        hit = fi != big
        g = torch.where(hit, fi, torch.zeros_like(fi))[:, None]
        uu, vv = u.gather(1, g)[:, 0], v.gather(1, g)[:, 0]
        t_out[i0:i0 + k] = torch.where(hit, tm, torch.full_like(tm, INF))
        f_out[i0:i0 + k] = torch.where(hit, fi, torch.full_like(fi, -1))
        zero = torch.zeros_like(uu)
        b_out[i0:i0 + k, 0] = torch.where(hit, uu, zero)
        b_out[i0:i0 + k, 1] = torch.where(hit, vv, zero)
        m_out[i0:i0 + k] = torch.where(hit, torch.minimum(torch.minimum(uu, vv), 1 - uu - vv), zero)
    return t_out, f_out, b_out, m_out


def vertex_normals(V, F):
    """-> (normals fp64 [nv, 3] (zero where the sum is zero), |sum| [nv], sum of |terms| [nv]): area-weighted, the sum of the
    faces' un-normalised cross products."""
    V = torch.as_tensor(V).double()
    F = torch.as_tensor(F).long().to(V.device)
    c = torch.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]], dim=-1)
    acc = torch.zeros_like(V)
    mag = torch.zeros(V.shape[0], dtype=torch.float64, device=V.device)
    for k in range(3):
        acc.index_add_(0, F[:, k], c)
        mag.index_add_(0, F[:, k], c.norm(dim=-1))
    l = acc.norm(dim=-1)
    n = torch.where(l[:, None] > 0, acc / torch.where(l > 0, l, torch.ones_like(l))[:, None], torch.zeros_like(acc))
    return n, l, mag


def texture_fetch(tex, uv, weight=None, mode="bilinear"):
    """The bake's convention in fp64: x = uv_x W - 1/2, y = (H - uv_y H) - 1/2, four taps clamped to the edge; nearest: texel
    (floor(H - uv_y H), floor(uv_x W)), clamped.  With `weight`, taps whose weight is 0 are dropped and the rest renormalised.
    -> (values [n, C], hole [n] bool)."""
    tex = torch.as_tensor(tex).double()
    if tex.dim() == 2:
        tex = tex[..., None]
    H, W, C = tex.shape
    uv = torch.as_tensor(uv).double().to(tex.device)
    flat = tex.reshape(H * W, C)
    wflat = None if weight is None else torch.as_tensor(weight).double().to(tex.device).reshape(-1)
    xu, yv = uv[:, 0] * W, H - uv[:, 1] * H
    if mode == "nearest":
        idx = torch.floor(yv).clamp(0, H - 1).long() * W + torch.floor(xu).clamp(0, W - 1).long()
        hole = torch.zeros_like(idx, dtype=torch.bool) if wflat is None else ~(wflat[idx] > 0)
        return torch.where(hole[:, None], torch.zeros((1, C), dtype=torch.float64, device=tex.device), flat[idx]), hole
    x, y = xu - 0.5, yv - 0.5
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    vals = torch.zeros((uv.shape[0], C), dtype=torch.float64, device=tex.device)
    wsum = torch.zeros(uv.shape[0], dtype=torch.float64, device=tex.device)
    for dy, dx, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
        idx = (y0 + dy).clamp(0, H - 1).long() * W + (x0 + dx).clamp(0, W - 1).long()
        if wflat is not None:
            w = torch.where(wflat[idx] > 0, w, torch.zeros_like(w))
        vals += w[:, None] * flat[idx]
        wsum += w
    if wflat is None:
        return vals, torch.zeros(uv.shape[0], dtype=torch.bool, device=tex.device)
    hole = ~(wsum > 0)
    return torch.where(hole[:, None], torch.zeros_like(vals), vals / torch.where(hole, torch.ones_like(wsum), wsum)[:, None]), hole


# ---- test meshes and rays ----
def uv_sphere(nlat=48, nlon=96, r=0.6):
    """A closed UV sphere: 2 + (nlat - 1) nlon vertices, 2 nlon (nlat - 1) faces (9 024 for 48 x 96), outward winding."""
    V = [[0.0, 0.0, r]]
    for i in range(1, nlat):
        th = math.pi * i / nlat
        for j in range(nlon):
            ph = 2 * math.pi * j / nlon
            V.append([r * math.sin(th) * math.cos(ph), r * math.sin(th) * math.sin(ph), r * math.cos(th)])
    V.append([0.0, 0.0, -r])

    def idx(i, j):
        return 1 + (i - 1) * nlon + (j % nlon)

    F = [[0, idx(1, j), idx(1, j + 1)] for j in range(nlon)]
    for i in range(1, nlat - 1):
        for j in range(nlon):
            F.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            F.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    S = len(V) - 1
    F += [[S, idx(nlat - 1, j + 1), idx(nlat - 1, j)] for j in range(nlon)]
    return torch.tensor(V, dtype=torch.float64).float().double(), torch.tensor(F, dtype=torch.int64)


def pinhole_rays(cam, W, H, focal, target=(0.0, 0.0, 0.0)):
    """Unit directions [H * W, 3] (fp64) of a pinhole camera at `cam` looking at `target`, pixel centres, row-major."""
    cam = torch.as_tensor(cam, dtype=torch.float64)
    fwd = torch.as_tensor(target, dtype=torch.float64) - cam
    fwd = fwd / fwd.norm()
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    right = torch.cross(fwd, up, dim=0)
    right = right / right.norm()
    up2 = torch.cross(right, fwd, dim=0)
    uu, vv = torch.meshgrid(torch.arange(W, dtype=torch.float64) + 0.5, torch.arange(H, dtype=torch.float64) + 0.5, indexing="xy")
    d = ((uu - W / 2) / focal)[..., None] * right + (-(vv - H / 2) / focal)[..., None] * up2 + fwd
    d = (d / d.norm(dim=-1, keepdim=True)).reshape(-1, 3)
    return cam[None].expand_as(d).contiguous(), d


def edge_targets(V, F, cam, n=3000, min_cos=0.2, seed=1):
    """Points on the mesh's vertices, edge midpoints and edge quarter points that face `cam` (cosine between the outward
    direction of a sphere-like mesh and the direction to the camera above min_cos), a random choice of n of them (fp64, rounded
    through fp32)."""
    V = torch.as_tensor(V).double()
    cam = torch.as_tensor(cam, dtype=torch.float64)
    E = torch.cat([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    E = torch.unique(torch.sort(E, 1).values, dim=0)
    tg = torch.cat([V, (V[E[:, 0]] + V[E[:, 1]]) / 2, V[E[:, 0]] * 0.25 + V[E[:, 1]] * 0.75]).float().double()
    nt = tg / tg.norm(dim=1, keepdim=True)
    to_cam = cam[None] - tg
    tg = tg[_dot(to_cam, nt) / to_cam.norm(dim=1) > min_cos]
    sel = torch.randperm(tg.shape[0], generator=torch.Generator().manual_seed(seed))[:n]
    return tg[sel]
