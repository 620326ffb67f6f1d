"""fp64 brute-force restatement of igl.point_mesh_squared_distance and of cal_mesh_err (evaluation/eval_mesh.py), in torch and
device-agnostic: CPU for the CPU tests, the GPU for the large check.  Test infrastructure: never uses the HIP library.

The closest point on a triangle follows Ericson's Voronoi-region routine (Real-Time Collision Detection, 5.1.5) in fp64, a
formulation independent of the kernel's; a triangle with (numerically) zero area falls back to the nearest of its three segments.
"""
from __future__ import annotations

import torch


def _dot(a, b):
    return (a * b).sum(-1)


def closest_on_segment(p, a, b):
    ab = b - a
    l2 = _dot(ab, ab)
    t = torch.where(l2 > 0, _dot(p - a, ab) / torch.where(l2 > 0, l2, torch.ones_like(l2)), torch.zeros_like(l2)).clamp(0.0, 1.0)
    return a + t[..., None] * ab


def _nearest(p, cands):
    best, bd = cands[0], _dot(p - cands[0], p - cands[0])
    for q in cands[1:]:
        d = _dot(p - q, p - q)
        take = d < bd
        best = torch.where(take[..., None], q, best)
        bd = torch.where(take, d, bd)
    return best


def closest_point_triangle(p, a, b, c):
    """Closest point of triangles (a, b, c) to points p, all [..., 3] fp64 (broadcasting)."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2

    def safe(x):
        return torch.where(x != 0, x, torch.ones_like(x))

    den = va + vb + vc
    res = a + ab * (vb / safe(den))[..., None] + ac * (vc / safe(den))[..., None]  # face region
    w = (d4 - d3) / safe((d4 - d3) + (d5 - d6))
    res = torch.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + w[..., None] * (c - b), res)  # edge BC
    w = d2 / safe(d2 - d6)
    res = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + w[..., None] * ac, res)  # edge AC
    res = torch.where(((d6 >= 0) & (d5 <= d6))[..., None], c.expand_as(res), res)  # vertex C
    v = d1 / safe(d1 - d3)
    res = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + v[..., None] * ab, res)  # edge AB
    res = torch.where(((d3 >= 0) & (d4 <= d3))[..., None], b.expand_as(res), res)  # vertex B
    res = torch.where(((d1 <= 0) & (d2 <= 0))[..., None], a.expand_as(res), res)  # vertex A
    n = torch.cross(ab.expand_as(res), ac.expand_as(res), dim=-1)
    degenerate = _dot(n, n) <= 1e-24 * _dot(ab, ab) * _dot(ac, ac)
    if bool(degenerate.any()):
        seg = _nearest(p.expand_as(res), [closest_on_segment(p, a, b).expand_as(res), closest_on_segment(p, b, c).expand_as(res),
                                          closest_on_segment(p, c, a).expand_as(res)])
        res = torch.where(degenerate[..., None], seg, res)
    return res


def point_face_sqr_dist(P, V, F, I):
    """fp64 squared distance and closest point of each P[k] to its face F[I[k]]."""
    P, V = P.double(), V.double()
    t = F.long()[I.long()]
    c = closest_point_triangle(P, V[t[:, 0]], V[t[:, 1]], V[t[:, 2]])
    return _dot(P - c, P - c), c


def _reduce(P, V, F, pidx, fidx, n):
    """min over the (point, face) pairs -> (sqrD, I (smallest index among exact minima), C)."""
    d, c = point_face_sqr_dist(P[pidx], V, F, fidx)
    inf = torch.full((n,), float("inf"), dtype=torch.float64, device=P.device)
    dmin = inf.scatter_reduce(0, pidx, d, reduce="amin")
    big = torch.full((n,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=P.device)
    cand = torch.where(d == dmin[pidx], fidx, torch.full_like(fidx, torch.iinfo(torch.int64).max))
    imin = big.scatter_reduce(0, pidx, cand, reduce="amin")
    return dmin, imin


def point_mesh_squared_distance(P, V, F, upper=None, point_chunk=None, face_chunk=1 << 20):
    """fp64 brute force over all faces: (sqrD [N], I [N] int64, C [N, 3]) on P's device.  Ties (exact fp64 equality) go to the
    smallest face index.  `upper` [N]: an optional upper bound of each point's squared distance (e.g. its fp64 distance to any
    one face); only the faces whose bounding sphere can come within it are evaluated, which cannot change the minimum."""
    P = torch.as_tensor(P).double()
    dev = P.device
    V = torch.as_tensor(V).double().to(dev)
    F = torch.as_tensor(F).long().to(dev)
    n, nf = P.shape[0], F.shape[0]
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    if point_chunk is None:
        point_chunk = max(1, (1 << 22) // max(nf, 1)) if upper is None else 512
    dmin = torch.full((n,), float("inf"), dtype=torch.float64, device=dev)
    imin = torch.zeros((n,), dtype=torch.int64, device=dev)
    if upper is not None:
        # bounding spheres (centroid m, radius r): |p - m| <= s + r, s = sqrt(upper), is necessary for a face to come within
        # upper.  Squared and expanded it is one fp64 product per chunk, A [k, 6] @ B [6, F] <= 0, with a margin far above the
        # expansion's cancellation (~1e-16 of |p|^2 + |m|^2)
        m = (a + b + c) / 3.0
        r = torch.sqrt(torch.stack([_dot(a - m, a - m), _dot(b - m, b - m), _dot(c - m, c - m)], -1).max(-1).values) * (1 + 1e-12)
        s = torch.sqrt(torch.as_tensor(upper).double().to(dev)) * (1 + 1e-9) + 1e-12
        pp = _dot(P, P)
        Amat = torch.stack([P[:, 0], P[:, 1], P[:, 2], torch.ones_like(s), s, pp - s * s], -1)
        Bmat = torch.stack([-2 * m[:, 0], -2 * m[:, 1], -2 * m[:, 2], _dot(m, m) - r * r, -2 * r, torch.ones_like(r)], 0)
        margin = 1e-10 * (pp + _dot(m, m).max() + (s + r.max()) ** 2)
    for i0 in range(0, n, point_chunk):
        p = P[i0:i0 + point_chunk]
        k = p.shape[0]
        for j0 in range(0, nf, face_chunk):
            sl = slice(j0, j0 + face_chunk)
            if upper is None:
                pi = torch.arange(k, device=dev).repeat_interleave(min(face_chunk, nf - j0))
                fi = torch.arange(j0, min(j0 + face_chunk, nf), device=dev).repeat(k)
            else:
                keep = Amat[i0:i0 + k] @ Bmat[:, sl] <= margin[i0:i0 + k, None]
                pi, fi = keep.nonzero(as_tuple=True)
                fi = fi + j0
            if pi.numel() == 0:
                continue
            d, i = _reduce(p, V, F, pi, fi, k)
            cur_d, cur_i = dmin[i0:i0 + k], imin[i0:i0 + k]
            better = (d < cur_d) | ((d == cur_d) & (i < cur_i))
            dmin[i0:i0 + k] = torch.where(better, d, cur_d)
            imin[i0:i0 + k] = torch.where(better, i, cur_i)
    found = torch.isfinite(dmin)
    _, C = point_face_sqr_dist(P, V, F, torch.where(found, imin, torch.zeros_like(imin)))
    return dmin, imin, C


def cal_mesh_err(va, fa, vb, fb, sqr_dist=point_mesh_squared_distance):
    """evaluation/eval_mesh.py:6-12, restated: D1 = sqrt(sqrD(va -> mesh b)), D2 = sqrt(sqrD(vb -> mesh a)),
    0.5 * (D1.mean() + D2.mean())."""
    sqrD1 = sqr_dist(va, vb, fb)[0]
    sqrD2 = sqr_dist(vb, va, fa)[0]
    return float((torch.sqrt(torch.as_tensor(sqrD1, dtype=torch.float64)).mean()
                  + torch.sqrt(torch.as_tensor(sqrD2, dtype=torch.float64)).mean()) * 0.5)


# ---- test meshes ----
def unit_cube():
    """[0, 1]^3 as 12 triangles (outward normals)."""
    v = torch.tensor([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)], dtype=torch.float64)
    f = torch.tensor([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4],
                      [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]], dtype=torch.int64)
    return v, f


def regular_tetrahedron():
    v = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=torch.int64)
    return v, f


def triangle_soup(n_faces=2000, degenerate_share=0.05, seed=0):
    """Random triangles in [0, 1]^3 (sizes from tiny to large); about `degenerate_share` of them have coincident or collinear
    vertices, built exactly in fp32."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand((n_faces, 1, 3), generator=g, dtype=torch.float64)
    size = 10 ** (-2.0 * torch.rand((n_faces, 1, 1), generator=g, dtype=torch.float64))
    tri = (centre + size * (torch.rand((n_faces, 3, 3), generator=g, dtype=torch.float64) - 0.5)).float()
    nd = int(round(n_faces * degenerate_share))
    idx = torch.randperm(n_faces, generator=g)[:nd]
    for j, k in enumerate(idx.tolist()):
        kind = j % 3
        if kind == 0:  # all three coincide
            tri[k, 1] = tri[k, 0]
            tri[k, 2] = tri[k, 0]
        elif kind == 1:  # two coincide
            tri[k, 2] = tri[k, 1]
        else:  # collinear along an axis-aligned line (exact in fp32): C outside the segment AB
            a = tri[k, 0].clone()
            tri[k, 1] = a + torch.tensor([0.25, 0.0, 0.0])
            tri[k, 2] = a + torch.tensor([-0.125, 0.0, 0.0])
    v = tri.reshape(-1, 3)
    f = torch.arange(3 * n_faces, dtype=torch.int64).reshape(-1, 3)
    return v.double(), f
