"""numpy restatement of Smart UV project (iron_amd/uv_unwrap.py, csrc/uvunwrap.hip) and of export_mesh's lattices,
for the CPU tests and the GPU parity tests.  Same fp32 face formulas and angle sets as the kernels; components come from
scipy.sparse.csgraph; the host packer (iron_amd.uv_unwrap.pack_boxes, plain numpy) is shared.  Every decision the algorithm makes
is returned with its margin, so a parity fixture that loses its margin fails loudly instead of flaking.  The projection normals are
summed in the kernels' fixed order (fixed_order_sum), so with IEEE fp32 on both sides every later value agrees bitwise."""
from __future__ import annotations

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from iron_amd.uv_unwrap import pack_boxes

f32 = np.float32


def face_geometry(V, F):
    """-> (unit normals fp32 [F,3] (zeros when degenerate), a = |(v1-v0) x (v2-v0)| fp32 [F])."""
    p = np.asarray(V, dtype=f32)[np.asarray(F)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
    a = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    n = np.zeros_like(c)
    ok = a > 0
    n[ok] = c[ok] / a[ok, None]
    return n, a


def dot(n, p):
    p = np.asarray(p, dtype=f32)
    return n[:, 0] * p[0] + n[:, 1] * p[1] + n[:, 2] * p[2]


def fixed_order_sum(x, block=256):
    """fp32 sum of the rows of x [N, 3] in the kernels' order: a tree over each block of 256 rows, then each of 256 lanes adds the
    block partials t, t + 256, ... in turn, then a tree over the lanes (k_uv_cone / k_uv_cone_sum)."""
    nb = max(1, -(-len(x) // block))
    s = np.zeros((nb * block, 3), dtype=f32)
    s[:len(x)] = x
    s = s.reshape(nb, block, 3)
    h = block // 2
    while h > 0:
        s[:, :h] = s[:, :h] + s[:, h:2 * h]
        h //= 2
    part = s[:, 0]
    m = -(-nb // block)
    q = np.zeros((m * block, 3), dtype=f32)
    q[:nb] = part
    q = q.reshape(m, block, 3)
    acc = np.zeros((block, 3), dtype=f32)
    for r in range(m):
        acc = acc + q[r]
    h = block // 2
    while h > 0:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def projections(n, a, angle_limit=66.0):
    """-> (P fp32 [K,3], margins dict).  margins: 'cone' = min |n.seed - cos(limit/2)| over the faces tested, 'stop' = min
    |max_p n.p - cos(limit)| at the stop decisions, 'argmin' = min gap between the farthest face and the runner-up."""
    alpha = np.radians(angle_limit)
    ch, cl = f32(np.cos(alpha / 2)), f32(np.cos(alpha))
    nondeg = a > 0
    tag = np.full(len(a), -1)
    seed = int(np.argmax(a))
    P, runmax = [], None
    mg = {"cone": np.inf, "stop": np.inf, "argmin": np.inf}
    k = 0
    while True:
        cand = (tag < 0) & nondeg
        if a[seed] > 0:
            d = dot(n, n[seed])
            new = cand & (d > ch)
            if cand.any():
                mg["cone"] = min(mg["cone"], float(np.abs(d[cand].astype(np.float64) - ch).min()))
        else:
            new = np.zeros_like(cand)
        tag[new] = k
        s = fixed_order_sum(np.where(new[:, None], n, f32(0)))
        ln = np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
        P.append((s / ln).astype(f32) if ln > 0 else np.array([0, 0, 1], f32))
        d = dot(n, P[-1])
        runmax = d if runmax is None else np.maximum(runmax, d)
        un = np.flatnonzero((tag < 0) & nondeg)
        if len(un) == 0:
            break
        vals = runmax[un]
        j = int(np.argmin(vals))
        if len(un) > 1:
            mg["argmin"] = min(mg["argmin"], float(np.partition(vals.astype(np.float64), 1)[1] - vals[j]))
        mg["stop"] = min(mg["stop"], abs(float(vals[j]) - float(cl)))
        if vals[j] >= cl:
            break
        seed = int(un[j])
        k += 1
    return np.stack(P), mg


def assign(n, a, P):
    """-> (g int [F], margin = min over non-degenerate faces of best - second-best n.p)."""
    D = np.stack([dot(n, p) for p in P], 1)
    g = np.argmax(D, 1)
    g[a == 0] = 0
    margin = np.inf
    if D.shape[1] > 1 and (a > 0).any():
        Ds = np.sort(D[a > 0].astype(np.float64), 1)
        margin = float((Ds[:, -1] - Ds[:, -2]).min())
    return g, margin


def components(F, group=None):
    """-> labels [F] (0..K-1 in order of first face), K.  Faces joined across edges with two distinct indices, equal group only."""
    F = np.asarray(F, dtype=np.int64)
    nf = len(F)
    g = np.zeros(nf, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    a, b = F, np.roll(F, -1, axis=1)
    lo, hi = np.minimum(a, b).reshape(-1), np.maximum(a, b).reshape(-1)
    face = np.repeat(np.arange(nf), 3)
    keep = lo != hi
    key, face = (lo[keep] << 32) | hi[keep], face[keep]
    o = np.argsort(key, kind="stable")
    key, face = key[o], face[o]
    rows, cols = [], []
    for d in range(1, len(key)):
        same = key[:-d] == key[d:]
        if not same.any():
            break
        i = np.flatnonzero(same)
        ok = g[face[i]] == g[face[i + d]]
        rows.append(face[i[ok]]); cols.append(face[i[ok] + d])
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    m = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nf, nf))
    k, lab = connected_components(m, directed=False)
    _, first = np.unique(lab, return_index=True)
    rank = np.empty(k, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(k)
    return rank[lab], k


def basis(p):
    p = np.asarray(p, dtype=f32)
    ab = np.abs(p)
    e = 0 if (ab[0] <= ab[1] and ab[0] <= ab[2]) else (1 if ab[1] <= ab[2] else 2)
    z = f32(0)
    c = [np.array([z, -p[2], p[1]]), np.array([p[2], z, -p[0]]), np.array([-p[1], p[0], z])][e].astype(f32)
    ln = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    t = (c / ln).astype(f32)
    b = np.array([p[1] * t[2] - p[2] * t[1], p[2] * t[0] - p[0] * t[2], p[0] * t[1] - p[1] * t[0]], dtype=f32)
    return t, b


def coarse_table():
    r = np.radians(np.arange(90, dtype=np.float64) * 1.0)
    return np.stack([np.cos(r), np.sin(r)], -1).astype(f32)


def fine_table(coarse_idx):
    deg = np.asarray(coarse_idx, dtype=np.float64)[:, None] * 1.0 + np.arange(-20, 21) * 0.05
    r = np.radians(deg)
    return np.stack([np.cos(r), np.sin(r)], -1).astype(f32)


def _boxes(x, y, c, s, starts):
    """x, y [T]; c, s [T, A] per-vt angle -> min/max per (island, angle) over sorted island segments."""
    xr = x[:, None] * c - y[:, None] * s
    yr = x[:, None] * s + y[:, None] * c
    return (np.minimum.reduceat(xr, starts, 0), np.minimum.reduceat(yr, starts, 0), np.maximum.reduceat(xr, starts, 0),
            np.maximum.reduceat(yr, starts, 0))


def _pick(b):
    area = (b[2] - b[0]) * (b[3] - b[1])  # fp32 [K, A]
    idx = np.argmin(area, 1)
    srt = np.sort(area.astype(np.float64), 1)
    best = srt[:, 0]
    rel = (srt[:, 1] - best) / np.maximum(best, 1e-30) if area.shape[1] > 1 else np.full(len(best), np.inf)
    return idx, rel


def smart_uv_project(V, F, angle_limit=66.0, island_margin=0.0):
    """-> dict: uvs fp32 [T,2], face_uvs [F,3], P, g, labels, K, scale, boxes (rotated, before the swap) and the decision margins."""
    V = np.asarray(V, dtype=f32)
    F = np.asarray(F, dtype=np.int64)
    n, a = face_geometry(V, F)
    P, mg = projections(n, a, angle_limit)
    g, mg["assign"] = assign(n, a, P)
    labels, K = components(F, g)
    corner = ((labels[:, None].astype(np.int64) << 32) | F).reshape(-1)
    uniq, inv = np.unique(corner, return_inverse=True)
    vt_vertex, vt_island = (uniq & 0xFFFFFFFF).astype(np.int64), (uniq >> 32).astype(np.int64)
    island_group = np.zeros(K, dtype=np.int64)
    island_group[labels] = g
    xy = np.zeros((len(uniq), 2), dtype=f32)
    for p_i in range(len(P)):
        t, b = basis(P[p_i])
        sel = island_group[vt_island] == p_i
        xy[sel, 0] = dot(V[vt_vertex[sel]], t)
        xy[sel, 1] = dot(V[vt_vertex[sel]], b)
    starts = np.flatnonzero(np.r_[True, vt_island[1:] != vt_island[:-1]])
    x, y = xy[:, 0], xy[:, 1]
    cs = coarse_table()
    coarse, rel_c = _pick(_boxes(x, y, cs[None, :, 0], cs[None, :, 1], starts))
    fine = fine_table(coarse)
    fv = fine[vt_island]
    bx = _boxes(x, y, fv[:, :, 0], fv[:, :, 1], starts)
    fidx, rel_f = _pick(bx)
    kk = np.arange(K)
    box = np.stack([bx[0][kk, fidx], bx[1][kk, fidx], bx[2][kk, fidx], bx[3][kk, fidx]], 1)
    bw, bh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    swap = bh > bw
    off, s = pack_boxes(np.where(swap, bh, bw), np.where(swap, bw, bh), island_margin)
    c, sn = fine[kk, fidx, 0][vt_island], fine[kk, fidx, 1][vt_island]
    ox, oy = (off[:, 0] / s).astype(f32)[vt_island], (off[:, 1] / s).astype(f32)[vt_island]
    xr, yr = x * c - y * sn, x * sn + y * c
    sw = swap[vt_island]
    u = np.where(sw, box[vt_island, 3] - yr, xr - box[vt_island, 0])
    w = np.where(sw, xr - box[vt_island, 0], yr - box[vt_island, 1])
    s32 = f32(s)
    uvs = np.stack([np.clip((u + ox) * s32, 0, 1), np.clip((w + oy) * s32, 0, 1)], -1).astype(f32)
    mg["coarse_area"] = float(rel_c.min()) if K else np.inf
    mg["fine_area"] = float(rel_f.min()) if K else np.inf
    mg["swap"] = float(np.abs(bh.astype(np.float64) - bw).min() / max(float(np.abs(bw).max()), 1e-30)) if K else np.inf
    return dict(uvs=uvs, face_uvs=inv.reshape(-1, 3), P=P, g=g, labels=labels, K=K, scale=s, normals=n, area=a, box=box, swap=swap,
                offsets=off, margins=mg, vt_island=vt_island)


# ---- checks shared by the CPU and GPU tests ----
def signed_uv_area(uvs, face_uvs):
    t = np.asarray(uvs, dtype=np.float64)[np.asarray(face_uvs)]
    return 0.5 * ((t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 2, 0] - t[:, 0, 0]) * (t[:, 1, 1] - t[:, 0, 1]))


def island_boxes(uvs, face_uvs, labels, K):
    t = np.asarray(uvs, dtype=np.float64)[np.asarray(face_uvs)]
    lo, hi = np.full((K, 2), np.inf), np.full((K, 2), -np.inf)
    for c in range(3):
        np.minimum.at(lo, labels, t[:, c])
        np.maximum.at(hi, labels, t[:, c])
    return lo, hi


def boxes_disjoint(lo, hi, gap, tol=1e-6):
    """True when every two boxes are >= gap - tol apart along x or y (sweep over x; O(K log K + overlapping pairs))."""
    o = np.argsort(lo[:, 0], kind="stable")
    active = []
    for i in o:
        active = [j for j in active if hi[j, 0] + gap - tol > lo[i, 0]]
        for j in active:
            if lo[i, 1] < hi[j, 1] + gap - tol and lo[j, 1] < hi[i, 1] + gap - tol:
                return False
        active.append(i)
    return True


# ---- closed-form meshes ----
def cube():
    V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=f32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # outward: -x, +x, -y, +y, -z, +z
    F = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], dtype=np.int64)
    return V, F


def height_field(n=24, amp=0.05, seed=0):
    r = np.random.default_rng(seed)
    xs = np.linspace(0, 1, n)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    Z = amp * np.sin(6 * X) * np.cos(5 * Y) + 0.002 * r.standard_normal(X.shape)
    V = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(f32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    F = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return V, F.astype(np.int64)


def uv_sphere(n_lat=12, n_lon=16, center=(0, 0, 0), r=1.0):
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    pts = [[0, 0, r]] + [[r * np.sin(t) * np.cos(p), r * np.sin(t) * np.sin(p), r * np.cos(t)] for t in th for p in ph] + [[0, 0, -r]]
    V = (np.array(pts) + np.asarray(center)).astype(f32)
    F = []
    for j in range(n_lon):
        F.append((0, 1 + j, 1 + (j + 1) % n_lon))
    for i in range(n_lat - 2):
        for j in range(n_lon):
            a, b = 1 + i * n_lon + j, 1 + i * n_lon + (j + 1) % n_lon
            c, d = a + n_lon, b + n_lon
            F += [(a, c, d), (a, d, b)]
    last = len(V) - 1
    base = 1 + (n_lat - 2) * n_lon
    for j in range(n_lon):
        F.append((base + j, last, base + (j + 1) % n_lon))
    return V, np.array(F, dtype=np.int64)


# ---- export_mesh's lattices (models/export_mesh.py get_grid_uniform / get_grid), restated ----
def grid_uniform_axes(resolution):
    x = np.linspace(-1.0, 1.0, resolution)
    return [x, x, x]


def grid_axes(points, resolution, eps=0.1):
    lo, hi = np.asarray(points, dtype=f32).min(0), np.asarray(points, dtype=f32).max(0)
    s = int(np.argmin(hi - lo))
    axes = [None] * 3
    axes[s] = np.linspace(lo[s] - eps, hi[s] + eps, resolution)
    step = (np.max(axes[s]) - np.min(axes[s])) / (resolution - 1)
    for i in range(3):
        if i != s:
            axes[i] = np.arange(lo[i] - eps, hi[i] + step + eps, step)
    return axes, s
