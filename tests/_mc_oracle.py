"""Vectorised numpy restatement of the marching cubes of csrc/mcubes.hip (conventions: iron_amd/mc_table.py and
include/iron_hip.h).  Test infrastructure: uses the generated case table, never the HIP library."""
from __future__ import annotations

import numpy as np

from iron_amd import mc_table

_TRI = np.full((256, 3 * mc_table.MAX_TRIS), -1, dtype=np.int64)
for _c, _t in enumerate(mc_table.TABLE):
    _flat = [e for tri in _t for e in tri]
    _TRI[_c, :len(_flat)] = _flat
_EDGE_ORIGIN = np.array(mc_table.EDGE_ORIGIN, dtype=np.int64)
_EDGE_AXIS = np.array(mc_table.EDGE_AXIS, dtype=np.int64)


def marching_cubes(u: np.ndarray, threshold: float = 0.0):
    """u float32 [nx, ny, nz] -> (verts float32 [V, 3] in index coordinates, tris int64 [T, 3])."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    thr = np.float32(threshold)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    if u.ndim != 3 or min(u.shape) < 2:
        return empty
    nx, ny, nz = u.shape
    with np.errstate(invalid="ignore"):
        above = u > thr  # NaN compares false: below
    # crossed owned edges of every lattice point, [nx, ny, nz, 3] (axis fastest = vertex order)
    crossed = np.zeros(u.shape + (3,), dtype=bool)
    crossed[:-1, :, :, 0] = above[:-1] != above[1:]
    crossed[:, :-1, :, 1] = above[:, :-1] != above[:, 1:]
    crossed[:, :, :-1, 2] = above[:, :, :-1] != above[:, :, 1:]
    flat = crossed.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1  # vertex index of (point, axis) where crossed
    idx = np.nonzero(flat)[0]
    p, axis = idx // 3, idx % 3
    i, j, k = p // (ny * nz), (p // nz) % ny, p % nz
    pt = np.stack([i, j, k], axis=1)
    q = pt.copy()
    q[np.arange(len(q)), axis] += 1
    u0 = u[i, j, k]
    u1 = u[q[:, 0], q[:, 1], q[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (thr - u0) / (u1 - u0)
        t = np.where(t >= np.float32(0), t, np.float32(0)).astype(np.float32)
        t = np.where(t > np.float32(1), np.float32(1), t).astype(np.float32)
    verts = pt.astype(np.float32)
    verts[np.arange(len(verts)), axis] += t
    # cells, in linear order of their min corner
    a = above.astype(np.int64)
    cube = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(mc_table.CORNERS):
        cube |= a[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] << c
    ci, cj, ck = np.nonzero((cube != 0) & (cube != 255))
    rows = _TRI[cube[ci, cj, ck]]  # [A, 3 * max]
    valid = rows >= 0
    e = np.where(valid, rows, 0)
    o = _EDGE_ORIGIN[e]  # [A, 3 * max, 3]
    oi, oj, ok = ci[:, None] + o[..., 0], cj[:, None] + o[..., 1], ck[:, None] + o[..., 2]
    lin = (oi * ny + oj) * nz + ok
    ids = vid[lin * 3 + _EDGE_AXIS[e]]
    tris = ids[valid].reshape(-1, 3)
    return verts, tris


def sphere(n: int, r: float, center=None) -> np.ndarray:
    """u = r - |x - c| on an n^3 lattice of index coordinates (above inside)."""
    c = (n - 1) / 2.0 if center is None else center
    g = np.arange(n, dtype=np.float64) - c
    d = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    return (r - d).astype(np.float32)


def edge_check(tris: np.ndarray):
    """(count of undirected edges, of those used by exactly 2 triangles in opposite directions)."""
    a = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]])
    b = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * (int(tris.max()) + 1 if len(tris) else 1) + hi
    sign = np.where(a < b, 1, -1)
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    s = np.zeros(len(uniq), dtype=np.int64)
    np.add.at(s, inv, sign)
    return len(uniq), int(((cnt == 2) & (s == 0)).sum())


def volume(verts: np.ndarray, tris: np.ndarray) -> float:
    """Divergence-theorem volume sum(v0 . (v1 x v2)) / 6, positive for outward normals."""
    v = verts.astype(np.float64)
    v0, v1, v2 = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6.0)
