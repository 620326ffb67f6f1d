"""numpy restatement of models/export_materials.py's sample_surface and accumulate_splat_material (the texture bake), and the
integer-only recipe of the G21 fixture mesh.  Pinned to the reference by tests/test_bake_oracle.py against G21; the GPU tests
compare csrc/texbake.hip with it."""
from __future__ import annotations

import hashlib

import numpy as np

G21_N = 12           # grid cells per side of the fixture surface
G21_HW = (96, 64)    # texture_H, texture_W of the splat cases


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def g21_mesh():
    """A bumpy height-field grid, 2 * 12^2 triangles, uv running from -0.05 to 1.05, plus one zero-area face at the end.
    -> (vertices float32 [V,3], faces int64 [F,3], uvs float32 [V,2], face_uvs int64 [F,3]); faces index uvs one to one."""
    n = G21_N
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    verts = np.stack([i / n, j / n, ((i * 7 + j * 13) % 11) / 44.0], axis=1).astype(np.float32)
    uvs = np.stack([(i * 11 - 6) / 120.0, (j * 11 - 6) / 120.0], axis=1).astype(np.float32)
    faces = []
    for a in range(n):
        for b in range(n):
            p00, p10, p01, p11 = a * (n + 1) + b, (a + 1) * (n + 1) + b, a * (n + 1) + b + 1, (a + 1) * (n + 1) + b + 1
            faces += [[p00, p10, p11], [p00, p11, p01]]
    faces.append([5, 5, 6])  # zero area
    faces = np.asarray(faces, dtype=np.int64)
    return verts, faces, uvs, faces.copy()


def g21_values(n, c, salt):
    """Integer recipe for splatted values in [0, 1]: [n, c] float32."""
    k = np.arange(n).reshape(-1, 1)
    ch = np.arange(c).reshape(1, -1)
    return (((k * 37 + ch * 11 + salt * 5) % 101) / 100.0).astype(np.float32)


def g21_edge_uvs():
    """uv on 0 and 1, outside [0, 1], and on texel borders of the 96 x 64 texture: taps that wrap and taps that drop."""
    xs = np.array([0.0, 1.0, -0.01, 1.01, 0.5, 0.999, 0.5 / 64, 1.0 / 64, 63.5 / 64, -0.5 / 64, 0.3], dtype=np.float32)
    ys = np.array([0.0, 1.0, -0.01, 1.01, 0.5, 0.003, 0.5 / 96, 1.0 / 96, 95.5 / 96, 1.02, 0.7], dtype=np.float32)
    u, v = np.meshgrid(xs, ys, indexing="ij")
    return np.stack([u.reshape(-1), v.reshape(-1)], axis=1).astype(np.float32)


def atlas(n_faces, size, gutter):
    """A per-triangle UV atlas: triangle k in cell (k // m, k % m) of an m x m grid, corners inset by `gutter` texels, so no two
    triangles share a texel or a splat neighbourhood.  -> (uvs float32 [3F, 2], face_uvs int64 [F, 3])."""
    m = int(np.ceil(np.sqrt(n_faces)))
    cell = size / m
    k = np.arange(n_faces)
    x0 = (k % m) * cell + gutter
    y0 = (k // m) * cell + gutter
    s = cell - 2 * gutter
    corners = np.stack([np.stack([x0, y0], 1), np.stack([x0 + s, y0], 1), np.stack([x0, y0 + s], 1)], 1) / size
    return corners.reshape(-1, 2).astype(np.float32), np.arange(3 * n_faces).reshape(-1, 3)


def face_areas(vertices, faces):
    """The reference's float32 normalised areas."""
    vec_cross = np.cross(vertices[faces[:, 0], :] - vertices[faces[:, 2], :], vertices[faces[:, 1], :] - vertices[faces[:, 2], :])
    a = np.sqrt(np.sum(vec_cross ** 2, 1))
    return a / np.sum(a)


def ceil_counts(vertices, faces, n_samples):
    return np.ceil(n_samples * face_areas(vertices, faces)).astype(np.int64)


def counts_after_removal(ceil_c, drawn):
    c = ceil_c.copy()
    c[drawn] -= 1  # fancy indexing: each distinct drawn face loses one
    return c


def points_from_draws(vertices, faces, uvs, face_uvs, face_idx, r):
    """P = (1 - sqrt(r1)) A + sqrt(r1)(1 - r2) B + sqrt(r1) r2 C in float64, then float32; the same weights on the uv corners."""
    s = np.sqrt(r[:, 0:1])
    A, B, C = (vertices[faces[face_idx, k], :] for k in range(3))
    P = (1 - s) * A + s * (1 - r[:, 1:]) * B + s * r[:, 1:] * C
    A, B, C = (uvs[face_uvs[face_idx, k], :] for k in range(3))
    Q = (1 - s) * A + s * (1 - r[:, 1:]) * B + s * r[:, 1:] * C
    return P.astype(np.float32), Q.astype(np.float32)


def splat_taps(uv, H, W):
    """-> (sample index, label, weight float32) of every kept tap, in the reference's float32 arithmetic."""
    u = (uv[:, 0].astype(np.float32) * np.float32(W)).astype(np.float32)
    v = (np.float32(H) - uv[:, 1].astype(np.float32) * np.float32(H)).astype(np.float32)
    one = np.float32(1.0)
    taps = [(u, v), (u, v - one), (u + one, v), (u, v + one), (u - one, v)]
    idx, lab, wts = [], [], []
    n = len(uv)
    for tu, tv in taps:
        col, row = np.floor(tu), np.floor(tv)
        with np.errstate(invalid="ignore"):
            label = (row * np.float32(W) + col)
            keep = (label >= 0) & (label < H * W)
        du = (tu - col) - np.float32(0.5)
        dv = (tv - row) - np.float32(0.5)
        w = np.exp(-(du * du + dv * dv) / np.float32(2.0)).astype(np.float32)
        idx.append(np.arange(n)[keep])
        lab.append(label[keep].astype(np.int64))
        wts.append(w[keep])
    return np.concatenate(idx), np.concatenate(lab), np.concatenate(wts)


def splat_sums(uv, values, H, W):
    """fp64 sums [H*W, C + 1] (weight last) of w * values and w."""
    i, lab, w = splat_taps(uv, H, W)
    vals = np.concatenate([values.astype(np.float64), np.ones((len(values), 1))], axis=1)
    out = np.zeros((H * W, vals.shape[1]))
    np.add.at(out, lab, w.astype(np.float64)[:, None] * vals[i])
    return out


def normalise(sums):
    w = sums[:, -1].astype(np.float32)
    return sums[:, :-1].astype(np.float32) / (w[:, None] + np.float32(1e-10)), w
