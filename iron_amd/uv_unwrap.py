"""Smart UV project and face connectivity on the HIP kernels (csrc/uvunwrap.hip): the UV layout that
models/export_uv.py gets from Blender's `bpy.ops.uv.smart_project()` at its default settings (angle limit 66 degrees, island margin
0, no area weighting, islands rotated to their smallest box and packed), restated as the contract below rather than as a copy of
Blender's code: no Blender run checks it, and bitwise agreement with Blender is not a goal.

smart_uv_project(vertices, faces) -> (uvs fp32 [T, 2], face_uvs int32 [F, 3]) on the vertices' device and the current stream:
- faces (fp32): n = (v1 - v0) x (v2 - v0) / a, a = |(v1 - v0) x (v2 - v0)|; a == 0 is degenerate (never seeds or joins a cone,
  takes projection 0).
- projection normals P: seed = the largest face (ties: smallest index); tag the untagged faces with n.seed > cos(limit / 2) and
  append the normalised sum of their normals; the untagged face with the smallest max_p n.p (ties: smallest index) seeds the next
  normal unless none is left or that value is >= cos(limit).  Every non-degenerate face then has n.p_g(f) >= cos(limit).
- g(f) = argmax_p n.p (ties: smallest p); islands = faces joined across shared edges with equal g (face_components).
- vts: the unique corner keys (island << 32 | vertex), in sorted order; a vertex on a seam gets one vt per island.
- a vt's 2-D point is (x.t, x.b) in the right-handed basis (t, b, p) of its island's normal (t = normalize(e x p), e the axis of
  the smallest |p_i|, ties: lowest i): every non-degenerate face maps with positive orientation.
- per island the rotation of the smallest box area among k * 1 degree (k = 0..89), then theta* + j * 0.05 degrees (j = -20..20),
  ties to the smaller angle; a box higher than wide is turned by +90 degrees.
- pack_boxes (host): shelf packing by descending height for a few strip widths, one global scale s (uniform texel density), boxes
  pairwise >= island_margin apart and >= island_margin / 2 from the border of [0, 1]^2.
- UV area of face f = s^2 * (a_f / 2) * (n_f . p_g(f)).  The output is bitwise reproducible.

There is no CPU path: CPU tensors are refused (numpy inputs go to the current device).
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np
import torch

from . import _args, _lib

WHAT = "mesh distance"  # what the argument messages of this module begin with: it shares mesh_distance's input rules

COARSE_STEP_DEG, COARSE_N = 1.0, 90
FINE_STEP_DEG, FINE_HALF = 0.05, 20
MAX_ROUNDS = 64  # hook / jump rounds of the union-find; pointer jumping makes a round at least halve every path


def _state(dev):
    return torch.zeros((2,), dtype=torch.int64, device=dev)  # 16 bytes: argmin word, bad flag, changed word


def _bad(n_verts):
    return _lib.IronError("a face indexes outside [0, %d) or references a non-finite vertex" % n_verts)


def edge_records(v: torch.Tensor, f: torch.Tensor, state: torch.Tensor):
    """-> (sorted_keys int64 [3F], perm int64 [3F]): the edge records of iron_mesh_edge_keys sorted on the device."""
    keys = torch.empty((3 * f.shape[0],), dtype=torch.int64, device=f.device)
    _lib.check(_lib.load().iron_mesh_edge_keys(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], keys.data_ptr(), state.data_ptr(),
                                               _lib.stream_ptr(f.device)))
    return torch.sort(keys, stable=True)  # the sentinel 2^63 - 1 (degenerate edges, bad faces) sorts last


def _components(sorted_keys, perm, group, n_faces, n_verts, state):
    """-> (labels int32 [F] = rank of the component's smallest face index, K, rounds)."""
    dev = sorted_keys.device
    parent = torch.empty((n_faces,), dtype=torch.int32, device=dev)
    rounds = C.c_int32(0)
    st = _lib.load().iron_mesh_components(sorted_keys.data_ptr(), perm.data_ptr(), sorted_keys.shape[0], _lib.ptr(group), n_faces,
                                          parent.data_ptr(), state.data_ptr(), MAX_ROUNDS, C.byref(rounds), _lib.stream_ptr(dev))
    if st == -1:
        raise _bad(n_verts)
    if st == _lib.IRON_ERR_RANGE:
        raise _lib.IronError("face components did not converge in %d rounds" % MAX_ROUNDS)
    _lib.check(st)
    is_root = parent == torch.arange(n_faces, dtype=torch.int32, device=dev)
    rank = torch.cumsum(is_root.to(torch.int32), 0, dtype=torch.int32) - 1
    labels = rank[parent.long()]
    return labels, int(rank[-1].item()) + 1, int(rounds.value)


def face_components(vertices, faces, group=None):
    """Connected components of the faces over shared edges (faces sharing only a vertex are not joined, nor through an edge whose two
    indices are equal); with `group` [F] only faces of equal group are joined.  -> (labels int32 [F] on the device, numbered 0..K-1
    in order of each component's first face, K).  A face index outside [0, V) or a non-finite referenced vertex raises IronError."""
    dev = _args.pick_device(WHAT, vertices, faces)
    with torch.cuda.device(dev):
        v = _args.device_array(vertices, torch.float32, dev, "vertices", (3,), what=WHAT)
        f = _args.face_array(faces, dev, what=WHAT)
        n = int(f.shape[0])
        if n == 0:
            return torch.zeros((0,), dtype=torch.int32, device=dev), 0
        if n >= (1 << 31) - 1 or v.shape[0] >= 1 << 31:
            raise _lib.IronError("face_components: %d faces / %d vertices do not fit int32 indices" % (n, v.shape[0]))
        g = None
        if group is not None:
            g = torch.as_tensor(group).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            if g.shape[0] != n:
                raise _lib.IronError("group must have one entry per face")
        state = _state(dev)
        keys, perm = edge_records(v, f, state)
        labels, k, _ = _components(keys, perm, g, n, int(v.shape[0]), state)
        return labels, k


def coarse_table() -> np.ndarray:
    """[90, 2] fp32 (cos, sin) of k * 1 degree."""
    r = np.radians(np.arange(COARSE_N, dtype=np.float64) * COARSE_STEP_DEG)
    return np.stack([np.cos(r), np.sin(r)], -1).astype(np.float32)


def fine_table(coarse_idx) -> np.ndarray:
    """[K, 41, 2] fp32 (cos, sin) of coarse_idx * 1 degree + j * 0.05 degree, j = -20..20."""
    deg = np.asarray(coarse_idx, dtype=np.float64)[:, None] * COARSE_STEP_DEG + np.arange(-FINE_HALF, FINE_HALF + 1) * FINE_STEP_DEG
    r = np.radians(deg)
    return np.stack([np.cos(r), np.sin(r)], -1).astype(np.float32)


PACK_WIDTHS = (0.7, 0.85, 1.0, 1.15, 1.3, 1.5, 2.0)  # candidate strip widths, in units of sqrt(sum of box areas)


def pack_boxes(w, h, margin=0.0):
    """Shelf packing of K boxes (world units, w >= h expected) into [0, 1]^2 with ONE scale s for all: boxes by descending height
    (ties: index), rows filled left to right up to a strip width, for each width of PACK_WIDTHS; the width with the largest s wins
    (ties: the first).  -> (lower-left corners [K, 2] float64 in UV units, s).  Boxes are pairwise >= margin apart and >= margin / 2
    from the border; IronError when no width can meet the margin."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    K, m = len(w), float(margin)
    if K == 0:
        return np.zeros((0, 2)), 1.0
    if not (0.0 <= m < 1.0):
        raise _lib.IronError("island_margin must lie in [0, 1), got %r" % margin)
    order = np.lexsort((np.arange(K), -h))
    base = math.sqrt(float((w * h).sum()))
    widths = sorted({max(float(w.max()), base * c) for c in PACK_WIDTHS})
    best = None
    for W in widths:
        x = np.empty(K)
        col = np.empty(K, dtype=np.int64)
        row = np.empty(K, dtype=np.int64)
        row_w, row_n, row_h = [], [], []
        cx, j = 0.0, 0
        for i in order:
            if not row_h or (j > 0 and cx + w[i] > W):
                row_h.append(h[i]); row_w.append(0.0); row_n.append(0)
                cx, j = 0.0, 0
            x[i], col[i], row[i] = cx, j, len(row_h) - 1
            cx += w[i]; j += 1
            row_w[-1], row_n[-1] = cx, j
        rw, rn, rh = np.asarray(row_w), np.asarray(row_n), np.asarray(row_h)
        num_w, num_h = 1.0 - rn * m, 1.0 - len(rh) * m
        if (num_w <= 0.0).any() or num_h <= 0.0:
            continue
        lim = [num_w[rw > 0] / rw[rw > 0]]
        if rh.sum() > 0:
            lim.append(np.array([num_h / rh.sum()]))
        lim = np.concatenate(lim)
        s = float(lim.min()) if len(lim) else 1.0
        if best is None or s > best[0]:
            best = (s, x, col, row, rh)
    if best is None:
        raise _lib.IronError("island_margin %g cannot be met with %d islands (a shelf layout needs margin < 1 / rows)" % (m, K))
    s, x, col, row, rh = best
    s *= 1.0 - 2.0 ** -20  # keeps fp32 rounding of the apply inside [0, 1]
    ycum = np.concatenate([[0.0], np.cumsum(rh)])[:-1]
    off = np.stack([0.5 * m + s * x + col * m, 0.5 * m + s * ycum[row] + row * m], -1)
    return off, s


def _ord_to_float(w: torch.Tensor) -> torch.Tensor:
    """The order-preserving uint32 encoding of fp32 (stored as int32) back to fp32."""
    u = w.to(torch.int64) & 0xFFFFFFFF
    neg = (u & 0x80000000) == 0  # a negative float was stored inverted
    bits = torch.where(neg, (~u) & 0xFFFFFFFF, u & 0x7FFFFFFF)
    return _bits_to_f32(bits)


def _bits_to_f32(bits: torch.Tensor) -> torch.Tensor:
    b = bits - ((bits >> 31) << 32)  # two's complement int32 value of the low 32 bits
    return b.to(torch.int32).view(torch.float32)


class _Stages:
    """Per-stage wall time (device synchronised) into `stats` when the caller asks for it; free otherwise."""

    def __init__(self, stats, dev):
        self.stats, self.dev = stats, dev
        if stats is not None:
            torch.cuda.synchronize(dev)
            self.t = time.perf_counter()

    def __call__(self, name):
        if self.stats is None:
            return
        torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        self.stats[name + "_ms"] = (now - self.t) * 1e3
        self.t = now


def smart_uv_project(vertices, faces, angle_limit=66.0, island_margin=0.0, stats=None):
    """vertices [V, 3], faces [F, 3] (CUDA tensors or numpy) -> (uvs fp32 [T, 2], face_uvs int32 [F, 3]) on the vertices' device,
    computed on the current stream (the module docstring states the algorithm).  Vertices and faces are not modified.  `stats`
    (a dict, optional) receives per-stage times and counts for tools/bench_uv.py (the stage timers synchronise the device)."""
    dev = _args.pick_device(WHAT, vertices, faces)
    if not (0.0 < float(angle_limit) < 90.0):
        raise _lib.IronError("angle_limit must lie in (0, 90) degrees, got %r" % angle_limit)
    with torch.cuda.device(dev):
        v = _args.device_array(vertices, torch.float32, dev, "vertices", (3,), what=WHAT)
        f = _args.face_array(faces, dev, what=WHAT)
        F, V = int(f.shape[0]), int(v.shape[0])
        if F == 0:
            return torch.zeros((0, 2), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
        if F >= (1 << 31) - 1 or V >= 1 << 31 or 3 * F >= 1 << 31:
            raise _lib.IronError("smart_uv_project: %d faces / %d vertices do not fit int32 indices" % (F, V))
        lib, sp = _lib.load(), _lib.stream_ptr(dev)
        tick = _Stages(stats, dev)

        # projection normals and the assignment g(f)
        alpha = math.radians(float(angle_limit))
        max_p = min(F, int(math.ceil(2.0 / (1.0 - math.cos(alpha / 4.0)))) + 1)  # seeds lie > limit/2 apart: a cap-packing bound
        ws = _args.sized_workspace(lib.iron_uv_workspace_bytes, F, device=dev)
        state = _state(dev)
        P = torch.empty((max_p, 3), dtype=torch.float32, device=dev)
        group = torch.empty((F,), dtype=torch.int32, device=dev)
        n_p, n_w = C.c_int32(0), C.c_int32(0)
        st = lib.iron_uv_projections(v.data_ptr(), V, f.data_ptr(), F, math.cos(alpha / 2.0), math.cos(alpha), max_p, ws.data_ptr(),
                                     state.data_ptr(), None, P.data_ptr(), group.data_ptr(), C.byref(n_p), C.byref(n_w), sp)
        if st == -1:
            raise _bad(V)
        if st == _lib.IRON_ERR_RANGE:
            raise _lib.IronError("smart_uv_project: more than %d projection normals" % max_p)
        _lib.check(st)
        del ws
        P = P[:n_p.value]
        tick("geometry_selection")

        # islands
        keys, perm = edge_records(v, f, state)
        tick("edge_sort")
        labels, K, rounds = _components(keys, perm, group, F, V, state)
        del keys, perm
        tick("component_rounds")

        # vts: unique (island, vertex) corner keys
        corner = ((labels.long()[:, None] << 32) | f.long()).reshape(-1)
        uniq, inv = torch.unique(corner, sorted=True, return_inverse=True)
        T = int(uniq.shape[0])
        vt_vertex = (uniq & 0xFFFFFFFF).to(torch.int32)
        vt_island = (uniq >> 32).to(torch.int32)
        face_uvs = inv.reshape(F, 3).to(torch.int32)
        island_group = torch.empty((K,), dtype=torch.int32, device=dev)
        island_group[labels.long()] = group  # every face of an island carries the island's group
        xy = torch.empty((T, 2), dtype=torch.float32, device=dev)
        _lib.check(lib.iron_uv_project(v.data_ptr(), vt_vertex.data_ptr(), vt_island.data_ptr(), T, island_group.data_ptr(), P.data_ptr(),
                                       xy.data_ptr(), sp))
        tick("vt_unique")

        # rotation: coarse then fine angle sets, smallest box area
        def search(cs, n_angles, per_island):
            boxes = torch.empty((K, n_angles, 4), dtype=torch.int32, device=dev)
            _lib.check(lib.iron_uv_rotation_search(xy.data_ptr(), vt_island.data_ptr(), T, K, cs.data_ptr(), n_angles, per_island,
                                                   boxes.data_ptr(), sp))
            b = _ord_to_float(boxes)  # -min x, -min y, max x, max y
            lo, hi = -b[..., :2], b[..., 2:]
            area = (hi[..., 0] - lo[..., 0]) * (hi[..., 1] - lo[..., 1])
            idx = torch.argmin(area, dim=1)  # the first minimum: ties go to the smaller angle
            sel = torch.arange(K, device=dev)
            return idx.cpu().numpy(), torch.cat([lo[sel, idx], hi[sel, idx]], 1).cpu().numpy()

        coarse, _ = search(torch.from_numpy(coarse_table()).to(dev), COARSE_N, 0)
        fine = fine_table(coarse)
        fidx, box = search(torch.from_numpy(fine).to(dev), 2 * FINE_HALF + 1, 1)
        tick("rotation_search")

        # packing (host)
        bw, bh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]  # fp32, as the search computed them
        swap = bh > bw
        off, s = pack_boxes(np.where(swap, bh, bw), np.where(swap, bw, bh), island_margin)
        cs = fine[np.arange(K), fidx]
        params = np.concatenate([cs, box, off / s], axis=1).astype(np.float32)
        tick("host_packing")

        uv = torch.empty((T, 2), dtype=torch.float32, device=dev)
        params_d = torch.from_numpy(params).to(dev)  # named: a temporary would go back to the allocator before the launch
        swap_d = torch.from_numpy(swap.astype(np.int32)).to(dev)
        _lib.check(lib.iron_uv_apply(xy.data_ptr(), vt_island.data_ptr(), T, params_d.data_ptr(), swap_d.data_ptr(), float(np.float32(s)),
                                     uv.data_ptr(), sp))
        tick("apply")
        if stats is not None:
            stats.update(n_normals=int(n_p.value), n_islands=K, n_vts=T, component_rounds=rounds,
                         host_waits=int(n_w.value) + rounds + 4,  # + K, the unique's size, the two angle picks
                         packing_efficiency=float((bw.astype(np.float64) * bh).sum() * s * s), scale=float(s))
        return uv, face_uvs
