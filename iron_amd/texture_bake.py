"""Material texture baking on the HIP kernels (csrc/texbake.hip): the surface sampling, Gaussian splat and
normalisation of models/export_materials.py, on device tensors.

Conventions (include/iron_hip.h, iron_bake_* block): per-face sample counts follow the reference's fp32 rule, the excess is
removed by draws with replacement from an in-kernel Philox generator keyed by (seed, round, index), samples come out ordered by
face.  The splat accumulates in int64 units of 2^-24, so a bake is bitwise reproducible.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _args, _lib

SCALE = float(1 << 24)   # fixed-point units per 1.0 in the splat accumulator
MAX_CHANNELS = 16        # splatted channels per sample (xyz + values), the weight comes on top


def _mesh(vertices, faces, uvs, face_uvs, dev):
    v = _args.device_array(vertices, torch.float32, dev, "vertices", (3,), strict=False)
    f = _args.device_array(faces, torch.int32, dev, "faces", (3,), strict=False)
    t = _args.device_array(uvs, torch.float32, dev, "uvs", (2,), strict=False)
    ft = _args.device_array(face_uvs, torch.int32, dev, "face_uvs", (3,), strict=False)
    if ft.shape[0] != f.shape[0]:
        raise _lib.IronError("face_uvs has %d rows, faces %d" % (ft.shape[0], f.shape[0]))
    return v, f, t, ft


def _count(v, f, ft, n_uvs, n_samples, seed, round, ceil_counts=None, counts=None):
    """iron_bake_count: per-face counts and their offsets in a call-scoped workspace -> (workspace, total).  Waits once."""
    lib = _lib.load()
    ws = _args.sized_workspace(lib.iron_bake_workspace_bytes, f.shape[0], device=v.device)
    total = C.c_int64(0)
    st = lib.iron_bake_count(v.data_ptr(), v.shape[0], f.data_ptr(), n_uvs, ft.data_ptr(), f.shape[0], int(n_samples),
                             int(seed) & ((1 << 64) - 1), int(round) & 0xFFFFFFFF, ws.data_ptr(), _lib.ptr(ceil_counts),
                             _lib.ptr(counts), C.byref(total), _lib.stream_ptr(v.device))
    if st == _lib.IRON_ERR_RANGE:
        raise _lib.IronError("sample_surface_gpu: n_samples = %d is above 2^24, where the fp32 count rule is not exact" % n_samples)
    if st == -1:
        raise _lib.IronError("sample_surface_gpu: a face indexes outside the vertices or uvs (or a bad argument)")
    _lib.check(st)
    return ws, int(total.value)


def _sample(v, f, t, ft, ws, total, seed, round, face_idx=False):
    lib = _lib.load()
    pts = torch.empty((total, 3), dtype=torch.float32, device=v.device)
    uv = torch.empty((total, 2), dtype=torch.float32, device=v.device)
    fi = torch.empty((total,), dtype=torch.int32, device=v.device) if face_idx else None
    _lib.check(lib.iron_bake_sample(v.data_ptr(), f.data_ptr(), t.data_ptr(), ft.data_ptr(), f.shape[0], int(seed) & ((1 << 64) - 1),
                                    int(round) & 0xFFFFFFFF, ws.data_ptr(), total, pts.data_ptr(), uv.data_ptr(), _lib.ptr(fi),
                                    _lib.stream_ptr(v.device)))
    return pts, uv, fi


def sample_surface_gpu(vertices, faces, uvs, face_uvs, n_samples, seed, round=0, return_face_idx=False, return_counts=False):
    """models/export_materials.py:13-55 on the device: -> (points fp32 [N,3], uv fp32 [N,2]) with N = sum of the per-face counts
    (N >= n_samples, like the reference), ordered by face.  `return_face_idx` appends int32 [N]; `return_counts` appends the
    int32 [F] counts before and after the excess removal.  Mesh arrays may be numpy or tensors; fp32 / int32 on the GPU."""
    dev = _args.pick_device("texture bake", vertices, faces, uvs, face_uvs, strict=False)
    n_samples = int(n_samples)
    if n_samples < 0:
        raise _lib.IronError("n_samples must be >= 0")
    with torch.cuda.device(dev):
        v, f, t, ft = _mesh(vertices, faces, uvs, face_uvs, dev)
        ceil_c = torch.empty((f.shape[0],), dtype=torch.int32, device=dev) if return_counts else None
        cnt = torch.empty_like(ceil_c) if return_counts else None
        if f.shape[0] == 0:
            ws, total = None, 0
        else:
            ws, total = _count(v, f, ft, t.shape[0], n_samples, seed, round, ceil_c, cnt)
        if total:
            pts, uv, fi = _sample(v, f, t, ft, ws, total, seed, round, return_face_idx)
        else:
            pts = torch.empty((0, 3), dtype=torch.float32, device=dev)
            uv = torch.empty((0, 2), dtype=torch.float32, device=dev)
            fi = torch.empty((0,), dtype=torch.int32, device=dev)
    out = (pts, uv)
    if return_face_idx:
        out += (fi,)
    if return_counts:
        out += (ceil_c, cnt)
    return out


def sample_surface_explicit(vertices, faces, uvs, face_uvs, face_idx, r1, r2):
    """The point rule of sample_surface for caller-given draws: face_idx [N], r1 / r2 fp64 [N] (the reference's np.random.rand
    columns) -> (points fp32 [N,3], uv fp32 [N,2]); a sample with an out-of-range face comes out NaN."""
    dev = _args.pick_device("texture bake", vertices, faces, uvs, face_uvs, face_idx, r1, r2, strict=False)
    with torch.cuda.device(dev):
        v, f, t, ft = _mesh(vertices, faces, uvs, face_uvs, dev)
        fi = torch.as_tensor(face_idx).detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        a = torch.as_tensor(r1).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        b = torch.as_tensor(r2).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        n = fi.shape[0]
        if a.shape[0] != n or b.shape[0] != n:
            raise _lib.IronError("face_idx, r1 and r2 must have the same length")
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().iron_bake_sample_explicit(v.data_ptr(), v.shape[0], f.data_ptr(), t.data_ptr(), t.shape[0], ft.data_ptr(),
                                                         f.shape[0], fi.data_ptr(), a.data_ptr(), b.data_ptr(), n, pts.data_ptr(),
                                                         uv.data_ptr(), _lib.stream_ptr(dev)))
    return pts, uv


class SplatAccumulator:
    """accumulate_splat_material (models/export_materials.py:77-140) into device images: `add(points, uvs, values)` splats
    w * xyz, w * values and w; `resolve()` returns (xyz [H,W,3], values [H,W,C], weight [H,W]) normalised like export_materials
    (acc / (w + 1e-10)).  The sums are int64 in 2^-24 units (bitwise reproducible); `max_samples` bounds the samples of all
    add() calls, and a term whose size could overflow that budget, or that is not finite, makes resolve() raise IronError."""

    def __init__(self, texture_H, texture_W, n_values=7, max_samples=1 << 28, device=None):
        self.H, self.W, self.n_values = int(texture_H), int(texture_W), int(n_values)
        if self.H <= 0 or self.W <= 0 or self.H * self.W > 1 << 24:
            raise _lib.IronError("texture size %dx%d: H*W must be in [1, 2^24]" % (self.H, self.W))
        if not 0 <= self.n_values <= MAX_CHANNELS - 3:
            raise _lib.IronError("n_values must be in [0, %d]" % (MAX_CHANNELS - 3))
        self.max_samples = int(max_samples)
        if self.max_samples <= 0:
            raise _lib.IronError("max_samples must be positive")
        # every texel receives at most 5 taps per sample: 5 * max_samples * term_bound <= 2^62
        self.term_bound = (1 << 62) // (5 * self.max_samples)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.acc = torch.zeros((self.H * self.W, 3 + self.n_values + 1), dtype=torch.int64, device=self.device)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.n_added = 0

    def add(self, points, uvs, values):
        dev = self.device
        p = _args.device_array(points, torch.float32, dev, "points", (3,), strict=False)
        uv = _args.device_array(uvs, torch.float32, dev, "uvs", (2,), strict=False)
        val = _args.device_array(values, torch.float32, dev, "values", (self.n_values,), strict=False)
        n = p.shape[0]
        if uv.shape[0] != n or val.shape[0] != n:
            raise _lib.IronError("points, uvs and values must have the same number of rows")
        if self.n_added + n > self.max_samples:
            raise _lib.IronError("SplatAccumulator: %d samples exceed max_samples = %d" % (self.n_added + n, self.max_samples))
        self.n_added += n
        with torch.cuda.device(dev):
            _lib.check(_lib.load().iron_bake_splat(uv.data_ptr(), p.data_ptr(), 3, val.data_ptr(), self.n_values, n, self.H, self.W,
                                                   self.term_bound, self.acc.data_ptr(), self.flag.data_ptr(), _lib.stream_ptr(dev)))
        return self

    def sums(self):
        """The raw accumulated sums in fp64, [H, W, 3 + C + 1] (the weight last)."""
        return (self.acc.double() / SCALE).reshape(self.H, self.W, -1)

    def resolve(self):
        c = 3 + self.n_values
        out = torch.empty((self.H, self.W, c), dtype=torch.float32, device=self.device)
        weight = torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            st = _lib.load().iron_bake_resolve(self.acc.data_ptr(), c, self.H, self.W, self.flag.data_ptr(), out.data_ptr(),
                                               weight.data_ptr(), _lib.stream_ptr(self.device))
        if st == _lib.IRON_ERR_RANGE:
            raise _lib.IronError("texture bake: a splatted value is not finite or too large for the int64 accumulator "
                                 "(|value| above %.3g for %d samples)" % (self.term_bound / SCALE, self.max_samples))
        _lib.check(st)
        return out[..., :3], out[..., 3:], weight


def bake_materials(vertices, faces, uvs, face_uvs, material_predictor, texture_H=2048, texture_W=2048, n_rounds=5,
                   n_samples=5_000_000, max_num_pts=320000, seed=0):
    """export_materials' bake (models/export_materials.py:169-207) on the device: n_rounds of sample_surface(n_samples), the
    material query in splits of max_num_pts (rendering_func.query_materials; predictors returning CPU tensors are accepted),
    the splat, then the normalisation.  -> (xyz [H,W,3], material [H,W,7], weight [H,W]) device fp32 tensors."""
    from .rendering_func import query_materials
    dev = _args.pick_device("texture bake", vertices, faces, uvs, face_uvs, strict=False)
    with torch.cuda.device(dev):
        v, f, t, ft = _mesh(vertices, faces, uvs, face_uvs, dev)
        acc = SplatAccumulator(texture_H, texture_W, 7, max_samples=max(1, int(n_rounds) * (int(n_samples) + f.shape[0])), device=dev)
        for r in range(int(n_rounds)):
            pts, uv = sample_surface_gpu(v, f, t, ft, n_samples, seed, round=r)
            if pts.shape[0] == 0:
                continue
            mat = query_materials(material_predictor, pts, max_num_pts)
            acc.add(pts, uv, mat)
            del pts, uv, mat
        return acc.resolve()
