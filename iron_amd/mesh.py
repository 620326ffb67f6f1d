"""Mesh extraction on the HIP kernels: marching cubes over a device-resident field (csrc/mcubes.hip) and the lattice query of
models/renderer.py:34-42 without the host round trip.

Conventions (include/iron_hip.h, iron_amd/mc_table.py): `u` is [nx, ny, nz] in extract_fields' 'ij' order (z fastest); a
corner is above when u > threshold (NaN: below); one vertex per crossed lattice edge, in index coordinates, ordered by (lattice
point, axis); triangles ordered by (cell, table order), right-hand normals from u > threshold toward u < threshold.  The output
is bitwise deterministic.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _args, _lib


def marching_cubes(u: torch.Tensor, threshold: float = 0.0):
    """u float32 [nx, ny, nz] on the GPU -> (verts float32 [V, 3] in index coordinates, tris int64 [T, 3]) on u's device, computed
    on the current stream.  Waits for the stream once, to learn the output sizes."""
    if not isinstance(u, torch.Tensor):
        raise _lib.IronError("marching_cubes expects a torch.Tensor")
    u = _lib.require_cuda_f32(u.detach(), "u")
    if u.dim() != 3:
        raise _lib.IronError("marching_cubes expects u of shape [nx, ny, nz], got %s" % (tuple(u.shape),))
    dev = u.device
    nx, ny, nz = (int(s) for s in u.shape)
    if max(nx, ny, nz) >= 1 << 31:
        raise _lib.IronError("marching_cubes: dims must fit int32, got %s" % (tuple(u.shape),))
    verts = torch.empty((0, 3), dtype=torch.float32, device=dev)
    tris = torch.empty((0, 3), dtype=torch.int64, device=dev)
    if min(nx, ny, nz) < 2:
        return verts, tris
    lib = _lib.load()
    thr = float(threshold)
    with torch.cuda.device(dev):
        # call-scoped and released afterwards: at 512^3 it is ~0.8 GB, too much to keep cached between rare calls
        ws = _args.sized_workspace(lib.iron_mc_workspace_bytes, nx, ny, nz, device=dev)
        nv, nt = C.c_int64(0), C.c_int64(0)
        st = lib.iron_mc_count(u.data_ptr(), nx, ny, nz, thr, ws.data_ptr(), C.byref(nv), C.byref(nt), _lib.stream_ptr(dev))
        if st == _lib.IRON_ERR_RANGE:
            raise _lib.IronError("marching_cubes: the mesh of a %dx%dx%d field has 2^31 or more vertices or triangles" % (nx, ny, nz))
        _lib.check(st)
        if nt.value == 0:
            return verts, tris
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        tris32 = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        _lib.check(lib.iron_mc_emit(u.data_ptr(), nx, ny, nz, thr, ws.data_ptr(), verts.data_ptr(), tris32.data_ptr(),
                                    _lib.stream_ptr(dev)))
        tris = tris32.long()
    return verts, tris


def extract_fields_gpu(bound_min, bound_max, resolution, query_func, max_points: int = 1 << 22) -> torch.Tensor:
    """The lattice and query of renderer.extract_fields (models/renderer.py:9-31), kept on the device: float32 [res, res, res]
    on the current device, evaluated in x-slabs of at most `max_points` points."""
    dev = torch.device("cuda", torch.cuda.current_device())
    res = int(resolution)
    axes = [torch.linspace(float(bound_min[i]), float(bound_max[i]), res).to(dev) for i in range(3)]
    u = torch.empty((res, res, res), dtype=torch.float32, device=dev)
    slab = max(1, min(res, max_points // (res * res)))
    lib = _lib.load()
    with torch.no_grad(), torch.cuda.device(dev):
        pts = torch.empty((slab * res * res, 3), dtype=torch.float32, device=dev)
        for x0 in range(0, res, slab):
            nx = min(slab, res - x0)
            p = pts[:nx * res * res]
            _lib.check(lib.iron_grid_points(axes[0][x0:x0 + nx].data_ptr(), axes[1].data_ptr(), axes[2].data_ptr(), nx, res, res,
                                            p.data_ptr(), _lib.stream_ptr(dev)))
            u[x0:x0 + nx] = query_func(p).detach().reshape(nx, res, res)
    return u


def extract_geometry_gpu(bound_min, bound_max, resolution, threshold, query_func):
    """models/renderer.py:34-42 on the device: query_func over the resolution^3 lattice (extract_fields_gpu), marching cubes,
    then the reference's scaling v / (res - 1) * (max - min) + min.  Returns (verts float64 [V, 3] in world coordinates,
    tris int64 [T, 3]) on the current device; float64 like the reference's vertices."""
    u = extract_fields_gpu(bound_min, bound_max, resolution, query_func)
    verts, tris = marching_cubes(u, threshold)
    del u
    b_min = torch.as_tensor(bound_min).detach().to(device=verts.device, dtype=torch.float64).reshape(1, 3)
    b_max = torch.as_tensor(bound_max).detach().to(device=verts.device, dtype=torch.float64).reshape(1, 3)
    verts = verts.double() / (int(resolution) - 1.0) * (b_max - b_min) + b_min
    return verts, tris
