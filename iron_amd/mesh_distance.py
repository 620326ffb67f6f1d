"""Point-to-mesh distance and the Chamfer metric on the HIP kernels (csrc/meshdist.hip): the
igl.point_mesh_squared_distance and cal_mesh_err of evaluation/eval_mesh.py, on the device.

Conventions (include/iron_hip.h, iron_bvh_* block): a linear BVH over the faces, built on the device (Morton keys, a device sort,
Karras' hierarchy, boxes bottom-up); one lane per query point finds the nearest face in fp32.  Ties in the fp32 distance go to the
smallest face index, so the answer does not depend on the tree, and the build and the query are bitwise reproducible.  fp64 inputs
are rounded to fp32 once on the way in.  There is no CPU path: CPU tensors are refused.
"""
from __future__ import annotations

import torch

from . import _args, _lib

WHAT = "mesh distance"  # what this module's messages begin with


class MeshBVH:
    """Linear BVH of a triangle mesh on the GPU: vertices [V, 3] (fp32; fp64 is rounded once), faces [F, 3] integer, numpy or
    CUDA tensors.  Built once at construction (one host wait, which reports a face index outside [0, V) or a non-finite
    referenced vertex as IronError); vertices no face references are ignored.  `query(points)`, `raycast(ray_o, ray_d)` and `occluded(ray_o, ray_d)` answer
    on the current stream."""

    def __init__(self, vertices, faces, device=None):
        dev = torch.device(device) if device is not None else _args.pick_device(WHAT, vertices, faces)
        if dev.type != "cuda":
            raise _lib.IronError("MeshBVH: the device must be a GPU, got %s" % dev)
        with torch.cuda.device(dev):
            self.vertices = _args.device_array(vertices, torch.float32, dev, "vertices", (3,), what=WHAT)
            self.faces = _args.face_array(faces, dev, what=WHAT)
        self.device = dev
        self.n_faces = int(self.faces.shape[0])
        if self.n_faces == 0:
            raise _lib.IronError("MeshBVH: the face list is empty")
        if self.n_faces >= (1 << 31) - 1 or self.vertices.shape[0] >= 1 << 31:
            raise _lib.IronError("MeshBVH: %d faces / %d vertices do not fit int32 indices" % (self.n_faces, self.vertices.shape[0]))
        with torch.cuda.device(dev):
            self.workspace, keys = self._keys()
            sorted_keys = self._sort(keys)
            self._hierarchy(sorted_keys)
            self._boxes(sorted_keys)

    # the four build steps, separately for tools/bench_meshdist.py
    def _keys(self):
        lib = _lib.load()
        ws = _args.sized_workspace(lib.iron_bvh_workspace_bytes, self.n_faces, device=self.device)
        keys = torch.empty((self.n_faces,), dtype=torch.int64, device=self.device)
        _lib.check(lib.iron_bvh_keys(self.vertices.data_ptr(), self.vertices.shape[0], self.faces.data_ptr(), self.n_faces, ws.data_ptr(),
                                     keys.data_ptr(), _lib.stream_ptr(self.device)))
        return ws, keys

    @staticmethod
    def _sort(keys):
        return torch.sort(keys).values  # the Morton code has its top two bits clear: signed order = unsigned order

    def _hierarchy(self, sorted_keys):
        _lib.check(_lib.load().iron_bvh_hierarchy(sorted_keys.data_ptr(), self.n_faces, self.workspace.data_ptr(),
                                                  _lib.stream_ptr(self.device)))

    def _boxes(self, sorted_keys):
        st = _lib.load().iron_bvh_boxes(self.vertices.data_ptr(), self.vertices.shape[0], self.faces.data_ptr(), self.n_faces,
                                        sorted_keys.data_ptr(), self.workspace.data_ptr(), _lib.stream_ptr(self.device))
        if st == -1:
            raise _lib.IronError("MeshBVH: a face indexes outside [0, %d) or references a non-finite vertex" % self.vertices.shape[0])
        _lib.check(st)

    def query(self, points):
        """points [N, 3] (numpy or CUDA tensor) -> (sqrD fp32 [N], I int32 [N], C fp32 [N, 3]) device tensors, in the order of
        the points: squared distance to the nearest face, its index (ties: the smallest) and the closest point on it."""
        with torch.cuda.device(self.device):
            p = _args.device_array(points, torch.float32, self.device, "points", (3,), what=WHAT)
            n = int(p.shape[0])
            sqr = torch.empty((n,), dtype=torch.float32, device=self.device)
            idx = torch.empty((n,), dtype=torch.int32, device=self.device)
            cp = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            if n:
                _lib.check(_lib.load().iron_point_mesh_distance(self.workspace.data_ptr(), self.n_faces, p.data_ptr(), n, sqr.data_ptr(),
                                                                idx.data_ptr(), cp.data_ptr(), _lib.stream_ptr(self.device)))
        return sqr, idx, cp

    def raycast(self, ray_o, ray_d, t_min=0.0, t_max=float("inf")):
        """ray_o, ray_d [N, 3] (numpy or CUDA tensors; directions need not be unit length) -> (t fp32 [N], face_idx int32 [N],
        bary fp32 [N, 2]) device tensors: the closest hit with t in (t_min, t_max] along ray_d, two-sided faces, ties in t to the
        smallest face index; bary holds the weights of the face's second and third vertex.  A miss, a non-finite ray or a zero
        direction gives (+inf, -1, 0).  Watertight across shared edges and vertices (csrc/meshrender.hip)."""
        with torch.cuda.device(self.device):
            o = _args.device_array(ray_o, torch.float32, self.device, "ray_o", (3,), what=WHAT)
            d = _args.device_array(ray_d, torch.float32, self.device, "ray_d", (3,), what=WHAT)
            n = int(o.shape[0])
            if d.shape[0] != n:
                raise _lib.IronError("ray_o has %d rows, ray_d %d" % (n, d.shape[0]))
            t = torch.empty((n,), dtype=torch.float32, device=self.device)
            idx = torch.empty((n,), dtype=torch.int32, device=self.device)
            bary = torch.empty((n, 2), dtype=torch.float32, device=self.device)
            if n:
                _lib.check(_lib.load().iron_mesh_raycast(self.workspace.data_ptr(), self.n_faces, o.data_ptr(), d.data_ptr(), n,
                                                         float(t_min), float(t_max), t.data_ptr(), idx.data_ptr(), bary.data_ptr(),
                                                         _lib.stream_ptr(self.device)))
        return t, idx, bary

    def occluded(self, ray_o, ray_d, t_min=0.0, t_max=float("inf"), skip_face=None):
        """ray_o, ray_d [N, 3] -> uint8 [N] device tensor: 1 when any face is met with t in (t_min, t_max].  skip_face [N] integer
        (optional): that face is ignored for that ray, -1 ignores none.  A non-finite ray or a zero direction gives 0.  The walk
        shares raycast's triangle and box tests and leaves at the first accepted face: the answer is exactly
        raycast(ray_o, ray_d, t_min, t_max)[1] >= 0 (csrc/envlight.hip)."""
        with torch.cuda.device(self.device):
            o = _args.device_array(ray_o, torch.float32, self.device, "ray_o", (3,), what=WHAT)
            d = _args.device_array(ray_d, torch.float32, self.device, "ray_d", (3,), what=WHAT)
            n = int(o.shape[0])
            if d.shape[0] != n:
                raise _lib.IronError("ray_o has %d rows, ray_d %d" % (n, d.shape[0]))
            skip = None
            if skip_face is not None:
                skip = _args.device_array(skip_face, torch.int32, self.device, "skip_face", (), what=WHAT)
                if skip.shape[0] != n:
                    raise _lib.IronError("ray_o has %d rows, skip_face %d" % (n, skip.shape[0]))
            occ = torch.empty((n,), dtype=torch.uint8, device=self.device)
            if n:
                _lib.check(_lib.load().iron_mesh_occluded(self.workspace.data_ptr(), self.n_faces, o.data_ptr(), d.data_ptr(), n,
                                                          float(t_min), float(t_max), _lib.ptr(skip), occ.data_ptr(),
                                                          _lib.stream_ptr(self.device)))
        return occ


def point_mesh_squared_distance(P, V, F):
    """igl.point_mesh_squared_distance(P, V, F) -> (sqrD [N], I [N], C [N, 3]).  numpy in, numpy out (float64, int64 indices);
    CUDA tensors in, tensors out on their device (sqrD and C in P's floating dtype, I int64), computed on the current stream."""
    dev = _args.pick_device(WHAT, P, V, F)
    bvh = MeshBVH(V, F, device=dev)
    sqr, idx, cp = bvh.query(P)
    if isinstance(P, torch.Tensor):
        dt = P.dtype if P.is_floating_point() else torch.float32
        return sqr.to(dt), idx.long(), cp.to(dt)
    return sqr.double().cpu().numpy(), idx.long().cpu().numpy(), cp.double().cpu().numpy()


def chamfer_distance(va, fa, vb, fb) -> float:
    """cal_mesh_err of evaluation/eval_mesh.py: 0.5 * (mean sqrt(sqrD(va -> mesh b)) + mean sqrt(sqrD(vb -> mesh a))), every
    vertex of each mesh queried against the other's surface.  The square roots and means run on the device in fp64; returns a
    Python float."""
    dev = _args.pick_device(WHAT, va, fa, vb, fb)
    with torch.cuda.device(dev):
        a = MeshBVH(va, fa, device=dev)
        b = MeshBVH(vb, fb, device=dev)
        d1 = b.query(a.vertices)[0]
        d2 = a.query(b.vertices)[0]
        ret = (torch.sqrt(d1.double()).mean() + torch.sqrt(d2.double()).mean()) * 0.5
        return float(ret.item())
