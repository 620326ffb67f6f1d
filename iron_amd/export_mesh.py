"""Drop-in for models/export_mesh.py (the stage-2 mesh export of render_surface.py, `export_mesh_and_materials`): the same public
names and signatures, without skimage or trimesh.  install_as_models() registers it as models.export_mesh.

export_mesh(sdf, path): the SDF on a uniform 100^3 lattice of [-1, 1]^3, marching cubes, the largest connected component by area
sets a frame (its mean and principal axes), then the SDF on a lattice aligned with that frame whose shortest axis has `resolution`
samples, marching cubes again, and the whole extraction rotated back to world coordinates is written as an OBJ (`v` and `f` lines).
No file is written when the aligned field has no sign change.  SDF values come from calls of at most `max_n_pts` points on the
device; lattices, marching cubes (iron_amd.mesh.marching_cubes) and components (iron_amd.uv_unwrap.face_components) stay there.

Conventions and deviations from the reference, on purpose:
- Lattices: the reference's numpy axes (np.linspace / np.arange, spacing taken from the x axis for all three), but the field is
  evaluated directly in [nx, ny, nz] order, which is the reference's (ny, nx, nz) volume after its transpose.
- Winding: marching_cubes' own -- right-hand normals point from sdf > 0 toward sdf < 0, i.e. into the surface of an SDF that is
  positive outside.
- Largest component: faces joined across shared edges, areas summed in fp64 in face order, the first maximum on ties.
- Frame: the eigenvectors (as rows, ascending eigenvalues, torch.linalg.eigh) of the exact area-weighted second moment of the
  component's triangles, each row signed so that its largest-magnitude entry (the first on ties) is positive; then, as in the
  reference, rows 1 and 2 are swapped when the determinant is negative.  The reference samples 10 000 random surface points and
  uses the removed torch.eig; here the frame is a function of the mesh and the output is deterministic.  The aligned lattice spans
  the component's vertices in that frame (the reference: its samples).
- export_mesh_no_translation keeps its quirk: the first-stage vertices are not translated to the lattice origin.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .mesh import marching_cubes
from .uv_unwrap import face_components


def _cuda():
    if not torch.cuda.is_available():
        raise _lib.IronError("export_mesh needs a GPU (iron_amd has no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def _meshgrid_points(x, y, z, dev):
    xx, yy, zz = np.meshgrid(x, y, z)
    return torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float).to(dev)


def get_grid_uniform(resolution):
    """models/export_mesh.py's uniform lattice of [-1, 1]^3: grid_points [res^3, 3] on the GPU in np.meshgrid's (y, x, z) order."""
    x = np.linspace(-1.0, 1.0, resolution)
    return {"grid_points": _meshgrid_points(x, x, x, _cuda()), "shortest_axis_length": 2.0, "xyz": [x, x, x], "shortest_axis_index": 0}


def _aligned_axes(points, resolution, eps):
    lo = torch.min(points, dim=0)[0].squeeze().numpy()
    hi = torch.max(points, dim=0)[0].squeeze().numpy()
    s = int(np.argmin(hi - lo))
    short = np.linspace(lo[s] - eps, hi[s] + eps, resolution)
    length = np.max(short) - np.min(short)
    step = length / (short.shape[0] - 1)
    axes = [short if i == s else np.arange(lo[i] - eps, hi[i] + step + eps, step) for i in range(3)]
    return axes, length, s


def get_grid(points, resolution, eps=0.1):
    """models/export_mesh.py's aligned lattice around `points` [N, 3] (CPU): the shortest side of their box gets `resolution`
    samples over [min - eps, max + eps], the others np.arange with the same step; grid_points on the GPU in (y, x, z) order."""
    axes, length, s = _aligned_axes(points, resolution, eps)
    return {"grid_points": _meshgrid_points(axes[0], axes[1], axes[2], _cuda()), "shortest_axis_length": length, "xyz": axes,
            "shortest_axis_index": s}


def _field(sdf, axes, max_n_pts, dev, frame=None, origin=None):
    """sdf over the lattice axes x, y, z in [nx, ny, nz] order (z fastest) -> float32 device tensor; with `frame` (3x3 rows) and
    `origin` the lattice point p is evaluated at p @ frame + origin (world = frame^T p + origin)."""
    nx, ny, nz = (len(a) for a in axes)
    ax = [torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev) for a in axes]
    u = torch.empty((nx * ny * nz,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    slab = max(1, min(nx, (1 << 24) // max(1, ny * nz)))
    with torch.no_grad():
        pts = torch.empty((slab * ny * nz, 3), dtype=torch.float32, device=dev)
        for x0 in range(0, nx, slab):
            n = min(slab, nx - x0)
            p = pts[:n * ny * nz]
            _lib.check(lib.iron_grid_points(ax[0][x0:].data_ptr(), ax[1].data_ptr(), ax[2].data_ptr(), n, ny, nz, p.data_ptr(),
                                            _lib.stream_ptr(dev)))
            if frame is not None:
                p = p @ frame + origin
            base = x0 * ny * nz
            for i in range(0, p.shape[0], max_n_pts):
                q = p[i:i + max_n_pts]
                u[base + i:base + i + q.shape[0]] = sdf(q).detach().reshape(-1).float()
    return u.reshape(nx, ny, nz)


def _triangle_areas(v, f):
    t = v[f]
    return 0.5 * torch.linalg.norm(torch.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=1), dim=1)


def _largest_component(verts, tris):
    labels, k = face_components(verts, tris)
    area = _triangle_areas(verts.double(), tris).cpu().numpy()
    comp = np.bincount(labels.cpu().numpy(), weights=area, minlength=k)  # fp64, face order
    keep = torch.from_numpy(np.flatnonzero(labels.cpu().numpy() == int(np.argmax(comp)))).to(tris.device)
    return tris[keep]


def _frame(verts, tris):
    """(mean [3], rows [3, 3]) of the exact area-weighted second moment of the triangles (fp64)."""
    t = verts.double()[tris]
    a = _triangle_areas(verts.double(), tris)
    A = a.sum()
    s = t.sum(dim=1)
    mean = (a[:, None] * s).sum(0) / (3.0 * A)
    # E[x x^T] over a triangle = (a a^T + b b^T + c c^T + s s^T) / 12
    second = (torch.einsum("f,fki,fkj->ij", a, t, t) + torch.einsum("f,fi,fj->ij", a, s, s)) / (12.0 * A)
    cov = second - torch.outer(mean, mean)
    _, vecs = torch.linalg.eigh(cov)
    rows = vecs.T.contiguous()
    big = torch.argmax(rows.abs(), dim=1)
    sign = torch.sign(rows[torch.arange(3, device=rows.device), big])
    rows = rows * sign[:, None]
    if torch.det(rows) < 0:
        rows = rows[[0, 2, 1]]
    return mean, rows


def _write_obj_vf(path, vertices, faces):
    with open(path, "w") as fp:
        fp.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in np.asarray(vertices, dtype=np.float32).astype(np.float64))
        fp.writelines("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in np.asarray(faces))


def _export(sdf, mesh_fpath, resolution, max_n_pts, translate_first):
    assert mesh_fpath.endswith(".obj"), f"must use .obj format: {mesh_fpath}"
    dev = _cuda()
    with torch.cuda.device(dev):
        # first stage: uniform 100^3 lattice, largest component
        x = np.linspace(-1.0, 1.0, 100)
        u = _field(sdf, [x, x, x], max_n_pts, dev)
        verts, tris = marching_cubes(u)
        del u
        if tris.shape[0] == 0:
            raise _lib.IronError("export_mesh: the SDF has no zero crossing on the 100^3 lattice of [-1, 1]^3")
        h0 = x[2] - x[1]
        verts = verts.double() * h0
        if translate_first:
            verts = verts + torch.tensor([x[0], x[0], x[0]], dtype=torch.float64, device=dev)
        comp = _largest_component(verts, tris)
        mean, rows = _frame(verts, comp)
        used = torch.unique(comp.reshape(-1))
        local = ((verts[used] - mean) @ rows.T).float().cpu()

        # second stage: the aligned lattice
        axes, _, short = _aligned_axes(local, resolution, 0.1)
        frame32, mean32 = rows.float(), mean.float()
        u = _field(sdf, axes, max_n_pts, dev, frame=frame32, origin=mean32)
        if not bool(((u.min() <= 0) & (u.max() >= 0)).item()):
            return None
        verts, tris = marching_cubes(u)
        del u
        h = axes[0][2] - axes[0][1]
        p0 = torch.tensor([axes[0][0], axes[1][0], axes[2][0]], dtype=torch.float64, device=dev)
        world = (verts.double() * h + p0) @ rows + mean
        _write_obj_vf(mesh_fpath, world.cpu().numpy(), tris.cpu().numpy())
        return {"vertices": world, "faces": tris, "spacing": float(h), "shape": tuple(len(a) for a in axes), "shortest_axis": short,
                "frame": rows, "mean": mean}


def export_mesh(sdf, mesh_fpath, resolution=512, max_n_pts=100000):
    """models/export_mesh.py:export_mesh: `sdf` maps [n, 3] device points to n values; writes `mesh_fpath` (.obj) unless the aligned
    field has no sign change.  Returns {"vertices" fp64 [V, 3], "faces" int64 [F, 3] (device), "spacing", "shape" of the aligned
    lattice, "shortest_axis", "frame" (rows), "mean"}, or None when nothing is written (the reference returns None)."""
    return _export(sdf, mesh_fpath, resolution, max_n_pts, translate_first=True)


def export_mesh_no_translation(sdf, mesh_fpath, resolution=512, max_n_pts=100000):
    """models/export_mesh.py:export_mesh_no_translation: as export_mesh, but the first-stage vertices stay in lattice units times
    the spacing (not moved to the lattice origin), which shifts the frame the reference derives from them."""
    return _export(sdf, mesh_fpath, resolution, max_n_pts, translate_first=False)
