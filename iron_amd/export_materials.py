"""Drop-in for models/export_materials.py (the stage-2 material texture export of render_surface.py --export_all): the same
public names and signatures, with sampling, splat and normalisation on the HIP kernels (iron_amd.texture_bake).
install_as_models() registers it as models.export_materials.

Deviations from the reference, all on purpose:
- No igl / trimesh / imageio.  The OBJ is read by a small reader (`v`, `vt`, `f a/b[/c]` with negative indices, polygons
  fan-triangulated), check_uvmap.ply by a binary PLY point-cloud writer, PNGs through PIL.
- EXR: written through imageio when it imports with an EXR plugin; otherwise each `.exr` becomes a float32 `.npy` beside the
  PNGs (same stem), with one warning per export.
- The random draws of sample_surface come from the kernels' Philox generator; the new `seed=None` parameter draws its seed from
  np.random, so a caller's np.random.seed makes the output reproducible.
- A non-finite material value raises IronError instead of producing NaN texels.
- accumulate_splat_material does not rescale the caller's `uv` array in place.
- Groupby (the reference's host group-by helper of the splat) is not built: the kernel replaces it.
"""
from __future__ import annotations

import os
import struct
import warnings

import numpy as np
import torch

from . import _lib
from .texture_bake import SplatAccumulator, bake_materials, sample_surface_gpu

MTL_TEXT = ("newmtl Wood\n"
            "Ka 1.000000 1.000000 1.000000\n"
            "Kd 0.640000 0.640000 0.640000\n"
            "Ks 0.500000 0.500000 0.500000\n"
            "Ns 96.078431\n"
            "Ni 1.000000\n"
            "d 1.000000\n"
            "illum 0\n"
            "map_Kd diffuse_albedo.png\n")


def to8b(x):
    return np.clip(x * 255.0, 0.0, 255.0).astype(np.uint8)


def _seed(seed):
    return int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64)) if seed is None else int(seed)


def sample_surface(vertices, face_vertices, texturecoords, face_texturecoords, n_samples, seed=None):
    """models/export_materials.py:13-55: numpy in, numpy out -> (points float32 [N,3], uv float32 [N,2]), N >= n_samples.
    Areas and counts are computed in float32 as for the float32 mesh export_materials reads."""
    pts, uv = sample_surface_gpu(np.asarray(vertices, dtype=np.float32), np.asarray(face_vertices), np.asarray(texturecoords, dtype=np.float32),
                                 np.asarray(face_texturecoords), n_samples, _seed(seed))
    return pts.cpu().numpy(), uv.cpu().numpy()


def accumulate_splat_material(xyz_image, material_image, weight_image, pcd, uv, material):
    """models/export_materials.py:77-140: splats the samples into the float32 images, which are updated in place and returned."""
    H, W = material_image.shape[:2]
    acc = SplatAccumulator(H, W, n_values=material_image.reshape(H, W, -1).shape[-1], max_samples=max(1, len(pcd)))
    acc.add(torch.from_numpy(np.ascontiguousarray(pcd, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(uv, dtype=np.float32)),
            torch.from_numpy(np.ascontiguousarray(material, dtype=np.float32).reshape(len(pcd), -1)))
    acc.resolve()  # raises on the range flag
    s = acc.sums().cpu().numpy()
    for img, delta in ((xyz_image, s[..., :3]), (material_image, s[..., 3:-1]), (weight_image, s[..., -1])):
        view = img.reshape(delta.shape)
        np.add(view, delta, out=view, casting="same_kind")  # the reference's float32 += float64 sums
    return xyz_image, material_image, weight_image


# ---- host I/O ----------------------------------------------------------------------------------------------------------------
def read_obj(path):
    """-> (vertices float32 [V,3], texturecoords float32 [T,2], face_vertices int64 [F,3], face_texturecoords int64 [F,3]) like
    igl.read_obj(path, dtype="float32") for `v`, `vt` and `f a/b[/c]` lines (negative indices count back from the last element;
    polygons are fan-triangulated).  Faces without texture indices give an empty face_texturecoords."""
    v, vt, f, ft = [], [], [], []
    with open(path, "r") as fp:
        for line in fp:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                v.append([float(x) for x in tok[1:4]])
            elif tok[0] == "vt":
                vt.append([float(x) for x in tok[1:3]])
            elif tok[0] == "f":
                fv, fuv = [], []
                for c in tok[1:]:
                    parts = c.split("/")
                    i = int(parts[0])
                    fv.append(i - 1 if i > 0 else len(v) + i)
                    if len(parts) > 1 and parts[1]:
                        j = int(parts[1])
                        fuv.append(j - 1 if j > 0 else len(vt) + j)
                for k in range(1, len(fv) - 1):
                    f.append([fv[0], fv[k], fv[k + 1]])
                    if len(fuv) == len(fv):
                        ft.append([fuv[0], fuv[k], fuv[k + 1]])
    vertices = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    texturecoords = np.asarray(vt, dtype=np.float32).reshape(-1, 2)
    faces = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    face_uv = np.asarray(ft, dtype=np.int64).reshape(-1, 3) if len(ft) == len(f) else np.zeros((0, 3), dtype=np.int64)
    return vertices, texturecoords, faces, face_uv


def write_obj(path, vertices, texturecoords, face_vertices, face_texturecoords):
    """A minimal OBJ with `v`, `vt` and `f a/b` lines (1-based), readable by read_obj and by Blender."""
    with open(path, "w") as fp:
        fp.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in np.asarray(vertices, dtype=np.float64))
        fp.writelines("vt %.9g %.9g\n" % tuple(t) for t in np.asarray(texturecoords, dtype=np.float64))
        fp.writelines("f %d/%d %d/%d %d/%d\n" % (a + 1, p + 1, b + 1, q + 1, c + 1, r + 1)
                      for (a, b, c), (p, q, r) in zip(np.asarray(face_vertices), np.asarray(face_texturecoords)))


def write_ply_points(path, points, colors_rgba):
    """Binary little-endian PLY point cloud: float x, y, z and uchar red, green, blue, alpha per vertex."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    col = np.ascontiguousarray(colors_rgba, dtype=np.uint8).reshape(-1, 4)
    rec = np.empty(len(pts), dtype=[("p", "<f4", 3), ("c", "u1", 4)])
    rec["p"], rec["c"] = pts, col
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n" % len(pts))
    with open(path, "wb") as fp:
        fp.write(header.encode("ascii"))
        fp.write(rec.tobytes())


def write_ply_mesh(path, vertices, triangles):
    """Binary little-endian PLY triangle mesh: float x, y, z per vertex, `uchar 3` and three int vertex indices per face."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_ply_mesh: a face names a vertex outside 0 .. %d" % (len(v) - 1))
    rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", 3)])
    rec["n"], rec["i"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    with open(path, "wb") as fp:
        fp.write(header.encode("ascii"))
        fp.write(v.astype("<f4").tobytes())
        fp.write(rec.tobytes())


def _write_png(path, img8):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img8)).save(path)


def _exr_writer():
    try:
        import imageio
        imageio.formats["EXR"]  # raises when no EXR plugin is available
    except Exception:
        return None
    return imageio.imwrite


def _write_exr(path, img, writer, note):
    img = np.ascontiguousarray(img, dtype=np.float32)
    if writer is not None:
        writer(path, img)
        return path
    out = path[:-4] + ".npy"
    np.save(out, img)
    if not note:
        warnings.warn("no imageio EXR plugin: float textures are written as .npy beside the PNGs")
        note.append(out)
    return out


def loadmesh_and_checkuv(obj_fpath, out_dir, seed=None):
    """models/export_materials.py:143-162: read the OBJ, write check_uvmap.ply (1 M samples coloured by uv) and check_uvmap.png;
    -> (vertices, face_vertices, texturecoords, face_texturecoords)."""
    os.makedirs(out_dir, exist_ok=True)
    vertices, texturecoords, face_vertices, face_texturecoords = read_obj(obj_fpath)
    if len(face_vertices) and len(face_texturecoords) != len(face_vertices):
        raise ValueError("%s has faces without texture coordinates (run the UV export first)" % obj_fpath)

    def make_rgba_color(float_rgb):
        float_rgba = np.concatenate((float_rgb, np.ones_like(float_rgb[:, 0:1])), axis=-1)
        return np.uint8(np.clip(float_rgba * 255.0, 0.0, 255.0))

    pcd, pcd_uv = sample_surface(vertices, face_vertices, texturecoords, face_texturecoords, n_samples=10**6, seed=seed)
    uv_color = np.concatenate((pcd_uv, np.zeros_like(pcd_uv[:, 0:1])), axis=-1)
    write_ply_points(os.path.join(out_dir, "check_uvmap.ply"), pcd, make_rgba_color(uv_color))
    W, H = 512, 512
    grid_w, grid_h = np.meshgrid(np.linspace(0.0, 1.0, W), np.linspace(1, 0.0, H))
    grid_color = np.stack((grid_w, grid_h, np.zeros_like(grid_w)), axis=2)
    _write_png(os.path.join(out_dir, "check_uvmap.png"), to8b(grid_color))
    return vertices, face_vertices, texturecoords, face_texturecoords


def export_materials(mesh_fpath, material_predictor, out_dir, max_num_pts=320000, texture_H=2048, texture_W=2048, seed=None):
    """models/export_materials.py:165-222: bake five rounds of 5 M samples into texture_H x texture_W textures, write xyz /
    diffuse_albedo / specular_albedo / roughness as .exr (or .npy, see the module docstring) and to8b .png, the .mtl, and prepend
    the `usemtl` line to the mesh file.  Returns {"xyz", "material", "weight"}: the normalised device textures."""
    os.makedirs(out_dir, exist_ok=True)
    vertices, face_vertices, texturecoords, face_texturecoords = loadmesh_and_checkuv(mesh_fpath, out_dir, seed=seed)
    xyz, material, weight = bake_materials(vertices, face_vertices, texturecoords, face_texturecoords, material_predictor,
                                           texture_H=texture_H, texture_W=texture_W, n_rounds=5, n_samples=5 * 10**6,
                                           max_num_pts=max_num_pts, seed=_seed(seed))
    final_xyz_image = xyz.cpu().numpy()
    final_material_image = material.cpu().numpy()

    writer, note = _exr_writer(), []
    _write_exr(os.path.join(out_dir, "xyz.exr"), final_xyz_image, writer, note)
    _write_exr(os.path.join(out_dir, "diffuse_albedo.exr"), final_material_image[:, :, :3], writer, note)
    _write_exr(os.path.join(out_dir, "specular_albedo.exr"), final_material_image[:, :, 3:6], writer, note)
    _write_exr(os.path.join(out_dir, "roughness.exr"), final_material_image[:, :, 6], writer, note)

    _write_png(os.path.join(out_dir, "xyz.png"), to8b(final_xyz_image * 0.5 + 0.5))
    _write_png(os.path.join(out_dir, "diffuse_albedo.png"), to8b(final_material_image[:, :, :3]))
    _write_png(os.path.join(out_dir, "specular_albedo.png"), to8b(final_material_image[:, :, 3:6]))
    _write_png(os.path.join(out_dir, "roughness.png"), to8b(final_material_image[:, :, 6]))

    out_mesh_fpath = mesh_fpath
    with open(out_mesh_fpath, "r") as original:
        data = original.read()
    with open(out_mesh_fpath, "w") as modified:
        modified.write("usemtl ./{}\n\n".format(os.path.basename(out_mesh_fpath)[:-4] + ".mtl") + data)

    with open(os.path.join(out_dir, os.path.basename(out_mesh_fpath)[:-4] + ".mtl"), "w") as fp:
        fp.write(MTL_TEXT)
    return {"xyz": xyz, "material": material, "weight": weight}
