"""Flash render of an exported asset on the HIP kernels (csrc/meshrender.hip): the mesh of export_mesh /
export_uv with the textures of export_materials, lit by a point light at the camera, the way the reference checks its assets with
render_synthetic_data/render_rgb_flash_mat.py (Mitsuba's roughplastic under a co-located flash).

Conventions (include/iron_hip.h, iron_mesh_raycast block): closest hits over the MeshBVH of mesh_distance (watertight, two-sided,
ties to the smallest face index); uv interpolated through the face's own face_uvs; the texture fetch in the bake's pixel convention
(x = uv_x W - 1/2, y = H - uv_y H - 1/2, taps the bake never wrote dropped when the weight image is given); shading by the same
ggx_colocated_point as GGXColocatedRenderer, with the normal never flipped towards the viewer.  Vertex normals are area-weighted
(the sum of the faces' un-normalised cross products): this project's choice, not pinned to Mitsuba's smoothing.  There is no CPU
path: CPU tensors are refused.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _args, _lib
from .envmap import EnvMap  # noqa: F401  (render_asset_env's light)
from .mesh_distance import MeshBVH

TEX_MODES = {"bilinear": 0, "nearest": 1}


WHAT = "mesh render"  # what this module's messages begin with


def vertex_normals(V, F) -> torch.Tensor:
    """Area-weighted vertex normals [V, 3] fp32 on the device: per vertex the sum of its faces' un-normalised cross products,
    normalised; the zero vector where the sum is zero.  Accumulated in int64 fixed point: bitwise reproducible.  Waits once."""
    dev = _args.pick_device(WHAT, V, F)
    with torch.cuda.device(dev):
        v = _args.device_array(V, torch.float32, dev, "vertices", (3,), what=WHAT)
        f = _args.face_array(F, dev, what=WHAT)
        out = torch.empty_like(v)
        _lib.check(_lib.load().iron_mesh_vertex_normals(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], out.data_ptr(),
                                                        _lib.stream_ptr(dev)))
    return out


def _texture(tex, dev, name="tex") -> torch.Tensor:
    t = _args.as_tensor(tex, WHAT)
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3 or not 1 <= t.shape[2] <= 8 or t.shape[0] * t.shape[1] == 0 or t.shape[0] * t.shape[1] > 1 << 24:
        raise _lib.IronError("%s must be [H, W, C <= 8] with 0 < H * W <= 2^24, got %s" % (name, tuple(t.shape)))
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _weight(weight, tex, dev):
    if weight is None:
        return None
    w = _args.as_tensor(weight, WHAT)
    if tuple(w.shape) != tuple(tex.shape[:2]):
        raise _lib.IronError("weight must be [H, W] = %s, got %s" % (tuple(tex.shape[:2]), tuple(w.shape)))
    return w.to(device=dev, dtype=torch.float32).contiguous()


def sample_texture(tex, uv, weight=None, mode="bilinear"):
    """tex [H, W, C <= 8] (or [H, W]) at uv [n, 2] in the bake's convention -> (values fp32 [n, C], hole bool [n]).  `weight`
    [H, W]: the bake's weight image; taps it marks unwritten (0) are dropped and the rest renormalised, `hole` where none is left."""
    if mode not in TEX_MODES:
        raise _lib.IronError("mode must be one of %s, got %r" % (sorted(TEX_MODES), mode))
    dev = _args.pick_device(WHAT, tex, uv, weight)
    with torch.cuda.device(dev):
        t = _texture(tex, dev)
        w = _weight(weight, t, dev)
        q = _args.device_array(uv, torch.float32, dev, "uv", (2,), what=WHAT)
        n, (H, W, Cn) = int(q.shape[0]), t.shape
        val = torch.empty((n, Cn), dtype=torch.float32, device=dev)
        hole = torch.empty((n,), dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().iron_texture_fetch(t.data_ptr(), _lib.ptr(w), H, W, Cn, q.data_ptr(), n, TEX_MODES[mode], val.data_ptr(),
                                                  hole.data_ptr(), _lib.stream_ptr(dev)))
    return val, hole.bool()


def _read_float_image(texture_dir, stems):
    """The first of STEM.exr (when imageio has an EXR plugin), STEM.npy, STEM.png (8-bit, / 255) that exists, else None."""
    for stem in stems:
        base = os.path.join(texture_dir, stem)
        if os.path.exists(base + ".exr"):
            try:
                import imageio
                imageio.formats["EXR"]  # raises when no EXR plugin is available
                return np.asarray(imageio.imread(base + ".exr"), dtype=np.float32)
            except Exception:
                pass
        if os.path.exists(base + ".npy"):
            return np.load(base + ".npy", allow_pickle=False).astype(np.float32)
        if os.path.exists(base + ".png"):
            from PIL import Image
            return np.asarray(Image.open(base + ".png"), dtype=np.float32) / 255.0
    return None


def read_asset(obj_path, texture_dir) -> dict:
    """The asset export_mesh / export_uv / export_materials write, as numpy arrays {vertices, faces, uvs, face_uvs, material
    [H, W, 7], weight [H, W] or None}: the OBJ by export_materials.read_obj; diffuse_albedo, specular_albedo and roughness (or the
    reference script's specular_roughness) from texture_dir, each as .exr when imageio has an EXR plugin, else the .npy beside it,
    else the 8-bit .png; weight.* likewise when present."""
    from .export_materials import read_obj
    v, vt, f, ft = read_obj(obj_path)
    if len(f) == 0 or len(ft) != len(f):
        raise _lib.IronError("%s has no faces, or faces without texture coordinates" % obj_path)
    maps = []
    for stems, ch in ((("diffuse_albedo",), 3), (("specular_albedo",), 3), (("roughness", "specular_roughness"), 1)):
        img = _read_float_image(texture_dir, stems)
        if img is None:
            raise _lib.IronError("no %s.{exr,npy,png} in %s" % ("|".join(stems), texture_dir))
        img = img.reshape(img.shape[0], img.shape[1], -1)
        if img.shape[2] < ch:
            img = np.repeat(img[:, :, :1], ch, axis=2)
        maps.append(img[:, :, :ch])
    if len({m.shape[:2] for m in maps}) != 1:
        raise _lib.IronError("the textures in %s differ in size" % texture_dir)
    weight = _read_float_image(texture_dir, ("weight",))
    if weight is not None:
        weight = weight.reshape(weight.shape[0], weight.shape[1], -1)[:, :, 0]
    return {"vertices": v, "faces": f, "uvs": vt, "face_uvs": ft, "material": np.ascontiguousarray(np.concatenate(maps, axis=2)),
            "weight": weight}


class MeshAsset:
    """A textured mesh on the GPU: vertices [V, 3], faces [F, 3], uvs [T, 2], face_uvs [F, 3] (numpy or CUDA tensors), material
    [H, W, 7] in bake_materials' channel order (kd 3, ks 3, roughness), optionally the bake's weight [H, W].  normals: "vertex"
    (area-weighted, interpolated) or "face" (geometric).  Builds the BVH (and the vertex normals) once."""

    def __init__(self, vertices, faces, uvs, face_uvs, material, weight=None, normals="vertex", device=None):
        if normals not in ("vertex", "face"):
            raise _lib.IronError("normals must be 'vertex' or 'face', got %r" % (normals,))
        dev = torch.device(device) if device is not None else _args.pick_device(WHAT, vertices, faces, uvs, face_uvs, material, weight)
        _args.refuse_cpu(WHAT, vertices, faces, uvs, face_uvs, material, weight)
        self.device = dev
        with torch.cuda.device(dev):
            self.bvh = MeshBVH(vertices, faces, device=dev)
            self.vertices, self.faces = self.bvh.vertices, self.bvh.faces
            self.uvs = _args.device_array(uvs, torch.float32, dev, "uvs", (2,), what=WHAT)
            self.face_uvs = _args.face_array(face_uvs, dev, what=WHAT)
            if self.face_uvs.shape[0] != self.faces.shape[0]:
                raise _lib.IronError("face_uvs has %d rows, faces %d" % (self.face_uvs.shape[0], self.faces.shape[0]))
            if self.uvs.shape[0] == 0 or int(self.face_uvs.min()) < 0 or int(self.face_uvs.max()) >= self.uvs.shape[0]:
                raise _lib.IronError("MeshAsset: a face_uvs index lies outside [0, %d)" % self.uvs.shape[0])
            self.material = _texture(material, dev, "material")
            if self.material.shape[2] != 7:
                raise _lib.IronError("material must have 7 channels (kd 3, ks 3, roughness), got %d" % self.material.shape[2])
            self.weight = _weight(weight, self.material, dev)
            self.normal_mode = normals
            self.normals = vertex_normals(self.vertices, self.faces) if normals == "vertex" else None

    @classmethod
    def load(cls, obj_path, texture_dir, normals="vertex", device=None):
        """The asset on disk (read_asset) on the GPU."""
        a = read_asset(obj_path, texture_dir)
        dev = torch.device(device) if device is not None else _args.pick_device(WHAT)
        return cls(a["vertices"], a["faces"], a["uvs"], a["face_uvs"], a["material"], weight=a["weight"], normals=normals, device=dev)

    def _shade_buffers(self, n):
        """The per-ray outputs of the shading entries and the two C structures that describe them and the mesh."""
        dev = self.device
        out = {k: torch.empty((n, 3), dtype=torch.float32, device=dev)
               for k in ("color", "diffuse_color", "specular_color", "normal", "points", "diffuse_albedo", "specular_albedo")}
        out["distance"] = torch.empty((n,), dtype=torch.float32, device=dev)
        out["specular_roughness"] = torch.empty((n,), dtype=torch.float32, device=dev)
        out["uv"] = torch.empty((n, 2), dtype=torch.float32, device=dev)
        out["hole"] = torch.empty((n,), dtype=torch.uint8, device=dev)
        H, W = self.material.shape[:2]
        mesh = _lib.iron_asset_mesh(self.vertices.data_ptr(), self.vertices.shape[0], self.faces.data_ptr(), self.faces.shape[0],
                                    self.uvs.data_ptr(), self.uvs.shape[0], self.face_uvs.data_ptr(), _lib.ptr(self.normals),
                                    self.material.data_ptr(), _lib.ptr(self.weight), H, W)
        return out, mesh, _lib.iron_asset_out(*[out[k].data_ptr() for k in _lib.ASSET_OUT_FIELDS])

    def shade(self, ray_o, ray_d, t, face_idx, bary, light, tables):
        """iron_asset_shade_ggx on n rays (ray_d unit) -> dict of per-ray device tensors, _lib.ASSET_OUT_FIELDS."""
        dev = self.device
        n = int(ray_o.shape[0])
        out, mesh, o = self._shade_buffers(n)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().iron_asset_shade_ggx(C.byref(mesh), float(light), tables[0].data_ptr(), tables[1].data_ptr(),
                                                        ray_o.data_ptr(), ray_d.data_ptr(), t.data_ptr(), face_idx.data_ptr(),
                                                        bary.data_ptr(), n, C.byref(o), _lib.stream_ptr(dev)))
        return out

    def shade_env(self, ray_o, ray_d, t, face_idx, bary, envmap, tables, n_light=64, n_brdf=64, seed=0, shadow_eps=1e-4, pixel_idx=None,
                  dump=False):
        """iron_asset_shade_env on n rays (ray_d unit): direct illumination by `envmap` (EnvMap) with n_light environment samples
        and n_brdf BRDF samples per ray, combined by the balance heuristic -> the dictionary of `shade`.  pixel_idx [n] int32
        (default: the ray's position) keys the random numbers, so a subset of the rays with their own indices reproduces the whole
        call bitwise.  dump=True adds the per-sample "dump_dir" [n, N, 3], "dump_denom" [n, N], "dump_vis" [n, N] uint8 and
        "dump_contrib" [n, N, 3] (N = n_light + n_brdf, environment samples first) for tests."""
        dev = self.device
        n, N = int(ray_o.shape[0]), int(n_light) + int(n_brdf)
        if n_light < 0 or n_brdf < 0 or N > 1 << 20:
            raise _lib.IronError("shade_env: n_light and n_brdf must be >= 0 with at most 2^20 samples together")
        out, mesh, o = self._shade_buffers(n)
        d = _lib.iron_env_dump(None, None, None, None)
        if dump:
            out["dump_dir"] = torch.empty((n, N, 3), dtype=torch.float32, device=dev)
            out["dump_denom"] = torch.empty((n, N), dtype=torch.float32, device=dev)
            out["dump_vis"] = torch.empty((n, N), dtype=torch.uint8, device=dev)
            out["dump_contrib"] = torch.empty((n, N, 3), dtype=torch.float32, device=dev)
            d = _lib.iron_env_dump(*[out[k].data_ptr() for k in ("dump_dir", "dump_denom", "dump_vis", "dump_contrib")])
        with torch.cuda.device(dev):
            pix = None if pixel_idx is None else _args.device_array(pixel_idx, torch.int32, dev, "pixel_idx", (), what=WHAT)
            if pix is not None and pix.shape[0] != n:
                raise _lib.IronError("ray_o has %d rows, pixel_idx %d" % (n, pix.shape[0]))
            env = envmap.c_struct()
            _lib.check(_lib.load().iron_asset_shade_env(C.byref(mesh), self.bvh.workspace.data_ptr(), C.byref(env), tables[0].data_ptr(),
                                                        tables[1].data_ptr(), ray_o.data_ptr(), ray_d.data_ptr(), t.data_ptr(),
                                                        face_idx.data_ptr(), bary.data_ptr(), _lib.ptr(pix), n, int(n_light), int(n_brdf),
                                                        int(seed) & 0xFFFFFFFF, float(shadow_eps), C.byref(o), C.byref(d),
                                                        _lib.stream_ptr(dev)))
        return out

    def shade_env_indirect(self, ray_o, ray_d, t, face_idx, bary, envmap, tables, n_paths=64, max_depth=2, seed=0, shadow_eps=1e-4,
                           pixel_idx=None, dump=False):
        """iron_asset_shade_env_indirect on n rays (ray_d unit): the light that leaves the primary hits after at least one
        interreflection, by n_paths (1 .. 2^16) paths per ray of at most max_depth (2 .. 8) surface vertices, the primary hit
        included -> {"indirect_diffuse", "indirect_specular" (through the primary hit's diffuse and specular lobe),
        "indirect_color" (their sum)}, [n, 3] each.  seed, shadow_eps and pixel_idx as in shade_env; a path's random numbers are
        disjoint from that call's.  dump=True adds "dump_" + every name of _lib.ENV_PATH_DUMP_FIELDS, per (ray, path, vertex)
        ([n, n_paths, max_depth, ...]; the two lobe weights per (ray, path)), for tests."""
        check_path_args(max_depth, n_paths, indirect=True)
        dev = self.device
        n, P, D = int(ray_o.shape[0]), int(n_paths), int(max_depth)
        out = {k: torch.empty((n, 3), dtype=torch.float32, device=dev) for k in ("indirect_diffuse", "indirect_specular")}
        d = _lib.iron_env_path_dump()
        if dump:
            for k in _lib.ENV_PATH_DUMP_FIELDS:
                shape = (n, P) if k.startswith("lobe_") else (n, P, D)
                kind = {"face": ((), torch.int32), "light_vis": ((), torch.uint8), "t": ((), torch.float32),
                        "denom_light": ((), torch.float32), "denom_brdf": ((), torch.float32)}.get(k, ((3,), torch.float32))
                out["dump_" + k] = torch.empty(shape + kind[0], dtype=kind[1], device=dev)
            d = _lib.iron_env_path_dump(*[out["dump_" + k].data_ptr() for k in _lib.ENV_PATH_DUMP_FIELDS])
        H, W = self.material.shape[:2]
        mesh = _lib.iron_asset_mesh(self.vertices.data_ptr(), self.vertices.shape[0], self.faces.data_ptr(), self.faces.shape[0],
                                    self.uvs.data_ptr(), self.uvs.shape[0], self.face_uvs.data_ptr(), _lib.ptr(self.normals),
                                    self.material.data_ptr(), _lib.ptr(self.weight), H, W)
        with torch.cuda.device(dev):
            pix = None if pixel_idx is None else _args.device_array(pixel_idx, torch.int32, dev, "pixel_idx", (), what=WHAT)
            if pix is not None and pix.shape[0] != n:
                raise _lib.IronError("ray_o has %d rows, pixel_idx %d" % (n, pix.shape[0]))
            env = envmap.c_struct()
            _lib.check(_lib.load().iron_asset_shade_env_indirect(C.byref(mesh), self.bvh.workspace.data_ptr(), C.byref(env),
                                                                 tables[0].data_ptr(), tables[1].data_ptr(), ray_o.data_ptr(),
                                                                 ray_d.data_ptr(), t.data_ptr(), face_idx.data_ptr(), bary.data_ptr(),
                                                                 _lib.ptr(pix), n, P, D, int(seed) & 0xFFFFFFFF, float(shadow_eps),
                                                                 out["indirect_diffuse"].data_ptr(), out["indirect_specular"].data_ptr(),
                                                                 C.byref(d), _lib.stream_ptr(dev)))
        out["indirect_color"] = out["indirect_diffuse"] + out["indirect_specular"]
        return out


def check_path_args(max_depth, n_paths, indirect=False):
    """The host-side refusal of the path integrator's two counts: max_depth 1 .. 8 (2 .. 8 for the indirect kernel itself, which does
    not run at 1), n_paths 1 .. 2^16."""
    lo = 2 if indirect else 1
    if int(max_depth) != max_depth or not lo <= max_depth <= 8:
        raise _lib.IronError("max_depth must be an integer in %d .. 8, got %r" % (lo, max_depth))
    if int(n_paths) != n_paths or not 1 <= n_paths <= 1 << 16:
        raise _lib.IronError("n_paths must be an integer in 1 .. 2^16, got %r" % (n_paths,))


_tables = {}


def _mts_tables(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _tables:
        from .renderer_ggx import load_mts_tables
        _tables[key] = tuple(t.to(dev) for t in load_mts_tables())
    return _tables[key]


def render_asset_uv(camera, asset, light, uv, env=None):
    """One ray per entry of uv [H, W, 2] (pixel coordinates of `camera`): the dictionary of render_asset_camera for one sample
    per pixel.  Pixels go to the ray cast's lanes row-major: one 8x8 pixel tile per 64-lane wave measured slower.
    env: None for the flash of intensity `light`, else the keywords of MeshAsset.shade_env plus `background`, `max_depth` and
    `n_paths` (render_asset_env); max_depth > 1 adds the key indirect_color."""
    _args.refuse_cpu(WHAT, uv, camera.K)
    dev = asset.device
    H, W = int(uv.shape[0]), int(uv.shape[1])
    with torch.cuda.device(dev):
        ray_o, ray_d, ray_d_norm = camera.get_rays(uv)
        o, d = ray_o.reshape(-1, 3), ray_d.reshape(-1, 3)
        t, face, bary = asset.bvh.raycast(o, d)
        if env is None:
            s = asset.shade(o, d, t, face, bary, light, _mts_tables(dev))
        else:
            env = dict(env)
            background = env.pop("background", False)
            max_depth, n_paths = env.pop("max_depth", 1), env.pop("n_paths", 64)
            s = asset.shade_env(o, d, t, face, bary, tables=_mts_tables(dev), **env)
            if max_depth > 1:  # the interreflections, lobe by lobe; the direct term above is untouched
                ind = asset.shade_env_indirect(o, d, t, face, bary, env["envmap"], _mts_tables(dev), n_paths=n_paths, max_depth=max_depth,
                                               seed=env.get("seed", 0), shadow_eps=env.get("shadow_eps", 1e-4))
                s["indirect_color"] = ind["indirect_color"]
                s["diffuse_color"] = s["diffuse_color"] + ind["indirect_diffuse"]
                s["specular_color"] = s["specular_color"] + ind["indirect_specular"]
                s["color"] = s["diffuse_color"] + s["specular_color"]
            if background:  # the map itself behind the asset
                s["color"] = torch.where((face < 0)[:, None], env["envmap"].lookup(d), s["color"])
    img = lambda x: x.reshape([H, W] + list(x.shape[1:]))  # noqa: E731
    res = {k: img(s[k]) for k in ("color", "diffuse_color", "specular_color", "normal", "diffuse_albedo", "specular_albedo",
                                  "specular_roughness", "distance", "points")}
    if "indirect_color" in s:
        res["indirect_color"] = img(s["indirect_color"])
    res["convergent_mask"] = img(face >= 0)
    res["depth"] = res["distance"] / ray_d_norm
    res.update({"uv": uv, "ray_o": ray_o, "ray_d": ray_d, "ray_d_norm": ray_d_norm, "face_idx": img(face), "barycentric": img(bary),
                "tex_uv": img(s["uv"]), "texture_hole": img(s["hole"].bool()), "t": img(t)})
    return res


# the maps render_asset_camera averages over a pixel's samples (misses count as zero: a box filter over the pixel)
AVERAGED = ("color", "diffuse_color", "specular_color", "normal", "diffuse_albedo", "specular_albedo", "specular_roughness", "distance",
            "depth", "points")


def subpixel_uvs(camera, samples_per_axis):
    """The s^2 sample grids [H, W, 2] of render_asset_camera, in its order (rows of the sub-pixel grid outer, columns inner):
    sample (j, i) of pixel (x, y) sits at (x + (i + 1/2) / s, y + (j + 1/2) / s)."""
    s = int(samples_per_axis)
    base = camera.get_uv() - 0.5
    return [base + torch.tensor([(i + 0.5) / s, (j + 0.5) / s], dtype=torch.float32, device=base.device) for j in range(s) for i in range(s)]


@torch.no_grad()
def render_asset_camera(camera, asset, light, samples_per_axis=1, _env=None):
    """Render `asset` (MeshAsset) from `camera` (raytracer.Camera, on the asset's device) under a point light of intensity `light`
    at the camera origin.  Returns render_camera's keys, all [H, W, ...] device tensors: color, diffuse_color, specular_color,
    normal, diffuse_albedo, specular_albedo, specular_roughness, convergent_mask, distance, depth, points, uv, ray_o, ray_d, plus
    face_idx (-1: miss), barycentric, tex_uv, texture_hole, and t, ray_d_norm, coverage.  Direct illumination only (render_asset_env
    has the interreflections).
    samples_per_axis = s > 1 casts s^2 rays per pixel on a regular sub-pixel grid (subpixel_uvs): the AVERAGED maps are the sum of
    the s^2 frames in that order, divided by s^2 (torch, fixed order: bitwise reproducible); convergent_mask is coverage >= 1/2
    (`coverage` is returned too); texture_hole is the union; the per-ray keys (t, face_idx, barycentric, tex_uv, ray_o, ray_d) are
    those of the first sample, uv the pixel centres."""
    s = int(samples_per_axis)
    if s < 1:
        raise _lib.IronError("samples_per_axis must be >= 1")
    _args.refuse_cpu(WHAT, camera.K)
    if s == 1:
        res = render_asset_uv(camera, asset, light, camera.get_uv(), env=_env and _env(0))
        res["coverage"] = res["convergent_mask"].float()
        return res
    res = None
    for k, uv in enumerate(subpixel_uvs(camera, s)):
        f = render_asset_uv(camera, asset, light, uv, env=_env and _env(k))
        if res is None:
            res = f
            averaged = AVERAGED + tuple(k for k in ("indirect_color",) if k in f)
            res["coverage"] = f["convergent_mask"].float()
        else:
            for k in averaged:
                res[k] = res[k] + f[k]
            res["coverage"] = res["coverage"] + f["convergent_mask"].float()
            res["texture_hole"] = res["texture_hole"] | f["texture_hole"]
    for k in averaged + ("coverage",):
        res[k] = res[k] / float(s * s)
    res["convergent_mask"] = res["coverage"] >= 0.5
    res["uv"] = camera.get_uv()
    return res


@torch.no_grad()
def render_asset_env(camera, asset, envmap, n_light=64, n_brdf=64, seed=0, samples_per_axis=1, background=False, shadow_eps=1e-4,
                     max_depth=1, n_paths=64):
    """Render `asset` from `camera` under the environment map `envmap` (EnvMap on the asset's device): direct illumination with
    visibility, n_light environment samples and n_brdf BRDF samples per ray combined by the balance heuristic (csrc/envlight.hip,
    DESIGN.md §16).  Returns render_asset_camera's dictionary with the same keys; distance and depth keep their meaning.  Sub-pixel
    frames are averaged exactly as there, sample k of the sub-pixel grid with seed + k.  background=True fills `color` of every
    ray that misses with envmap.lookup(ray_d) (before the averaging); the default leaves zeros there, like the flash render.
    max_depth (1 .. 8): the largest number of surface vertices on a light path, the primary hit included.  1 is direct illumination
    alone.  Above 1, n_paths (1 .. 2^16) paths per ray add the interreflections (MeshAsset.shade_env_indirect; the
    direct term is unchanged): the dictionary gains indirect_color, diffuse_color and specular_color are direct + indirect of that
    lobe (averaged over the sub-pixel frames like every map), and color = diffuse_color + specular_color of the averaged maps; under
    background=True a pixel with a ray that misses keeps the mean of its frames' colours, which holds the map."""
    check_path_args(max_depth, n_paths)
    env = lambda k: {"envmap": envmap, "n_light": n_light, "n_brdf": n_brdf, "seed": int(seed) + k,  # noqa: E731
                     "shadow_eps": shadow_eps, "background": background}
    if max_depth == 1:
        return render_asset_camera(camera, asset, 0.0, samples_per_axis=samples_per_axis, _env=env)
    res = render_asset_camera(camera, asset, 0.0, samples_per_axis=samples_per_axis,
                              _env=lambda k: dict(env(k), max_depth=int(max_depth), n_paths=int(n_paths)))
    lobes = res["diffuse_color"] + res["specular_color"]
    # a pixel with a ray that misses under background=True keeps the mean of its frames' colours, which holds the map
    res["color"] = torch.where((res["coverage"] >= 1.0)[..., None], lobes, res["color"]) if background else lobes
    return res
