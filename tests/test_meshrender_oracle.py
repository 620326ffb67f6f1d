"""CPU: the fp64 oracle of the asset renderer (tests/_meshrender_oracle.py) against closed forms, and the host surface of
iron_amd.mesh_render (import, CPU tensors refused, the asset reader)."""
import math
import os

import numpy as np
import pytest
import torch

import _meshdist_oracle as MO
import _meshrender_oracle as O

INF = float("inf")


def _rays(o, d):
    return torch.tensor(o, dtype=torch.float64), torch.tensor(d, dtype=torch.float64)


def test_cube_axis_aligned_and_diagonal_rays():
    v, f = MO.unit_cube()
    o, d = _rays([[-1, 0.5, 0.25], [0.5, 0.25, -2], [0.25, 3.0, 0.5], [2, 2, 2], [-1, -1, -1], [-1.0, 0.25, 0.5]],
                 [[1, 0, 0], [0, 0, 1], [0, -2, 0], [1, 0, 0], [-1, -1, -1], [1.0, 0.5, 0.0]])
    t, face, bary, margin = O.closest_hit(o, d, v, f)
    # (-1,.5,.25)+t(1,0,0) meets x=0 at 1; (.5,.25,-2)+t(0,0,1) meets z=0 at 2; a direction of length 2 halves t: y=1 at 1;
    # the last leaves (-1,.25,.5) along (1,.5,0): x=0 at t=1, y=.75 inside
    assert t[:3].tolist() == [1.0, 2.0, 1.0]
    assert t[3] == INF and face[3] == -1 and t[4] == INF
    assert t[5] == 1.0
    assert (face[:3] >= 0).all() and (margin[:3] > 0).all()
    # the hit point from the barycentrics
    tri = v[f[face[0]]]
    p = (1 - bary[0, 0] - bary[0, 1]) * tri[0] + bary[0, 0] * tri[1] + bary[0, 1] * tri[2]
    assert torch.allclose(p, torch.tensor([0.0, 0.5, 0.25], dtype=torch.float64), atol=1e-15)
    # the main diagonal from outside: corner (0,0,0) at |(-1,-1,-1)| = sqrt 3 for a unit direction
    o, d = _rays([[-1, -1, -1]], [[1 / math.sqrt(3)] * 3])
    t = O.closest_hit(o, d, v, f)[0]
    assert abs(float(t[0]) - math.sqrt(3)) < 1e-14


def test_rays_through_a_corner_and_an_edge_hit():
    v, f = MO.unit_cube()
    # through the corner (0,0,0) along (1,1,1) (integers: exact), and through the midpoint of the edge x=0,z=1 along (1,0,-1)
    o, d = _rays([[-1, -1, -1], [-1, 0.5, 2.0], [0.0, 0.3, -1.0]], [[1, 1, 1], [1, 0, -1], [0, 0, 1]])
    t, face, _, margin = O.closest_hit(o, d, v, f)
    assert t.tolist() == [1.0, 1.0, 1.0]
    assert (face >= 0).all()
    assert (margin == 0).all()  # on the boundary of the winning face
    # ties go to the smallest face index: the corner belongs to faces 0, 1, 4, 5, 8, 9
    assert int(face[0]) == 0


def test_window_and_invalid_rays():
    v, f = MO.unit_cube()
    o, d = _rays([[-1, 0.5, 0.25]], [[1, 0, 0]])
    assert float(O.closest_hit(o, d, v, f, t_min=1.5)[0]) == 2.0      # the nearer hit cut, the farther exposed
    assert float(O.closest_hit(o, d, v, f, t_min=1.0)[0]) == 2.0      # the near end is exclusive
    assert float(O.closest_hit(o, d, v, f, t_max=1.0)[0]) == 1.0      # the far end inclusive
    assert float(O.closest_hit(o, d, v, f, t_max=0.5)[0]) == INF
    o, d = _rays([[-1, 0.5, 0.25], [float("nan"), 0.5, 0.25], [-1, 0.5, 0.25]], [[0, 0, 0], [1, 0, 0], [INF, 0, 0]])
    t, face, _, _ = O.closest_hit(o, d, v, f)
    assert (t == INF).all() and (face == -1).all()


def test_fp32_restatement_runs_the_same_formulas():
    v, f = MO.unit_cube()
    o, d = _rays([[-1, 0.5, 0.25], [0.3, 0.4, 5.0]], [[1, 0, 0], [0.1, -0.05, -1.0]])
    t64, f64, _, _ = O.closest_hit(o, d, v, f)
    t32, f32, b32, _ = O.closest_hit(o, d, v, f, dtype=torch.float32)
    assert t32.dtype == torch.float32 and b32.dtype == torch.float32
    assert (f64 == f32).all() and torch.allclose(t32.double(), t64, rtol=1e-6)


def test_vertex_normals_closed_forms():
    v, f = MO.unit_cube()
    n, l, mag = O.vertex_normals(v, f)
    # the eight normals are unit and all on one side of the surface (the side the winding of the face list decides); corner 0
    # touches one triangle of each of its three faces' pairs or two: (1,1,1)-symmetric there
    assert torch.allclose(n.norm(dim=1), torch.ones(8, dtype=torch.float64))
    side = (n * (v - 0.5)).sum(-1)
    assert (side > 0).all() or (side < 0).all()
    assert torch.allclose(n[0].abs(), torch.full((3,), 1 / math.sqrt(3), dtype=torch.float64))
    sv, sf = O.uv_sphere(12, 24, 1.0)
    sn = O.vertex_normals(sv, sf)[0]
    assert float((sn - sv / sv.norm(dim=1, keepdim=True)).norm(dim=1).max()) < (math.pi / 12) ** 2  # radial to second order in the 15-degree step
    assert sn[0].tolist() == [0.0, 0.0, 1.0]  # exactly at the symmetric pole
    # an unreferenced vertex, and two opposite faces that cancel
    v2 = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=torch.float64)
    f2 = torch.tensor([[0, 1, 2], [0, 2, 1]])
    n2, l2, mag2 = O.vertex_normals(v2, f2)
    assert (n2 == 0).all() and (l2 == 0).all() and mag2[0] == 2.0 and mag2[3] == 0.0


def test_fetch_at_texel_centres_returns_the_texel():
    g = torch.Generator().manual_seed(0)
    H, W, C = 5, 7, 3
    tex = torch.rand((H, W, C), generator=g, dtype=torch.float64)
    rows, cols = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    # texel (row, col) has its centre at uv = ((col + 1/2) / W, 1 - (row + 1/2) / H): the bake's v = H - uv_y H
    uv = torch.stack([(cols.reshape(-1) + 0.5) / W, 1.0 - (rows.reshape(-1) + 0.5) / H], -1).double()
    for mode in ("bilinear", "nearest"):
        val, hole = O.texture_fetch(tex, uv, mode=mode)
        assert not hole.any()
        assert torch.allclose(val, tex.reshape(-1, C), atol=1e-13), mode
    # half-way between two texel centres: their mean; beyond the edge: the edge texel
    val, _ = O.texture_fetch(tex, torch.tensor([[1.0 / W, 1.0 - 0.5 / H], [0.0, 1.0], [1.0, 0.0]], dtype=torch.float64))
    assert torch.allclose(val[0], (tex[0, 0] + tex[0, 1]) / 2, atol=1e-13)
    assert torch.allclose(val[1], tex[0, 0], atol=1e-13) and torch.allclose(val[2], tex[H - 1, W - 1], atol=1e-13)


def test_weighted_fetch_of_a_constant_texture_is_the_constant():
    g = torch.Generator().manual_seed(1)
    H, W = 9, 11
    tex = torch.full((H, W, 2), 0.375, dtype=torch.float64)
    weight = torch.rand((H, W), generator=g, dtype=torch.float64) + 0.01
    uv = torch.rand((500, 2), generator=g, dtype=torch.float64)
    val, hole = O.texture_fetch(tex, uv, weight=weight)
    assert not hole.any() and torch.allclose(val, torch.full_like(val, 0.375), atol=1e-14)
    # a zero patch: taps inside it are dropped; where all four are zero the value is 0 and the sample is a hole
    weight[2:6, 3:8] = 0.0
    junk = tex.clone()
    junk[2:6, 3:8] = 123.0  # what an unbaked texel holds must not matter
    val, hole = O.texture_fetch(junk, uv, weight=weight)
    assert hole.any() and not hole.all()
    assert (val[hole] == 0).all() and torch.allclose(val[~hole], torch.full_like(val[~hole], 0.375), atol=1e-14)
    nv, nh = O.texture_fetch(junk, uv, weight=weight, mode="nearest")
    assert (nv[nh] == 0).all() and (nv[~nh] == 0.375).all()


# ---- the package's host surface ----
def test_mesh_render_imports_and_refuses_cpu_tensors():
    from iron_amd import _lib, mesh_render, render_asset  # noqa: F401
    from iron_amd.mesh_distance import MeshBVH
    assert hasattr(MeshBVH, "raycast")
    v, f = MO.unit_cube()
    with pytest.raises(_lib.IronError, match="CPU tensors"):
        mesh_render.vertex_normals(v.float(), f)
    with pytest.raises(_lib.IronError, match="CPU tensors"):
        mesh_render.sample_texture(torch.zeros(4, 4, 3), torch.zeros(2, 2))
    with pytest.raises(_lib.IronError, match="CPU tensors"):
        mesh_render.MeshAsset(v.float(), f, torch.zeros(3, 2), torch.zeros(12, 3, dtype=torch.int64), torch.zeros(4, 4, 7))
    with pytest.raises(_lib.IronError):
        mesh_render.sample_texture(np.zeros((4, 4, 3), np.float32), np.zeros((2, 2), np.float32), mode="cubic")


def test_read_asset_round_trips_a_tiny_obj_and_npy_textures(tmp_path):
    from iron_amd import _lib, mesh_render
    from iron_amd.export_materials import write_obj
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], dtype=np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int64)
    vt = np.array([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9], [0.9, 0.9], [0.5, 0.5]], dtype=np.float32)
    ft = np.array([[0, 1, 2], [4, 1, 3]], dtype=np.int64)
    obj = os.path.join(tmp_path, "model.obj")
    write_obj(obj, v, vt, f, ft)
    rng = np.random.default_rng(0)
    kd, ks, rough = (rng.random((6, 8, 3), dtype=np.float32), rng.random((6, 8, 3), dtype=np.float32), rng.random((6, 8), dtype=np.float32))
    np.save(os.path.join(tmp_path, "diffuse_albedo.npy"), kd)
    np.save(os.path.join(tmp_path, "specular_albedo.npy"), ks)
    np.save(os.path.join(tmp_path, "specular_roughness.npy"), rough)  # the reference script's name
    a = mesh_render.read_asset(obj, str(tmp_path))
    assert np.array_equal(a["vertices"], v) and np.array_equal(a["faces"], f)
    assert np.array_equal(a["uvs"], vt) and np.array_equal(a["face_uvs"], ft)
    assert a["material"].shape == (6, 8, 7) and a["material"].dtype == np.float32 and a["weight"] is None
    assert np.array_equal(a["material"][..., :3], kd) and np.array_equal(a["material"][..., 3:6], ks)
    assert np.array_equal(a["material"][..., 6], rough)
    # the project's own name wins over the reference's; a weight image is picked up; 8-bit PNG is the last resort
    np.save(os.path.join(tmp_path, "roughness.npy"), rough * 0.5)
    np.save(os.path.join(tmp_path, "weight.npy"), np.ones((6, 8), np.float32))
    a = mesh_render.read_asset(obj, str(tmp_path))
    assert np.array_equal(a["material"][..., 6], rough * 0.5) and a["weight"].shape == (6, 8)
    os.remove(os.path.join(tmp_path, "diffuse_albedo.npy"))
    with pytest.raises(_lib.IronError, match="diffuse_albedo"):
        mesh_render.read_asset(obj, str(tmp_path))
    from PIL import Image
    Image.fromarray((kd * 255).astype(np.uint8)).save(os.path.join(tmp_path, "diffuse_albedo.png"))
    a = mesh_render.read_asset(obj, str(tmp_path))
    assert np.abs(a["material"][..., :3] - kd).max() <= 1.0 / 255.0
    if not torch.cuda.is_available():  # the device half of load() needs a GPU and says so
        with pytest.raises(_lib.IronError, match="GPU"):
            mesh_render.MeshAsset.load(obj, str(tmp_path))
