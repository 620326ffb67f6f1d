"""GPU: iron_amd.export_mesh (models/export_mesh.py without skimage / trimesh) on analytic SDFs and on S0, and the whole export
chain export_mesh -> export_uv (in place) -> export_materials with a position-map check of the baked xyz texture."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RES = 128


def sphere(p, c=(0.0, 0.0, 0.0), r=0.5):
    return torch.linalg.norm(p - torch.tensor(c, device=p.device, dtype=p.dtype), dim=-1) - r


def capsule(p, a=(-0.5, -0.4, -0.3), b=(0.45, 0.35, 0.3), r=0.2):
    a = torch.tensor(a, device=p.device, dtype=p.dtype)
    b = torch.tensor(b, device=p.device, dtype=p.dtype)
    t = (((p - a) @ (b - a)) / ((b - a) @ (b - a))).clamp(0, 1)
    return torch.linalg.norm(p - (a + t[:, None] * (b - a)), dim=-1) - r


@pytest.mark.parametrize("name", ["sphere", "capsule"])
def test_vertices_lie_on_the_analytic_surface_and_near_the_reference_extraction(tmp_path, name):
    from iron_amd.export_materials import read_obj
    from iron_amd.export_mesh import export_mesh
    from iron_amd.mesh import extract_geometry_gpu
    from iron_amd.mesh_distance import chamfer_distance
    fn = sphere if name == "sphere" else capsule
    path = str(tmp_path / "mesh.obj")
    out = export_mesh(fn, path, resolution=RES)
    assert out is not None and os.path.exists(path)
    h = out["spacing"]
    assert out["shape"][out["shortest_axis"]] == RES
    v, _, f, _ = read_obj(path)
    assert len(f) == out["faces"].shape[0] > 0
    d = fn(torch.from_numpy(v).double().cuda()).abs().max().item()
    assert d <= 0.5 * h, (d, h)
    with torch.no_grad():
        rv, rf = extract_geometry_gpu(torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), RES, 0.0, lambda p: -fn(p))
    cd = chamfer_distance(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), rv.float(), rf)
    assert cd <= h, (cd, h)


def test_no_file_without_a_sign_change_and_far_floater_is_cut(tmp_path):
    from iron_amd.export_materials import read_obj
    from iron_amd.export_mesh import export_mesh
    calls = {"n": 0}

    def vanishing(p):  # a sphere on the 100^3 lattice, then positive everywhere: the aligned lattice sees no sign change
        calls["n"] += p.shape[0]
        return sphere(p) if calls["n"] <= 100 ** 3 else torch.ones(p.shape[0], device=p.device)

    path = str(tmp_path / "none.obj")
    assert export_mesh(vanishing, path, resolution=64) is None and not os.path.exists(path)

    def with_floater(p):
        return torch.minimum(sphere(p), sphere(p, c=(0.85, 0.85, 0.85), r=0.06))

    path = str(tmp_path / "floater.obj")
    export_mesh(with_floater, path, resolution=64)
    v = read_obj(path)[0]
    assert np.linalg.norm(v, axis=1).max() < 0.7  # only the big sphere: the floater lies outside the padded frame


def test_models_import_line_resolves():
    import iron_amd
    iron_amd.install_as_models()
    from models.export_mesh import export_mesh, export_mesh_no_translation  # noqa: F401
    import iron_amd.export_mesh as E
    assert export_mesh is E.export_mesh and export_mesh_no_translation is E.export_mesh_no_translation


def test_chain_export_mesh_export_uv_export_materials(tmp_path):
    from iron_amd import scenes
    from iron_amd.export_materials import export_materials, read_obj
    from iron_amd.export_mesh import export_mesh
    from iron_amd.export_uv import export_uv
    from iron_amd.rendering_func import MaterialPredictor
    from iron_amd.texture_bake import sample_surface_gpu
    from iron_amd.uv_unwrap import face_components
    nets = {k: n.cuda() for k, n in scenes.build_networks("S0").items()}
    sdf_fn = lambda x: nets["sdf_network"](x)[..., 0]  # the driver's sdf_fn (render_surface.py:420)
    path = str(tmp_path / "mesh.obj")
    with torch.no_grad():
        export_mesh(sdf_fn, path, resolution=256)
    export_uv(path, path)
    v, t, f, ft = read_obj(path)
    assert len(ft) == len(f) > 0
    W = 1024
    out_dir = str(tmp_path / "out")
    res = export_materials(path, MaterialPredictor(nets["sdf_network"], nets), out_dir, texture_H=W, texture_W=W, seed=3)
    for n in ("xyz.png", "diffuse_albedo.png", "specular_albedo.png", "roughness.png", "mesh.mtl"):
        assert os.path.exists(os.path.join(out_dir, n)), n
    xyz = res["xyz"]
    # position map: a sample whose texel lies >= 3 texels inside its island's box finds its own position in that texel
    V, F, T, FT = (torch.from_numpy(a).cuda() for a in (v, f, t, ft))
    pts, uv, fi = sample_surface_gpu(V, F, T, FT, 200000, 11, return_face_idx=True)
    T3 = torch.cat([T, torch.zeros_like(T[:, :1])], 1)
    lab, K = face_components(T3, FT)  # islands = faces joined through shared vts
    tri = T[FT.long()]
    lo = torch.full((K, 2), 2.0, device="cuda").scatter_reduce(0, lab.long()[:, None].expand(-1, 2), tri.min(1).values, "amin")
    hi = torch.full((K, 2), -1.0, device="cuda").scatter_reduce(0, lab.long()[:, None].expand(-1, 2), tri.max(1).values, "amax")
    isl = lab.long()[fi.long()]
    inner = ((uv - lo[isl]) * W >= 3).all(1) & ((hi[isl] - uv) * W >= 3).all(1)
    col = (uv[:, 0] * W).long().clamp(0, W - 1)
    row = (W - uv[:, 1] * W).long().clamp(0, W - 1)
    err = torch.linalg.norm(xyz[row, col] - pts, dim=1)[inner]
    wa = torch.linalg.norm(torch.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]], dim=1), dim=1).sum()
    ta = ((tri[:, 1, 0] - tri[:, 0, 0]) * (tri[:, 2, 1] - tri[:, 0, 1]) - (tri[:, 2, 0] - tri[:, 0, 0]) * (tri[:, 1, 1] - tri[:, 0, 1])).sum()
    texel = float(torch.sqrt(wa / ta)) / W  # world size of a texel (an upper estimate: foreshortening makes uv area smaller)
    frac = float((err <= 5 * texel).float().mean())
    print("chain: %d faces, %d islands, inner samples %d, texel %.3e, within 5 texels %.5f, p99 %.3f texels"
          % (len(f), K, int(inner.sum()), texel, frac, float(torch.quantile(err, 0.99)) / texel))
    assert int(inner.sum()) > 100000
    assert frac >= 0.99, frac
