"""GPU: marching cubes on gfx950 (csrc/mcubes.hip, iron_amd.mesh) against the numpy restatement (tests/_mc_oracle.py), its
closedness at full size, and extract_geometry without PyMCubes (models/renderer.py:34-42, 455-462)."""
import sys

import numpy as np
import pytest
import torch

import _mc_oracle as O
from iron_amd import mc_table

pytestmark = pytest.mark.gpu


def _hip(u_np, threshold=0.0):
    from iron_amd.mesh import marching_cubes
    v, t = marching_cubes(torch.from_numpy(np.ascontiguousarray(u_np)).cuda(), threshold)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and t.dtype == torch.int64 and v.is_cuda and t.is_cuda
    return v.cpu().numpy(), t.cpu().numpy()


def _same(u_np, threshold=0.0):
    v, t = _hip(u_np, threshold)
    rv, rt = O.marching_cubes(u_np, threshold)
    assert v.shape == rv.shape and t.shape == rt.shape, (v.shape, rv.shape, t.shape, rt.shape)
    assert np.array_equal(t, rt)
    if len(v):
        assert np.abs(v - rv).max() <= 1e-6
    return v, t


def test_sphere_64_matches_oracle():
    v, t = _same(O.sphere(64, 25.0))
    assert len(t) > 20000
    n_edges, n_good = O.edge_check(t)
    assert n_good == n_edges


@pytest.mark.parametrize("shape,threshold,seed", [((33, 40, 47), 0.0, 0), ((17, 9, 64), 0.0, 1), ((33, 40, 47), 0.37, 2),
                                                  ((5, 70, 3), -0.2, 3), ((65, 64, 66), 0.0, 4)])
def test_noise_fields_match_oracle(shape, threshold, seed):
    """White noise: about a third of the faces are ambiguous.  (65, 64, 66) has 1073 blocks of lattice points: two scan levels."""
    u = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    _same(u, threshold)


def test_nan_counts_as_below():
    u = np.random.default_rng(7).standard_normal((20, 21, 22)).astype(np.float32)
    u[np.random.default_rng(8).random(u.shape) < 0.05] = np.nan
    v, _ = _same(u)
    assert np.isfinite(v).all()


def test_all_single_cell_cases_match_oracle():
    rng = np.random.default_rng(11)
    for case in range(256):
        u = np.empty((2, 2, 2), np.float32)
        for c, (dx, dy, dz) in enumerate(mc_table.CORNERS):
            mag = np.float32(rng.uniform(0.1, 2.0))
            u[dx, dy, dz] = mag if (case >> c) & 1 else -mag
        v, t = _same(u)
        assert len(t) == len(mc_table.TABLE[case])


def test_empty_meshes():
    for shape in [(1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 3, 3), (4, 0, 4)]:
        v, t = _hip(np.ones(shape, np.float32))
        assert v.shape == (0, 3) and t.shape == (0, 3)
    for val in (1.0, -1.0):
        v, t = _hip(np.full((9, 10, 11), val, np.float32))
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_refuses_cpu_and_bad_inputs():
    from iron_amd._lib import IronError
    from iron_amd.mesh import marching_cubes
    with pytest.raises(IronError):
        marching_cubes(torch.zeros(4, 4, 4))
    with pytest.raises(IronError):
        marching_cubes(torch.zeros(4, 4, device="cuda"))
    with pytest.raises(IronError):
        marching_cubes(torch.zeros(4, 4, 4, device="cuda", dtype=torch.float64))


def _closed_on_gpu(t: torch.Tensor, n_verts: int) -> bool:
    a = t.reshape(-1)
    b = t[:, [1, 2, 0]].reshape(-1)
    key = torch.minimum(a, b) * n_verts + torch.maximum(a, b)
    sign = torch.where(a < b, 1, -1)
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    s = torch.zeros_like(uniq).index_add_(0, inv, sign)
    return bool(((cnt == 2) & (s == 0)).all())


def test_sphere_512_closed_and_deterministic():
    from iron_amd.mesh import marching_cubes
    n, r = 512, 200.0
    g = torch.arange(n, dtype=torch.float32, device="cuda") - (n - 1) / 2.0
    u = r - torch.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    v1, t1 = marching_cubes(u)
    v2, t2 = marching_cubes(u)
    torch.cuda.synchronize()
    assert len(t1) > 1_000_000
    assert torch.equal(t1, t2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32))
    assert int(t1.min()) == 0 and int(t1.max()) == len(v1) - 1
    assert _closed_on_gpu(t1, len(v1))
    v0, v1_, v2_ = (v1[t1[:, i]].double() for i in range(3))
    vol = float((v0 * torch.cross(v1_, v2_, dim=1)).sum() / 6.0)
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 1e-3
    d = (v1.double() - (n - 1) / 2.0).norm(dim=1)
    assert float((d - r).abs().max()) < 0.05


def _s0_sdf():
    from iron_amd import scenes
    return scenes.build_networks("S0")["sdf_network"].cuda()


def _check_mesh(verts, tris, sdf, lo, hi, res):
    assert isinstance(verts, np.ndarray) and isinstance(tris, np.ndarray)
    assert verts.dtype == np.float64 and tris.dtype == np.int64 and verts.shape[1] == 3 and tris.shape[1] == 3
    assert len(tris) > 1000
    assert (verts >= np.asarray(lo) - 1e-9).all() and (verts <= np.asarray(hi) + 1e-9).all()  # world coordinates
    cell = float(max((np.asarray(hi) - np.asarray(lo)) / (res - 1)))
    with torch.no_grad():
        s = sdf.sdf(torch.from_numpy(verts).float().cuda()).abs().max().item()
    assert s <= cell, (s, cell)
    # edges away from the grid boundary are shared by exactly two triangles, in opposite directions
    idx = np.round((verts - np.asarray(lo)) / (np.asarray(hi) - np.asarray(lo)) * (res - 1), 6)
    inner = ((idx > 0) & (idx < res - 1)).all(axis=1)
    keep = inner[tris].all(axis=1)
    n_edges, n_good = O.edge_check(tris[keep])
    on_boundary = n_edges - n_good
    assert keep.all() and on_boundary == 0  # S0's surface (radius ~0.5) lies well inside [-1, 1]^3


def test_extract_geometry_without_mcubes(monkeypatch):
    from iron_amd.renderer import extract_geometry
    monkeypatch.setitem(sys.modules, "mcubes", None)
    sdf = _s0_sdf()
    lo, hi, res = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 128
    verts, tris = extract_geometry(torch.tensor(lo), torch.tensor(hi), res, 0.0, lambda p: -sdf.sdf(p))
    _check_mesh(verts, tris, sdf, lo, hi, res)
    # normals point outward: u = -sdf is above inside
    v = verts[tris]
    assert np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() > 0


def test_neus_renderer_extract_geometry_without_mcubes(monkeypatch):
    from iron_amd.mesh import extract_fields_gpu, marching_cubes
    from iron_amd.renderer import NeuSRenderer
    monkeypatch.setitem(sys.modules, "mcubes", None)
    sdf = _s0_sdf()
    r = NeuSRenderer(None, sdf, None, None, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=0.0)
    lo, hi, res = torch.tensor([-1.0, -1.1, -0.9]), torch.tensor([1.0, 0.9, 1.1]), 128
    verts, tris = r.extract_geometry(lo, hi, resolution=res, threshold=0.0)
    _check_mesh(verts, tris, sdf, lo.numpy(), hi.numpy(), res)
    # the same triangles as marching cubes on the host-copied field of the reference's extract_fields
    from iron_amd.renderer import extract_fields
    u = extract_fields(lo, hi, res, lambda p: -sdf.sdf(p))
    rv, rt = O.marching_cubes(u, 0.0)
    assert np.array_equal(tris, rt)
    ref = rv.astype(np.float64) / (res - 1.0) * (hi - lo).numpy()[None] + lo.numpy()[None]
    assert np.abs(verts - ref).max() <= 1e-6
    ug = extract_fields_gpu(lo, hi, res, lambda p: -sdf.sdf(p))
    assert np.array_equal(ug.cpu().numpy(), u)
    gv, gt = marching_cubes(ug)
    assert np.array_equal(gt.cpu().numpy(), tris)
