"""CPU: the numpy restatement of Smart UV project (tests/_uv_oracle.py) against closed-form cases, the host packer's guarantees,
the output guarantees of iron_amd/uv_unwrap.py on a low-resolution S0 mesh, and export_mesh's lattices against the reference's
formulas."""
import numpy as np
import pytest
import torch

import _mc_oracle as M
import _uv_oracle as O

COS66 = float(np.cos(np.radians(66.0)))


def check_guarantees(V, F, r, margin=0.0):
    """The output guarantees of DESIGN.md §13 on an oracle result."""
    uvs, fuv, n, a = r["uvs"], r["face_uvs"], r["normals"], r["area"]
    nd = a > 0
    assert uvs.dtype == np.float32 and (uvs >= 0).all() and (uvs <= 1).all()
    ua = O.signed_uv_area(uvs, fuv)
    assert (ua[nd] > 0).all(), ua[nd].min()
    cosg = (n.astype(np.float64) * r["P"][r["g"]]).sum(1)
    assert (cosg[nd] >= COS66 - 1e-5).all()
    want = r["scale"] ** 2 * (a.astype(np.float64) / 2) * cosg
    # fp32 rounding: every UV coordinate (magnitude <= 1) carries a few roundings of the projection, rotation, offset and scale;
    # 2^-20 per coordinate times the UV perimeter bounds what that does to the area of a small face
    t = np.asarray(uvs, dtype=np.float64)[np.asarray(fuv)]
    perim = sum(np.linalg.norm(t[:, i] - t[:, (i + 1) % 3], axis=1) for i in range(3))
    err = np.abs(ua - want)[nd]
    bound = (1e-3 * want + 2.0 ** -20 * perim)[nd]
    assert (err <= bound).all(), float((err / bound).max())
    lo, hi = O.island_boxes(uvs, fuv, r["labels"], r["K"])
    assert O.boxes_disjoint(lo, hi, margin)
    assert (lo >= margin / 2 - 1e-6).all() and (hi <= 1 - margin / 2 + 1e-6).all()


def test_cube_gives_six_axis_normals_and_six_equal_square_islands():
    V, F = O.cube()
    r = O.smart_uv_project(V, F)
    axes = {tuple(p) for p in np.rint(r["P"]).astype(int)}
    assert len(r["P"]) == 6 and np.array_equal(np.abs(r["P"]), np.rint(np.abs(r["P"])))
    assert axes == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}
    assert r["K"] == 6
    for k in range(6):  # each island is the two triangles of one face
        assert len(np.unique(np.asarray(F)[r["labels"] == k] // 1)) == 4
    bw, bh = r["box"][:, 2] - r["box"][:, 0], r["box"][:, 3] - r["box"][:, 1]
    assert np.all(bw == 1.0) and np.all(bh == 1.0)  # angle 0: the unit squares unrotated
    lo, hi = O.island_boxes(r["uvs"], r["face_uvs"], r["labels"], r["K"])
    size = hi - lo
    assert np.allclose(size, size[0], atol=1e-6, rtol=0) and abs(size[0, 0] - size[0, 1]) < 1e-6
    check_guarantees(V, F, r)


def test_bumpy_height_field_inside_33_degrees_is_one_island():
    V, F = O.height_field()
    n, a = O.face_geometry(V, F)
    assert (n[:, 2] > np.cos(np.radians(33.0))).all()  # every normal within 33 degrees of +z
    r = O.smart_uv_project(V, F)
    assert len(r["P"]) == 1 and r["K"] == 1
    check_guarantees(V, F, r)


def test_two_disjoint_spheres_share_no_island():
    V1, F1 = O.uv_sphere(center=(-2, 0, 0))
    V2, F2 = O.uv_sphere(center=(2, 0, 0))
    V, F = np.concatenate([V1, V2]), np.concatenate([F1, F2 + len(V1)])
    r = O.smart_uv_project(V, F)
    first = set(r["labels"][:len(F1)].tolist())
    second = set(r["labels"][len(F1):].tolist())
    assert first and second and not (first & second)
    check_guarantees(V, F, r)


def test_components_non_manifold_degenerate_edge_and_vertex_contact():
    # a non-manifold fan: three faces on edge (0, 1); with groups 0, 1, 0 the first and last join although not adjacent in the run
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    assert O.components(fan)[1] == 1
    lab, k = O.components(fan, group=[0, 1, 0])
    assert k == 2 and lab[0] == lab[2] != lab[1]
    # [5, 5, 6] and [5, 5, 7] share only their degenerate edge (5, 5); [0, 1, 2] and [0, 3, 4] only a vertex
    lab, k = O.components(np.array([[5, 5, 6], [5, 5, 7], [0, 1, 2], [0, 3, 4]]))
    assert k == 4 and list(lab) == [0, 1, 2, 3]


def test_zero_area_face_takes_projection_zero_and_the_rest_keeps_the_guarantees():
    V, F = O.cube()
    V = np.concatenate([V, np.array([[2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)])
    F = np.concatenate([F, np.array([[8, 9, 10]])])  # collinear: a == 0
    r = O.smart_uv_project(V, F)
    assert r["area"][-1] == 0 and r["g"][-1] == 0
    assert len(r["P"]) == 6
    check_guarantees(V, F, r)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("margin", [0.0, 0.01])
def test_packer_keeps_gaps_and_bounds_on_random_boxes(seed, margin):
    from iron_amd.uv_unwrap import pack_boxes
    g = np.random.default_rng(seed)
    K = int(g.integers(1, 300))
    w = g.uniform(0.01, 1.0, K) ** 2
    h = w * g.uniform(0.05, 1.0, K)
    off, s = pack_boxes(w, h, margin)
    lo, hi = off, off + s * np.stack([w, h], 1)
    assert (lo >= margin / 2 - 1e-12).all() and (hi <= 1 - margin / 2 + 1e-12).all()
    assert O.boxes_disjoint(lo, hi, margin, tol=1e-12)
    if margin == 0:
        assert (w * h).sum() * s * s > 0.4  # a shelf layout of boxes at most 20:1 fills well over a third of the square


def test_packer_refuses_an_infeasible_margin():
    from iron_amd._lib import IronError
    from iron_amd.uv_unwrap import pack_boxes
    K = 10000
    with pytest.raises(IronError, match="10000 islands"):
        pack_boxes(np.full(K, 1e-3), np.full(K, 1e-3), 2.0 / np.sqrt(K))


@pytest.fixture(scope="module")
def s0_low():
    from oracle import iron_ref as R
    from iron_amd import scenes
    from _util import cpu_sd
    res = 40
    sd = cpu_sd(scenes.build_networks("S0")["sdf_network"])
    x = np.linspace(-1, 1, res).astype(np.float32)
    X = np.stack(np.meshgrid(x, x, x, indexing="ij"), -1).reshape(-1, 3)
    with torch.no_grad():
        u = -R.sdf_forward(sd, R.SDFSpec(), torch.from_numpy(X))[:, 0].numpy().reshape(res, res, res)
    v, f = M.marching_cubes(u)
    return (v / (res - 1) * 2 - 1).astype(np.float32), f


def test_s0_low_resolution_output_guarantees_and_packing_floor(s0_low):
    V, F = s0_low
    r = O.smart_uv_project(V, F)
    check_guarantees(V, F, r)
    bw, bh = r["box"][:, 2] - r["box"][:, 0], r["box"][:, 3] - r["box"][:, 1]
    eff = float((bw.astype(np.float64) * bh).sum() * r["scale"] ** 2)
    assert eff >= 0.70, eff  # measured 0.771 (20 islands, 3576 faces at 40^3)
    r2 = O.smart_uv_project(V, F)
    assert np.array_equal(r["uvs"], r2["uvs"]) and np.array_equal(r["face_uvs"], r2["face_uvs"])


def test_export_mesh_lattices_follow_the_reference_formulas():
    from iron_amd.export_mesh import _aligned_axes
    ax = O.grid_uniform_axes(100)
    assert len(ax[0]) == 100 and ax[0][0] == -1.0 and ax[0][-1] == 1.0
    g = np.random.default_rng(0)
    for s in range(3):
        scale = np.array([1.0, 1.0, 1.0])
        scale[s] = 0.3
        pts = torch.from_numpy((g.uniform(-1, 1, (500, 3)) * scale).astype(np.float32))
        axes, _, short = _aligned_axes(pts, 64, 0.1)
        want, want_s = O.grid_axes(pts.numpy(), 64)
        assert short == want_s == s and len(axes[s]) == 64
        for i in range(3):
            assert np.array_equal(axes[i], want[i])
