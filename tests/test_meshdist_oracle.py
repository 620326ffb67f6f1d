"""CPU: the fp64 point-to-mesh oracle (tests/_meshdist_oracle.py) against closed-form answers, and the host side of
iron_amd.mesh_distance / iron_amd.eval_mesh (no CPU path; the reference's names)."""
import inspect
import math

import numpy as np
import pytest
import torch

import _meshdist_oracle as O


def _check(P, V, F, want_d2, want_c=None):
    d, i, c = O.point_mesh_squared_distance(torch.tensor(P, dtype=torch.float64), V, F)
    assert torch.allclose(d, torch.tensor(want_d2, dtype=torch.float64), atol=1e-14, rtol=1e-12), (d, want_d2)
    if want_c is not None:
        assert torch.allclose(c, torch.tensor(want_c, dtype=torch.float64), atol=1e-14)
    # the closest point is on the returned face and at the returned distance
    dd, cc = O.point_face_sqr_dist(torch.tensor(P, dtype=torch.float64), V, F, i)
    assert torch.allclose(dd, d, atol=1e-14)
    return d, i, c


def test_cube_every_region_kind():
    V, F = O.unit_cube()
    P = [[0.5, 0.5, 1.5],    # face interior (above z = 1)
         [1.5, 0.5, 1.5],    # edge x = 1, z = 1
         [1.5, 1.5, 1.5],    # vertex (1, 1, 1)
         [-0.25, 0.3, 0.6],  # face x = 0 from outside
         [0.5, 0.5, 0.2],    # inside, nearest face z = 0
         [0.7, 0.4, 0.5],    # inside, nearest face x = 1
         [1.0, 1.0, 1.0],    # on a vertex
         [1.0, 0.5, 1.0],    # on an edge
         [0.3, 0.4, 1.0]]    # on a face
    want = [0.25, 0.5, 0.75, 0.0625, 0.04, 0.09, 0.0, 0.0, 0.0]
    want_c = [[0.5, 0.5, 1.0], [1.0, 0.5, 1.0], [1.0, 1.0, 1.0], [0.0, 0.3, 0.6], [0.5, 0.5, 0.0], [1.0, 0.4, 0.5],
              [1.0, 1.0, 1.0], [1.0, 0.5, 1.0], [0.3, 0.4, 1.0]]
    _check(P, V, F, want, want_c)


def test_cube_corner_tie_goes_to_the_smallest_face():
    V, F = O.unit_cube()
    d, i, c = _check([[1.25, 1.25, 1.25]], V, F, [3 * 0.0625], [[1.0, 1.0, 1.0]])
    corner = [k for k in range(12) if 7 in F[k].tolist()]
    assert int(i[0]) == min(corner)


def test_regular_tetrahedron():
    V, F = O.regular_tetrahedron()
    P = [[0.0, 0.0, 0.0],       # centre: the inradius 1 / sqrt(3) to every face
         [2.0, 2.0, 2.0],       # beyond vertex (1, 1, 1)
         [-1.0, -1.0, -1.0],    # straight out of the face opposite (1, 1, 1), onto its centroid
         [0.0, 0.0, 1.5]]       # out of the edge (1,1,1)-(-1,-1,1) along +z: nearest point (0, 0, 1)
    want = [1.0 / 3.0, 3.0, 4.0 / 3.0, 0.25]
    want_c = [None, [1.0, 1.0, 1.0], [-1.0 / 3.0, -1.0 / 3.0, -1.0 / 3.0], [0.0, 0.0, 1.0]]
    d, i, c = _check(P, V, F, want)
    for k, w in enumerate(want_c):
        if w is not None:
            assert torch.allclose(c[k], torch.tensor(w, dtype=torch.float64), atol=1e-14)


def test_degenerate_triangles():
    V = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0],     # a point
                      [5.0, 0.0, 0.0], [5.0, 0.0, 0.0], [6.0, 0.0, 0.0],     # two coincident: segment (5..6, 0, 0)
                      [0.0, 5.0, 0.0], [0.0, 6.0, 0.0], [0.0, 5.5, 0.0]],    # collinear, C between A and B
                     dtype=torch.float64)
    F = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    P = [[0.0, 0.0, -2.0], [5.5, 1.0, 0.0], [7.0, 0.0, 0.0], [0.0, 6.5, 0.0], [1.0, 5.25, 0.0]]
    want = [4.0, 1.0, 1.0, 0.25, 1.0]
    want_c = [[0.0, 0.0, 0.0], [5.5, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 6.0, 0.0], [0.0, 5.25, 0.0]]
    d, i, c = _check(P, V, F, want, want_c)
    assert i.tolist() == [0, 1, 1, 2, 2]
    assert torch.isfinite(d).all() and torch.isfinite(c).all()


def test_collinear_with_the_third_vertex_outside():
    V = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [3.0, 0.0, 0.0]], dtype=torch.float64)
    F = torch.tensor([[0, 1, 2]])
    _check([[2.5, 0.0, 1.0], [-1.0, 0.0, 0.0]], V, F, [1.0, 1.0], [[2.5, 0.0, 0.0], [0.0, 0.0, 0.0]])


def test_pruned_oracle_equals_the_full_scan():
    V, F = O.triangle_soup(300, seed=3)
    P = torch.rand((64, 3), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 1.4 - 0.2
    d, i, c = O.point_mesh_squared_distance(P, V, F)
    upper, _ = O.point_face_sqr_dist(P, V, F, torch.randint(0, len(F), (len(P),), generator=torch.Generator().manual_seed(2)))
    d2, i2, c2 = O.point_mesh_squared_distance(P, V, F, upper=upper)
    assert torch.equal(d, d2) and torch.equal(i, i2) and torch.equal(c, c2)


def test_cal_mesh_err_restatement():
    # a cube against the same cube scaled by 2 about its centre: an inner vertex is 1/2 from the outer faces, an outer vertex
    # sqrt(3)/2 from the inner corner
    V, F = O.unit_cube()
    W = (V - 0.5) * 2.0 + 0.5
    assert math.isclose(O.cal_mesh_err(V, F, W, F), 0.5 * (0.5 + math.sqrt(0.75)), rel_tol=1e-14)
    assert O.cal_mesh_err(V, F, V, F) == 0.0


def test_cpu_tensors_are_refused():
    from iron_amd._lib import IronError
    from iron_amd.mesh_distance import MeshBVH, chamfer_distance, point_mesh_squared_distance
    V, F = O.unit_cube()
    with pytest.raises(IronError):
        point_mesh_squared_distance(torch.zeros((4, 3)), V.float(), F)
    with pytest.raises(IronError):
        point_mesh_squared_distance(np.zeros((4, 3)), V.float(), F.numpy())
    with pytest.raises(IronError):
        chamfer_distance(V.float(), F, V.numpy(), F.numpy())
    with pytest.raises(IronError):
        MeshBVH(V, F)


def test_eval_mesh_has_the_reference_interface():
    from iron_amd import eval_mesh
    assert list(inspect.signature(eval_mesh.cal_mesh_err).parameters) == ["va", "fa", "vb", "fb"]
    assert list(inspect.signature(eval_mesh.eval_obj_meshes).parameters) == ["pred_mesh_fpath", "trgt_mesh_fpath"]
    from iron_amd import mesh_distance
    assert list(inspect.signature(mesh_distance.point_mesh_squared_distance).parameters) == ["P", "V", "F"]
