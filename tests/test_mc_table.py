"""CPU: the marching-cubes case table (iron_amd/mc_table.py -> csrc/mc_table.h) and the meshes it gives, through the numpy
restatement of csrc/mcubes.hip (tests/_mc_oracle.py)."""
import numpy as np
import pytest

from iron_amd import mc_table
import _mc_oracle as O


def test_committed_header_is_the_generator_output():
    with open(mc_table.HEADER_PATH) as f:
        assert f.read() == mc_table.render_header(), "csrc/mc_table.h is stale: run python -m iron_amd.mc_table"


def test_table_rows_fit_the_generated_maximum():
    assert mc_table.MAX_TRIS == max(len(t) for t in mc_table.TABLE)
    assert "constexpr int kMcMaxTris = %d;" % mc_table.MAX_TRIS in mc_table.render_header()
    assert len(mc_table.TABLE[0]) == 0 and len(mc_table.TABLE[255]) == 0
    for c in range(256):  # complementary cases cross the same edges
        assert {e for t in mc_table.TABLE[c] for e in t} == {e for t in mc_table.TABLE[255 - c] for e in t}


@pytest.mark.parametrize("case", range(256))
def test_single_cell_vertices_lie_on_crossed_edges(case):
    rng = np.random.default_rng(case)
    u = np.empty((2, 2, 2), np.float32)
    for c, (dx, dy, dz) in enumerate(mc_table.CORNERS):
        mag = np.float32(rng.uniform(0.1, 2.0))
        u[dx, dy, dz] = mag if (case >> c) & 1 else -mag
    verts, tris = O.marching_cubes(u)
    crossed = set()
    for e in range(12):
        o = mc_table.EDGE_ORIGIN[e]
        q = list(o)
        q[mc_table.EDGE_AXIS[e]] += 1
        if (u[o] > 0) != (u[tuple(q)] > 0):
            crossed.add((o, mc_table.EDGE_AXIS[e]))
    assert len(verts) == len(crossed)
    found = set()
    for v in verts:
        frac = [a for a in range(3) if v[a] != np.round(v[a])]
        assert len(frac) == 1, v  # strictly inside one lattice edge (|u| >= 0.1 at the corners)
        a = frac[0]
        o = tuple(int(np.floor(v[i])) for i in range(3))
        found.add((o, a))
        u0, u1 = u[o], u[tuple(o[i] + (i == a) for i in range(3))]
        assert abs(float(v[a] - o[a]) - float(-u0 / (u1 - u0))) < 1e-6
    assert found == crossed
    assert len(tris) == len(mc_table.TABLE[case])
    if len(verts):
        assert set(np.unique(tris)) == set(range(len(verts)))  # every crossed edge is used


@pytest.mark.parametrize("seed", range(40))
def test_random_fields_give_closed_orientable_meshes(seed):
    rng = np.random.default_rng(1000 + seed)
    u = np.full((8, 8, 8), -1.0, np.float32)  # below-threshold border: the surface cannot leave the grid
    u[1:7, 1:7, 1:7] = rng.standard_normal((6, 6, 6)).astype(np.float32)
    verts, tris = O.marching_cubes(u)
    assert len(tris) > 0
    n_edges, n_good = O.edge_check(tris)
    assert n_good == n_edges  # every undirected edge in exactly 2 triangles, traversed in opposite directions
    assert O.volume(verts, tris) > 0  # right-hand normals point out of the above region


def test_ambiguous_faces_are_resolved_the_same_way_by_both_cells():
    # a checkerboard makes every face ambiguous
    i, j, k = np.meshgrid(*[np.arange(7)] * 3, indexing="ij")
    u = np.where((i + j + k) % 2 == 0, 1.0, -1.0).astype(np.float32)
    u[[0, -1], :, :] = u[:, [0, -1], :] = u[:, :, [0, -1]] = -1.0
    verts, tris = O.marching_cubes(u)
    n_edges, n_good = O.edge_check(tris)
    assert n_good == n_edges
    # separating the above corners turns every interior above point into its own closed octahedron-like blob
    assert O.volume(verts, tris) > 0


def test_sphere_volume_by_divergence_theorem():
    r = 25.0
    verts, tris = O.marching_cubes(O.sphere(64, r))
    n_edges, n_good = O.edge_check(tris)
    assert n_good == n_edges
    vol = O.volume(verts, tris)
    exact = 4.0 / 3.0 * np.pi * r ** 3
    assert vol > 0 and abs(vol / exact - 1.0) < 0.01


def test_threshold_nan_and_degenerate_inputs():
    u = O.sphere(12, 4.0)
    v0, t0 = O.marching_cubes(u, 0.5)
    v1, t1 = O.marching_cubes(u - np.float32(0.5), 0.0)
    assert np.array_equal(t0, t1)
    nan = u.copy()
    nan[6, 6, :] = np.nan  # NaN is below: a tunnel through the blob, still closed
    v, t = O.marching_cubes(nan)
    n_edges, n_good = O.edge_check(t)
    assert n_good == n_edges and np.isfinite(v).all()
    for shape in [(1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 3, 3)]:
        v, t = O.marching_cubes(np.ones(shape, np.float32))
        assert v.shape == (0, 3) and t.shape == (0, 3)
    for val in (1.0, -1.0):
        v, t = O.marching_cubes(np.full((4, 5, 6), val, np.float32))
        assert len(v) == 0 and len(t) == 0
