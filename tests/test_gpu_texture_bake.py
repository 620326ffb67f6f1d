"""GPU: the material texture bake on gfx950 (csrc/texbake.hip, iron_amd.texture_bake, iron_amd.export_materials) against G21 and
the numpy restatement (tests/_bake_oracle.py), its determinism, and a full 2048^2 bake of scene S0."""
import os

import numpy as np
import pytest
import torch

import _bake_oracle as O
from _util import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g21():
    return golden("g21_bake.npz")


@pytest.mark.parametrize("k", [0, 1])
def test_explicit_draw_sampling_matches_g21(g21, k):
    from iron_amd.texture_bake import sample_surface_explicit
    v, f, t, ft = O.g21_mesh()
    p = "sample%d__" % k
    face_idx = np.repeat(np.arange(len(f)), g21[p + "counts"])
    r = g21[p + "r"]
    P, Q = sample_surface_explicit(v, f, t, ft, face_idx, r[:, 0], r[:, 1])
    assert np.abs(P.cpu().numpy() - g21[p + "points"]).max() <= 1e-6
    assert np.abs(Q.cpu().numpy() - g21[p + "uv"]).max() <= 1e-6


@pytest.mark.parametrize("k", [0, 1])
def test_counts_follow_the_reference_rule(g21, k):
    from iron_amd.texture_bake import sample_surface_gpu
    v, f, t, ft = O.g21_mesh()
    p = "sample%d__" % k
    n = int(g21[p + "n"])
    x = n * O.face_areas(v, f).astype(np.float64)
    near = (np.abs(x - np.round(x)) <= 1e-5 * np.maximum(np.abs(x), 1.0)) & (x > 0)
    assert not near.any()
    pts, uv, fi, ceil_c, cnt = sample_surface_gpu(v, f, t, ft, n, seed=7, round=k, return_face_idx=True, return_counts=True)
    ceil_c, cnt, fi = ceil_c.cpu().numpy(), cnt.cpu().numpy(), fi.cpu().numpy()
    assert np.array_equal(ceil_c, g21[p + "ceil_counts"])
    removed = ceil_c - cnt
    assert set(np.unique(removed)) <= {0, 1} and (removed[ceil_c == 0] == 0).all()
    floor_num = int(ceil_c.sum()) - n
    assert 0 < removed.sum() <= floor_num
    assert cnt[-1] == 0  # the zero-area face
    assert len(pts) == cnt.sum() >= n
    assert np.array_equal(fi, np.repeat(np.arange(len(f)), cnt))  # ordered by face
    assert np.isfinite(pts.cpu().numpy()).all() and np.isfinite(uv.cpu().numpy()).all()


def _grid_mesh(F):
    """The first F faces of a planar vertex grid (jittered, fixed seed; two triangles per cell), about one face in ten made
    degenerate by repeating a vertex index, and one shared UV triangle -> (v, f, uvs, face_uvs, degenerate mask)."""
    side = 726 if F > 1058 else 24  # 2 * 725^2 = 1 051 250 faces; 2 * 23^2 = 1058
    rng = np.random.default_rng(1234)
    ii, jj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    v = np.stack([ii, jj, np.zeros_like(ii)], -1).reshape(-1, 3).astype(np.float32)
    v[:, :2] += rng.uniform(-0.3, 0.3, (side * side, 2)).astype(np.float32)
    a = (ii[:-1, :-1] * side + jj[:-1, :-1]).reshape(-1)
    f = np.stack([np.stack([a, a + side, a + 1], -1), np.stack([a + 1, a + side, a + side + 1], -1)], 1).reshape(-1, 3)[:F].copy()
    assert len(f) == F
    degenerate = rng.random(F) < 0.1
    degenerate[0] = False  # the one-face mesh keeps its area
    f[degenerate, 2] = f[degenerate, 1]
    t = np.array([[0, 0], [1, 0], [0, 1]], dtype=np.float32)
    return v, f, t, np.tile(np.array([[0, 1, 2]]), (F, 1)), degenerate


@pytest.mark.parametrize("F", [1, 1023, 1024, 1025, 1051250])
def test_counts_and_offsets_across_the_scan_boundaries(F):
    """The pair scan (csrc/pair_scan.hip) at its block boundaries, through the bake: level lengths [1, 1], [1023, 1], [1024, 1],
    [1025, 2, 1] and [1051250, 1027, 2, 1] (three scan levels).  The sample offsets are the exclusive scan of the counts, so the
    face of every sample must be repeat_interleave(arange(F), counts); the count rule is test_counts_follow_the_reference_rule's."""
    from iron_amd.texture_bake import sample_surface_gpu
    v, f, t, ft, degenerate = _grid_mesh(F)
    n = min(3 * F, 1 << 24)
    run = lambda: sample_surface_gpu(v, f, t, ft, n, seed=13, return_face_idx=True, return_counts=True)  # noqa: E731
    pts, uv, fi, ceil_c, cnt = first = run()
    assert torch.equal(fi.long(), torch.repeat_interleave(torch.arange(F, device=fi.device), cnt.long()))  # ordered by face
    assert len(pts) == len(uv) == int(cnt.sum()) >= n
    removed = (ceil_c - cnt).cpu().numpy()
    ceil_np = ceil_c.cpu().numpy()
    assert set(np.unique(removed)) <= {0, 1} and (removed[ceil_np == 0] == 0).all()
    assert 0 <= int(removed.sum()) <= int(ceil_np.sum()) - n
    assert (cnt.cpu().numpy()[degenerate] == 0).all() and (ceil_np[~degenerate] > 0).all()
    assert all(torch.equal(x, y) for x, y in zip(first, run()))


def test_seeded_sampling_is_reproducible_and_seed_dependent():
    from iron_amd.texture_bake import sample_surface_gpu
    v, f, t, ft = O.g21_mesh()
    a = sample_surface_gpu(v, f, t, ft, 20000, seed=3)
    b = sample_surface_gpu(v, f, t, ft, 20000, seed=3)
    c = sample_surface_gpu(v, f, t, ft, 20000, seed=4)
    d = sample_surface_gpu(v, f, t, ft, 20000, seed=3, round=1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for other in (c, d):
        m = min(len(a[0]), len(other[0]))
        assert not torch.equal(a[0][:m], other[0][:m])


def test_two_triangles_split_and_barycentric_means():
    from iron_amd.texture_bake import sample_surface_gpu
    # areas 1 : 3
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [10, 0, 0], [13, 0, 0], [10, 1, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    t = np.array([[0, 0], [1, 0], [0, 1]], dtype=np.float32)
    ft = np.array([[0, 1, 2], [0, 1, 2]])
    n = 10 ** 7
    pts, uv, fi = sample_surface_gpu(v, f, t, ft, n, seed=11, return_face_idx=True)
    fi = fi.cpu().numpy()
    N = len(fi)
    n0 = int((fi == 0).sum())
    sd = np.sqrt(N * 0.25 * 0.75)
    assert abs(n0 - N * 0.25) <= 4 * sd + 1, (n0, N)
    # uv = b1 * (1, 0) + b2 * (0, 1): barycentric means 1/3 each, sd of one coordinate is sqrt(1/18)
    m = uv.double().mean(dim=0).cpu().numpy()
    assert np.abs(m - 1.0 / 3.0).max() <= 4 * np.sqrt(1.0 / 18.0 / N)


def _splat_g21(g21, dev_calls=(0, 1, 2)):
    from iron_amd.texture_bake import SplatAccumulator
    H, W = O.G21_HW
    acc = SplatAccumulator(H, W, 7, max_samples=10 ** 5)
    for c in dev_calls:
        acc.add(torch.from_numpy(g21["splat%d__pcd" % c]).cuda(), torch.from_numpy(g21["splat%d__uv" % c]).cuda(),
                torch.from_numpy(g21["splat%d__material" % c]).cuda())
    return acc


def test_splat_parity_with_g21_over_three_calls(g21):
    acc = _splat_g21(g21)
    xyz, mat, w = (x.cpu().numpy() for x in acc.resolve())
    rw = g21["splat_after2__weight"]
    assert np.abs(w - rw).max() <= 1e-6 * (1 + rw.max())
    assert (np.abs(w - rw) <= 1e-6 * (1 + rw)).all()
    den = rw[..., None] + np.float32(1e-10)
    rx = g21["splat_after2__xyz"] / den
    rm = g21["splat_after2__material"] / den
    assert np.abs(xyz - rx).max() <= 1e-6
    assert np.abs(mat - rm).max() <= 1e-6
    assert ((w > 0) == (rw > 0)).all()


def test_accumulate_splat_material_mirror_updates_in_place(g21):
    from iron_amd.export_materials import accumulate_splat_material
    H, W = O.G21_HW
    xyz = np.zeros((H, W, 3), np.float32)
    mat = np.zeros((H, W, 7), np.float32)
    wgt = np.zeros((H, W), np.float32)
    for c in range(3):
        out = accumulate_splat_material(xyz, mat, wgt, g21["splat%d__pcd" % c], g21["splat%d__uv" % c].copy(), g21["splat%d__material" % c])
        assert out[0] is xyz and out[1] is mat and out[2] is wgt
        if c == 0:
            assert np.abs(wgt - g21["splat_after0__weight"]).max() <= 1e-5
    assert np.abs(wgt - g21["splat_after2__weight"]).max() <= 1e-5
    assert np.abs(mat - g21["splat_after2__material"]).max() <= 1e-5


def test_splat_is_bitwise_reproducible(g21):
    a = _splat_g21(g21).acc
    b = _splat_g21(g21).acc
    assert torch.equal(a, b)


@pytest.mark.parametrize("bad", [float("nan"), 1e30])
def test_bad_material_value_raises_range(g21, bad):
    from iron_amd import _lib
    from iron_amd.texture_bake import SplatAccumulator
    m = torch.from_numpy(g21["splat0__material"]).cuda().clone()
    m[17, 3] = bad
    acc = SplatAccumulator(*O.G21_HW, 7, max_samples=10 ** 5)
    acc.add(torch.from_numpy(g21["splat0__pcd"]).cuda(), torch.from_numpy(g21["splat0__uv"]).cuda(), m)
    with pytest.raises(_lib.IronError, match="not finite or too large"):
        acc.resolve()


# ---- S0: a full bake ---------------------------------------------------------------------------------------------------------
RES, TEX, GUTTER = 128, 2048, 3


def s0_mesh(res=RES):
    from iron_amd import scenes
    from iron_amd.mesh import extract_geometry_gpu
    sdf = scenes.build_networks("S0")["sdf_network"].cuda()
    lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
    with torch.no_grad():
        v, f = extract_geometry_gpu(torch.tensor(lo), torch.tensor(hi), res, 0.0, lambda p: -sdf.sdf(p))
    return sdf, v.float(), f


@pytest.fixture(scope="module")
def s0_bake():
    from iron_amd import scenes
    from iron_amd.rendering_func import MaterialPredictor
    from iron_amd.texture_bake import bake_materials
    sdf, v, f = s0_mesh()
    assert (TEX / np.ceil(np.sqrt(len(f)))) - 2 * GUTTER >= 2, "atlas cells too small for the gutter"
    uvs, fuv = O.atlas(len(f), TEX, GUTTER)
    nets = {k: n.cuda() for k, n in scenes.build_networks("S0").items()}
    pred = MaterialPredictor(nets["sdf_network"], nets)
    runs = [bake_materials(v, f, uvs, fuv, pred, TEX, TEX, n_rounds=2, n_samples=2_000_000, seed=5) for _ in range(2)]
    return dict(sdf=sdf, v=v, f=f, uvs=uvs, fuv=fuv, pred=pred, runs=runs)


def test_s0_bake_is_bitwise_identical_on_two_runs(s0_bake):
    (a, b) = s0_bake["runs"]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int((a[2] > 0).sum()) > 100000


def test_s0_bake_matches_an_fp64_index_add_restatement(s0_bake):
    from iron_amd.rendering_func import query_materials
    from iron_amd.texture_bake import sample_surface_gpu
    v, f, uvs, fuv, pred = (s0_bake[k] for k in ("v", "f", "uvs", "fuv", "pred"))
    xyz, mat, w = s0_bake["runs"][0]
    H = W = TEX
    sums = torch.zeros((H * W, 11), dtype=torch.float64, device="cuda")
    for r in range(2):
        pts, uv = sample_surface_gpu(v, f, uvs, fuv, 2_000_000, 5, round=r)
        m = query_materials(pred, pts)
        vals = torch.cat([pts, m, torch.ones_like(pts[:, :1])], 1).double()
        i, lab, wt = O.splat_taps(uv.cpu().numpy(), H, W)
        i, lab = torch.from_numpy(i).cuda(), torch.from_numpy(lab).cuda()
        sums.index_add_(0, lab, torch.from_numpy(wt).cuda().double()[:, None] * vals[i])
    rw = sums[:, -1].float()
    ref = sums[:, :-1].float() / (rw[:, None] + 1e-10)
    assert float((w.reshape(-1) - rw).abs().max()) <= 1e-6 * (1 + float(rw.max()))
    got = torch.cat([xyz, mat], -1).reshape(H * W, -1)
    assert float((got - ref).abs().max()) <= 1e-6


def test_s0_texels_lie_on_the_surface_and_hold_its_materials(s0_bake):
    from iron_amd.rendering_func import query_materials
    sdf, v, f = s0_bake["sdf"], s0_bake["v"], s0_bake["f"]
    xyz, mat, w = s0_bake["runs"][0]
    keep = w > 0
    x = xyz[keep]
    cell = 2.0 / (RES - 1)
    # a texel is a convex combination of samples on ONE triangle (the gutters keep triangles apart), and a point of a marching-
    # cubes triangle lies in a cell with a sign change: |sdf| <= L * sqrt(3) * cell, with the S0 SDF's Lipschitz constant ~1
    with torch.no_grad():
        s = sdf.sdf(x).abs().max().item()
    bound = 1.5 * np.sqrt(3.0) * cell
    assert s <= bound, (s, bound)
    # materials: |m(mean x) - mean m(x)| <= L_m * max distance of a texel's samples from their mean <= L_m * max triangle edge
    tri = v[f]
    edge = float(torch.stack([(tri[:, 0] - tri[:, 1]).norm(dim=1), (tri[:, 1] - tri[:, 2]).norm(dim=1),
                              (tri[:, 2] - tri[:, 0]).norm(dim=1)]).max())
    g = torch.Generator(device="cuda").manual_seed(0)
    p = x[torch.randint(0, len(x), (20000,), device="cuda", generator=g)]
    d = torch.nn.functional.normalize(torch.randn(p.shape, device="cuda", generator=g), dim=1) * 1e-2
    lip = float(((query_materials(s0_bake["pred"], p + d) - query_materials(s0_bake["pred"], p)).abs().max(dim=1).values
                 / 1e-2).max())
    err = float((query_materials(s0_bake["pred"], x) - mat[keep]).abs().max())
    assert err <= 2.0 * lip * edge + 1e-5, (err, lip, edge)


def test_export_materials_end_to_end(tmp_path):
    from PIL import Image
    from iron_amd import scenes
    from iron_amd.export_materials import MTL_TEXT, export_materials, read_obj, write_obj
    from iron_amd.rendering_func import MaterialPredictor
    sdf, v, f = s0_mesh(48)
    uvs, fuv = O.atlas(len(f), 512, GUTTER)
    obj = str(tmp_path / "mesh.obj")
    write_obj(obj, v.cpu().numpy(), uvs, f.cpu().numpy(), fuv)
    head = open(obj).read()
    nets = {k: n.cuda() for k, n in scenes.build_networks("S0").items()}
    out_dir = str(tmp_path / "out")
    res = export_materials(obj, MaterialPredictor(nets["sdf_network"], nets), out_dir, texture_H=512, texture_W=512, seed=1)
    names = ["check_uvmap.ply", "check_uvmap.png", "xyz.png", "diffuse_albedo.png", "specular_albedo.png", "roughness.png", "mesh.mtl"]
    for n in names:
        assert os.path.exists(os.path.join(out_dir, n)), n
    for stem in ("xyz", "diffuse_albedo", "specular_albedo", "roughness"):
        assert os.path.exists(os.path.join(out_dir, stem + ".exr")) or os.path.exists(os.path.join(out_dir, stem + ".npy"))
    to8b = lambda x: np.clip(x * 255.0, 0.0, 255.0).astype(np.uint8)
    xyz, mat = res["xyz"].cpu().numpy(), res["material"].cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, "xyz.png"))), to8b(xyz * 0.5 + 0.5))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, "diffuse_albedo.png"))), to8b(mat[..., :3]))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, "specular_albedo.png"))), to8b(mat[..., 3:6]))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, "roughness.png"))), to8b(mat[..., 6]))
    assert open(os.path.join(out_dir, "mesh.mtl")).read() == MTL_TEXT
    assert open(obj).read() == "usemtl ./mesh.mtl\n\n" + head
    assert len(read_obj(obj)[2]) == len(f)
