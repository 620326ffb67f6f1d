"""CPU: the numpy restatement of the texture bake (tests/_bake_oracle.py) against G21, the reference's own
models/export_materials.py (tests/golden/make_golden_bake.py), and the host side of iron_amd.export_materials."""
import importlib
import json
import sys

import numpy as np
import pytest

import _bake_oracle as O
from _util import golden
from test_surface_signatures import _compatible


@pytest.fixture(scope="module")
def g21():
    return golden("g21_bake.npz")


def test_g21_mesh_rebuilds_bit_for_bit(g21):
    v, f, t, ft = O.g21_mesh()
    assert O.sha256(v, f, t, ft) == str(g21["sha256__mesh"])
    assert len(f) == 2 * O.G21_N ** 2 + 1
    assert O.face_areas(v, f)[-1] == 0.0


@pytest.mark.parametrize("k", [0, 1])
def test_counts_and_points_match_the_reference(g21, k):
    v, f, t, ft = O.g21_mesh()
    p = "sample%d__" % k
    n = int(g21[p + "n"])
    ceil_c = O.ceil_counts(v, f, n)
    assert np.array_equal(ceil_c, g21[p + "ceil_counts"])
    counts = O.counts_after_removal(ceil_c, g21[p + "drawn"])
    assert np.array_equal(counts, g21[p + "counts"])
    assert counts[-1] == 0 and counts.sum() == len(g21[p + "points"]) >= n
    face_idx = np.repeat(np.arange(len(f)), counts)
    P, Q = O.points_from_draws(v, f, t, ft, face_idx, g21[p + "r"])
    assert np.array_equal(P, g21[p + "points"]) and np.array_equal(Q, g21[p + "uv"])


def test_splat_restatement_matches_the_reference(g21):
    H, W = O.G21_HW
    sums = np.zeros((H * W, 11))
    for c in range(3):
        vals = np.concatenate([g21["splat%d__pcd" % c], g21["splat%d__material" % c]], axis=1)
        sums += O.splat_sums(g21["splat%d__uv" % c], vals, H, W)
        if c in (0, 2):
            ref_w = g21["splat_after%d__weight" % c].reshape(-1)
            assert np.abs(sums[:, -1] - ref_w).max() <= 1e-6 * (1 + ref_w.max())
            ref = np.concatenate([g21["splat_after%d__xyz" % c], g21["splat_after%d__material" % c]], axis=-1).reshape(H * W, -1)
            assert np.abs(sums[:, :-1] - ref).max() <= 1e-6 * (1 + np.abs(ref).max())
    # the edge grid reaches wrapped taps on both sides and drops others
    i, lab, _ = O.splat_taps(g21["splat1__uv"], H, W)
    assert len(lab) < 5 * len(g21["splat1__uv"])
    assert (lab % W == W - 1).any() and (lab % W == 0).any()


def test_obj_round_trip(tmp_path):
    from iron_amd.export_materials import read_obj, write_obj
    v, f, t, ft = O.g21_mesh()
    path = str(tmp_path / "m.obj")
    write_obj(path, v, t, f, ft)
    v2, t2, f2, ft2 = read_obj(path)
    assert np.array_equal(v2, v) and np.array_equal(t2, t) and np.array_equal(f2, f) and np.array_equal(ft2, ft)
    # quads fan-triangulated, negative indices, v//n and plain v faces
    with open(path, "w") as fp:
        fp.write("usemtl ./m.mtl\n\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
                 "f 1/1/1 2/2/1 3/3/1 4/4/1\nf -4/-4 -2/-2 -1/-1\n")
    v3, t3, f3, ft3 = read_obj(path)
    assert v3.shape == (4, 3) and t3.shape == (4, 2)
    assert f3.tolist() == [[0, 1, 2], [0, 2, 3], [0, 2, 3]] and ft3.tolist() == f3.tolist()
    with open(path, "w") as fp:
        fp.write("v 0 0 0\nv 1 0 0\nv 1 1 0\nf 1//1 2//1 3//1\n")
    _, _, f4, ft4 = read_obj(path)
    assert f4.tolist() == [[0, 1, 2]] and ft4.shape == (0, 3)


def test_ply_header_and_payload(tmp_path):
    from iron_amd.export_materials import write_ply_points
    pts = np.arange(12, dtype=np.float32).reshape(4, 3)
    col = np.arange(16, dtype=np.uint8).reshape(4, 4)
    path = str(tmp_path / "p.ply")
    write_ply_points(path, pts, col)
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    assert head.decode("ascii").splitlines() == [
        "ply", "format binary_little_endian 1.0", "element vertex 4", "property float x", "property float y", "property float z",
        "property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    rec = np.frombuffer(body, dtype=[("p", "<f4", 3), ("c", "u1", 4)])
    assert np.array_equal(rec["p"], pts) and np.array_equal(rec["c"], col)


def test_mtl_text_and_usemtl_line_are_the_references(g21):
    from iron_amd.export_materials import MTL_TEXT
    assert MTL_TEXT == str(g21["mtl_text"])
    assert "usemtl ./{}\n\n".format("mesh.obj"[:-4] + ".mtl") == str(g21["usemtl_line"])


NOT_BUILT = {"Groupby": "host group-by helper of the reference's splat; the splat kernel (csrc/texbake.hip) replaces it"}


def test_export_materials_signatures_are_compatible_with_the_reference(g21):
    import iron_amd.export_materials as EM
    sigs = json.loads(str(g21["signatures_json"]))
    assert set(sigs) == {"sample_surface", "accumulate_splat_material", "loadmesh_and_checkuv", "export_materials", "to8b", "Groupby"}
    for name, entry in sigs.items():
        if name in NOT_BUILT:
            assert not hasattr(EM, name)
            continue
        assert entry["type"] == "function"
        assert _compatible(entry["params"], getattr(EM, name)) is None, (name, _compatible(entry["params"], getattr(EM, name)))
    x = np.array([-0.5, 0.0, 0.5, 1.0, 2.0], dtype=np.float32)
    assert np.array_equal(EM.to8b(x), np.clip(x * 255.0, 0.0, 255.0).astype(np.uint8))


def test_install_as_models_resolves_the_export_import_line():
    import iron_amd
    import iron_amd.export_materials
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    try:
        for k in saved:
            del sys.modules[k]
        iron_amd.install_as_models()
        ns = {}
        exec("from models.export_materials import export_materials, sample_surface, accumulate_splat_material", ns)
        assert ns["export_materials"] is iron_amd.export_materials.export_materials
        assert ns["sample_surface"] is iron_amd.export_materials.sample_surface
        assert importlib.import_module("models.export_materials") is iron_amd.export_materials
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved)
