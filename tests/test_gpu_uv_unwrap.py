"""GPU: Smart UV project and face connectivity on the HIP kernels (csrc/uvunwrap.hip, iron_amd.uv_unwrap) against the numpy
restatement (tests/_uv_oracle.py): parity on the closed-form cases and on S0 at 128^3, the output guarantees and determinism on S0 at
512^3, errors, and iron_amd.export_uv (OBJ round trip, in place, the command line)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _uv_oracle as O
from test_uv_oracle import check_guarantees

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda", 0)


def run(V, F, **kw):
    from iron_amd.uv_unwrap import smart_uv_project
    uv, fuv = smart_uv_project(torch.from_numpy(np.asarray(V, np.float32)).to(dev()), torch.from_numpy(np.asarray(F)).to(dev()), **kw)
    return uv.cpu().numpy(), fuv.cpu().numpy()


def s0_mesh(res):
    from iron_amd import scenes
    from iron_amd.mesh import extract_geometry_gpu
    sdf = scenes.build_networks("S0")["sdf_network"].cuda()
    with torch.no_grad():
        v, f = extract_geometry_gpu(torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), res, 0.0, lambda p: -sdf.sdf(p))
    return v.float(), f


def parity(V, F, exact_margins=True):
    """GPU output == oracle: projection normals within 1e-5, assignments / islands / face_uvs equal, UVs within 1e-5."""
    from iron_amd.uv_unwrap import face_components
    r = O.smart_uv_project(V, F)
    if exact_margins:  # the oracle's decisions are clear of fp32 rounding by more than 1e-5
        mg = r["margins"]
        for k in ("cone", "stop", "assign"):
            assert mg[k] > 1e-5, (k, mg)
    uv, fuv = run(V, F)
    assert np.array_equal(fuv, r["face_uvs"])
    assert uv.shape == r["uvs"].shape and float(np.abs(uv - r["uvs"]).max()) <= 1e-5
    lab, k = face_components(torch.from_numpy(np.asarray(V, np.float32)).to(dev()), torch.from_numpy(np.asarray(F)).to(dev()),
                             group=torch.from_numpy(r["g"]).to(dev()))
    assert k == r["K"] and np.array_equal(lab.cpu().numpy(), r["labels"])
    return r, uv, fuv


def test_parity_cube_height_field_spheres_and_degenerate_face():
    V, F = O.cube()
    parity(V, F)
    parity(*O.height_field())
    V1, F1 = O.uv_sphere(center=(-2, 0, 0))
    V2, F2 = O.uv_sphere(center=(2, 0, 0))
    # the spheres are symmetric: exact ties in n.p, which both sides break by index with identical fp32 arithmetic
    r, uv, _ = parity(np.concatenate([V1, V2]), np.concatenate([F1, F2 + len(V1)]), exact_margins=False)
    assert np.array_equal(uv, r["uvs"])
    Vd = np.concatenate([V, np.array([[2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)])
    parity(Vd, np.concatenate([F, np.array([[8, 9, 10]])]))


def test_components_on_the_device_match_the_rules():
    from iron_amd.uv_unwrap import face_components
    V = torch.zeros((8, 3), device=dev())
    V[:, 0] = torch.arange(8, device=dev()).float()
    V[:, 1] = torch.arange(8, device=dev()).float() ** 2  # no three points collinear (irrelevant to connectivity)
    fan = torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]], device=dev())
    assert face_components(V, fan)[1] == 1
    lab, k = face_components(V, fan, group=torch.tensor([0, 1, 0], device=dev()))
    assert k == 2 and lab.tolist() == [0, 1, 0]
    lab, k = face_components(V, torch.tensor([[5, 5, 6], [5, 5, 7], [0, 1, 2], [0, 3, 4]], device=dev()))
    assert k == 4 and lab.tolist() == [0, 1, 2, 3]


@pytest.fixture(scope="module")
def s0_128():
    v, f = s0_mesh(128)
    return v.cpu().numpy(), f.cpu().numpy()


def test_parity_s0_128(s0_128):
    V, F = s0_128
    # at ~1e5 faces some face always lies within 1e-5 of a threshold; the oracle sums the projection normals in the kernels' order,
    # so the arithmetic agrees bitwise and the margins are reported, not required
    r, uv, fuv = parity(V, F, exact_margins=False)
    print("S0 128^3: %d faces, %d normals, %d islands, margins %s" % (len(F), len(r["P"]), r["K"], r["margins"]))
    assert np.array_equal(uv, r["uvs"])


@pytest.fixture(scope="module")
def s0_512():
    v, f = s0_mesh(512)
    from iron_amd.uv_unwrap import smart_uv_project
    stats = {}
    a = smart_uv_project(v, f, stats=stats)
    b = smart_uv_project(v, f)
    return v, f, a, b, stats


def test_s0_512_guarantees_and_bitwise_determinism(s0_512):
    v, f, (uv, fuv), (uv2, fuv2), stats = s0_512
    assert torch.equal(uv, uv2) and torch.equal(fuv, fuv2)
    print("S0 512^3:", stats)
    V, F = v.cpu().numpy(), f.cpu().numpy()
    n, a = O.face_geometry(V, F)
    P, _ = O.projections(n, a)
    g, _ = O.assign(n, a, P)
    labels, K = O.components(F, g)
    assert K == stats["n_islands"] and len(P) == stats["n_normals"]
    r = dict(uvs=uv.cpu().numpy(), face_uvs=fuv.cpu().numpy(), normals=n, area=a, P=P, g=g, labels=labels, K=K, scale=stats["scale"])
    check_guarantees(V, F, r)


def test_errors_and_empty_mesh():
    from iron_amd._lib import IronError
    V, F = O.cube()
    Fb = F.copy()
    Fb[3, 1] = len(V)
    with pytest.raises(IronError):
        run(V, Fb)
    Vn = V.copy()
    Vn[2, 1] = np.nan
    with pytest.raises(IronError):
        run(Vn, F)
    uv, fuv = run(V, np.zeros((0, 3), np.int64))
    assert uv.shape == (0, 2) and fuv.shape == (0, 3)


def _obj_lines(path, tag):
    return [l for l in open(path).read().splitlines() if l.startswith(tag + " ")]


def test_export_uv_round_trip_in_place_and_command_line(tmp_path, s0_128):
    from iron_amd.export_materials import read_obj
    from iron_amd.export_mesh import _write_obj_vf
    from iron_amd.export_uv import export_uv
    V, F = s0_128
    src = str(tmp_path / "mesh.obj")
    _write_obj_vf(src, V, F)
    v_lines = _obj_lines(src, "v")
    out = str(tmp_path / "out.obj")
    export_uv(src, out)
    assert _obj_lines(out, "v") == v_lines
    v2, t2, f2, ft2 = read_obj(out)
    assert np.array_equal(f2, F) and np.array_equal(v2, V)
    uv, fuv = run(V, F)
    assert np.array_equal(t2, uv) and np.array_equal(ft2, fuv)
    assert not _obj_lines(out, "vn")
    export_uv(src, src)  # in place, as render_surface.py calls it
    assert open(src).read() == open(out).read()
    cli = str(tmp_path / "cli.obj")
    _write_obj_vf(cli, V, F)
    r = subprocess.run([sys.executable, "-m", "iron_amd.export_uv", "--background", cli, cli], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(cli).read() == open(out).read()
    with pytest.raises(AssertionError):
        export_uv(src, str(tmp_path / "x.ply"))
