"""GPU: point-to-mesh distance over the linear BVH (csrc/meshdist.hip, iron_amd.mesh_distance) against the fp64 brute-force
oracle (tests/_meshdist_oracle.py): the precision contract of DESIGN.md §12, the tie rule, exact self-distance, a 1 M-face mesh,
determinism, the Chamfer metric, errors, and the `python -m iron_amd.eval_mesh` command."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _meshdist_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


def dev():
    return torch.device("cuda", 0)


def field(kind, n, radius=None, period=8.0):
    g = torch.arange(n, dtype=torch.float32, device=dev())
    if kind == "sphere":
        c = g - (n - 1) / 2.0
        r = 0.4 * n if radius is None else radius
        return r - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    w = 2.0 * math.pi / period  # period 8 cells: tools/bench_mesh.py's dense gyroid (21 M faces at 256^3)
    s, co = torch.sin(g * w), torch.cos(g * w)
    return (s[:, None, None] * co[None, :, None] + s[None, :, None] * co[None, None, :] + s[None, None, :] * co[:, None, None]).contiguous()


def mc_mesh(kind, n, radius=None, period=8.0):
    from iron_amd.mesh import marching_cubes
    v, f = marching_cubes(field(kind, n, radius, period))
    assert f.shape[0] > 0
    return v, f


def queries(V, F, n, seed=0, inflate=0.2):
    ref = V[F.reshape(-1)]
    lo, hi = ref.min(0).values, ref.max(0).values
    e = (hi - lo).max()
    g = torch.Generator(device=V.device).manual_seed(seed)
    r = torch.rand((n, 3), generator=g, device=V.device, dtype=torch.float32)
    return (lo - inflate * e) + r * (hi - lo + 2 * inflate * e)


def diag(V, F):
    ref = V[F.reshape(-1)].double()
    return float(torch.linalg.norm(ref.max(0).values - ref.min(0).values))


def check_contract(P, V, F, sq, I, C, upper_from_result=False):
    """distances within 2e-6 * diag of the fp64 minimum, C on face I, |P - C|^2 = sqrD to fp32 rounding."""
    P64, V64, F64 = P.double(), V.double(), F.long()
    D = diag(V, F)
    I = I.long()
    assert (I >= 0).all() and (I < F.shape[0]).all()
    dI, cI = O.point_face_sqr_dist(P64, V64, F64, I)
    ref_d, _, _ = O.point_mesh_squared_distance(P64, V64, F64, upper=dI if upper_from_result else None)
    tol = 2e-6 * D
    assert (torch.sqrt(sq.double()) - torch.sqrt(ref_d)).abs().max().item() <= tol
    assert (torch.sqrt(dI) - torch.sqrt(ref_d)).abs().max().item() <= tol
    # C lies on face I: its fp64 distance to the face, and its barycentric coordinates (the rounding of C's coordinates alone,
    # |C| 2^-24, moves them by up to |C| 2^-24 / h for the face's smallest altitude h: the tolerance adds that)
    C64 = C.double()
    dC, _ = O.point_face_sqr_dist(C64, V64, F64, I)
    assert torch.sqrt(dC).max().item() <= tol
    t = F64[I]
    a, b, c = V64[t[:, 0]], V64[t[:, 1]], V64[t[:, 2]]
    ab, ac, ap = b - a, c - a, C64 - a
    n = torch.cross(ab, ac, dim=-1)
    nn = (n * n).sum(-1)
    longest = torch.stack([(ab * ab).sum(-1), (ac * ac).sum(-1), ((c - b) ** 2).sum(-1)], -1).max(-1).values
    ok = nn > 1e-12 * longest * longest  # not degenerate: barycentrics are defined
    h = torch.sqrt(nn / longest.clamp_min(1e-300))
    w_b = (torch.cross(ap, ac, dim=-1) * n).sum(-1) / nn.clamp_min(1e-300)
    w_c = (torch.cross(ab, ap, dim=-1) * n).sum(-1) / nn.clamp_min(1e-300)
    w_a = 1.0 - w_b - w_c
    btol = 1e-5 + 8 * EPS32 * C64.abs().max(-1).values / h.clamp_min(1e-300)
    for w in (w_a, w_b, w_c):
        assert ((w >= -btol) & (w <= 1 + btol) | ~ok).all()
    pc = ((P64 - C64) ** 2).sum(-1)
    assert ((pc - sq.double()).abs() <= 8 * EPS32 * pc + 1e-37).all()


def run(P, V, F):
    from iron_amd.mesh_distance import MeshBVH
    return MeshBVH(V, F).query(P)


def _small_meshes():
    v, f = O.unit_cube()
    yield "cube", v.float().to(dev()), f.to(dev())
    v, f = O.regular_tetrahedron()
    yield "tetrahedron", v.float().to(dev()), f.to(dev())
    v, f = O.triangle_soup(2000, 0.05, seed=0)
    yield "soup", v.float().to(dev()), f.to(dev())
    v, f = mc_mesh("sphere", 48)
    yield "sphere48", v, f


@pytest.mark.parametrize("name", ["cube", "tetrahedron", "soup", "sphere48"])
def test_against_the_fp64_oracle(name):
    V, F = next((v, f) for n, v, f in _small_meshes() if n == name)
    P = torch.cat([queries(V, F, 3000, seed=1), V])
    sq, I, C = run(P, V, F)
    assert torch.isfinite(sq).all() and torch.isfinite(C).all()
    check_contract(P, V, F, sq, I, C)


def test_corner_tie_goes_to_the_smallest_face_index():
    v, f = O.unit_cube()
    V, F = v.float().to(dev()), f.to(dev())
    P = torch.tensor([[1.25, 1.25, 1.25], [-0.5, -0.5, -0.5]], device=dev())
    sq, I, C = run(P, V, F)
    fl = f.tolist()
    assert I[0].item() == min(k for k in range(12) if 7 in fl[k])
    assert I[1].item() == min(k for k in range(12) if 0 in fl[k])
    assert sq[0].item() == 0.1875 and sq[1].item() == 0.75
    assert torch.equal(C[0].cpu(), torch.tensor([1.0, 1.0, 1.0])) and torch.equal(C[1].cpu(), torch.zeros(3))


@pytest.mark.parametrize("kind,n", [("sphere", 48), ("gyroid", 256)])
def test_vertices_are_at_distance_zero(kind, n):
    V, F = mc_mesh(kind, n)
    used = torch.unique(F.reshape(-1))
    P = V[used]
    sq, I, C = run(P, V, F)
    assert (sq == 0).all()
    assert torch.equal(C, P)


def test_one_million_faces_against_the_oracle_on_the_gpu():
    V, F = mc_mesh("gyroid", 256, period=160.0)
    assert 900_000 < F.shape[0] < 2_000_000
    P = queries(V, F, 4096, seed=7, inflate=0.05)
    sq, I, C = run(P, V, F)
    check_contract(P, V, F, sq, I, C, upper_from_result=True)


def test_build_and_query_are_bitwise_reproducible():
    from iron_amd.mesh_distance import MeshBVH
    V, F = mc_mesh("gyroid", 96)
    P = torch.cat([queries(V, F, 20000, seed=3), V[:5000]])
    a, b = MeshBVH(V, F), MeshBVH(V, F)
    assert torch.equal(a.workspace, b.workspace)
    ra, rb = a.query(P), b.query(P)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    for x, y in zip(ra, a.query(P)):
        assert torch.equal(x, y)


def test_chamfer_of_concentric_spheres():
    from iron_amd.mesh_distance import chamfer_distance, point_mesh_squared_distance
    va, fa = mc_mesh("sphere", 256, radius=80.0)
    vb, fb = mc_mesh("sphere", 256, radius=100.0)
    ab = chamfer_distance(va, fa, vb, fb)
    assert abs(ab - 20.0) <= 0.05
    assert chamfer_distance(vb, fb, va, fa) == ab
    assert chamfer_distance(va, fa, va, fa) == 0.0
    # the combination rule, on the kernel's own distances
    assert math.isclose(O.cal_mesh_err(va, fa, vb, fb, sqr_dist=point_mesh_squared_distance), ab, rel_tol=1e-12)


def test_chamfer_against_the_fp64_restatement():
    from iron_amd.mesh_distance import chamfer_distance
    va, fa = mc_mesh("sphere", 48, radius=15.0)
    vb, fb = mc_mesh("sphere", 48, radius=17.5)
    got = chamfer_distance(va, fa, vb, fb)
    want = O.cal_mesh_err(va.double(), fa, vb.double(), fb)
    assert abs(got - want) <= max(1e-5 * abs(want), 1e-7 * diag(vb, fb))


def test_numpy_and_fp64_in_numpy_out():
    from iron_amd.mesh_distance import point_mesh_squared_distance
    v, f = O.regular_tetrahedron()
    P = np.array([[0.0, 0.0, 0.0], [2.0, 2.0, 2.0]])
    sq, I, C = point_mesh_squared_distance(P, v.numpy(), f.numpy())
    assert sq.dtype == np.float64 and I.dtype == np.int64 and C.dtype == np.float64
    assert abs(sq[0] - 1.0 / 3.0) <= 1e-6 and sq[1] == 3.0 and (C[1] == 1.0).all()
    Pt = torch.tensor(P, device=dev())
    sq2, I2, C2 = point_mesh_squared_distance(Pt, v.to(dev()), f.to(dev()))
    assert sq2.device == Pt.device and sq2.dtype == torch.float64 and I2.dtype == torch.int64
    assert np.array_equal(sq2.cpu().numpy(), sq) and np.array_equal(I2.cpu().numpy(), I)


def test_errors_and_edge_cases():
    from iron_amd._lib import IronError
    from iron_amd.mesh_distance import MeshBVH
    v, f = O.unit_cube()
    V, F = v.float().to(dev()), f.to(dev())
    bad = F.clone()
    bad[5, 1] = V.shape[0]
    with pytest.raises(IronError):
        MeshBVH(V, bad)
    bad = F.clone()
    bad[2, 0] = -1
    with pytest.raises(IronError):
        MeshBVH(V, bad)
    Vn = V.clone()
    Vn[3, 2] = float("nan")
    with pytest.raises(IronError):
        MeshBVH(Vn, F)
    with pytest.raises(IronError):
        MeshBVH(V, F[:0])
    sq, I, C = MeshBVH(V, F).query(torch.zeros((0, 3), device=dev()))
    assert sq.shape == (0,) and I.shape == (0,) and C.shape == (0, 3)
    # unreferenced vertices, even non-finite or far away, do not enter the build
    extra = torch.tensor([[float("nan"), 0.0, 0.0], [1e30, 1e30, 1e30]], device=dev())
    P = queries(V, F, 2000, seed=5)
    want = MeshBVH(V, F).query(P)
    got = MeshBVH(torch.cat([V, extra]), F).query(P)
    for x, y in zip(want, got):
        assert torch.equal(x, y)


def _write_obj(path, v, f):
    with open(path, "w") as fp:
        for p in v.tolist():
            fp.write("v %.9g %.9g %.9g\n" % tuple(p))
        for t in f.tolist():
            fp.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))


def test_eval_mesh_command(tmp_path):
    from iron_amd.export_materials import read_obj
    from iron_amd.mesh_distance import chamfer_distance
    va, fa = mc_mesh("sphere", 48, radius=15.0)
    vb, fb = mc_mesh("sphere", 40, radius=14.0)
    pa, pb = str(tmp_path / "pred.obj"), str(tmp_path / "trgt.obj")
    _write_obj(pa, va.cpu(), fa.cpu())
    _write_obj(pb, vb.cpu(), fb.cpu())
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "iron_amd.eval_mesh", pa, pb], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    v1, _, f1, _ = read_obj(pa)
    v4, _, f4, _ = read_obj(pb)
    assert np.array_equal(v1, va.cpu().numpy())
    want = chamfer_distance(v1, f1, v4, f4)
    assert r.stdout == "\tChamfer_dist:  %s\n" % want
    assert abs(want - chamfer_distance(va, fa, vb, fb)) <= 1e-12
