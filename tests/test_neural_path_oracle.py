"""CPU: the preconditions of tests/test_gpu_neural_path.py, from the oracle alone (tests/_neuralpath_oracle.py): the
paths of the neural relight's interreflections do reach second and third vertices on the test field, and the two-box scene of the
two-integrator test is what that test takes it for."""
import torch

import _envlight_oracle as EO
import _meshrender_oracle as O
import _neuralpath_oracle as NP


def test_the_population_is_not_empty():
    """(16, 3) on the fixture view of bumpy04_s1: the fp64 estimator must reach at least 500 vertices 1 and 100 vertices 2."""
    e = NP.estimate("bumpy04_s1", 16, 3)
    v = e["vertices"]
    print("bumpy04_s1 %d x %d, (16, 3): hits %d, paths at vertex 0 / 1 / 2 / 3: %s; bounce rays %d, hits %d, from the front %d; shadow rays "
          "%d, occluded %d; fp32 against fp64 hit / miss differs on %d bounce rays"
          % (NP.RES, NP.RES, e["hits"], v, e["bounce_rays"], e["bounce_hits"], e["front"], e["shadow_rays"], e["occluded"], e["fp32_flips"]))
    assert v[0] == e["hits"] * 16 and e["hits"] > 300
    assert v[1] >= 500 and v[2] >= 100
    assert 0 < e["occluded"] < e["shadow_rays"]
    assert e["fp32_flips"] <= 1e-3 * e["bounce_rays"] + 1
    tot = e["indirect_diffuse"] + e["indirect_specular"]
    assert torch.isfinite(tot).all() and float(tot.min()) >= 0 and float(tot.max()) > 0
    assert torch.allclose(e["values"].mean(1), tot, rtol=1e-12, atol=0)


def test_convex_field_has_no_interreflection():
    e = NP.estimate("S0", 4, 2)
    assert e["hits"] > 100 and e["bounce_rays"] > 100
    assert e["bounce_hits"] == 0 and e["vertices"][1] == 0
    assert (e["indirect_diffuse"] == 0).all() and (e["indirect_specular"] == 0).all()


def test_origin_rounds_each_step_on_its_own():
    g = torch.Generator().manual_seed(3)
    x, n = torch.randn((1000, 3), generator=g), EO._unit(torch.randn((1000, 3), generator=g, dtype=torch.float64)).float()
    st = NP.vertex(x, n, n, x, x, x[:, 0], dtype=torch.float32)
    o = NP.origin(st, 1e-3, torch.float32)
    assert torch.equal(o, x + torch.tensor(1e-3, dtype=torch.float32) * n)
    exact = x.double() + 1e-3 * n.double()
    assert float((o.double() - exact).abs().max()) <= 2.0 ** -22   # two roundings of numbers below 4


def test_the_crease_scene():
    sc = NP.crease()
    V, F = sc["V"], sc["F"]
    assert F.shape == (24, 3) and sc["material"].shape == (1, 1, 7) and float(V.norm(dim=1).max()) < 0.95   # inside the unit sphere
    # the distance function vanishes on the mesh's vertices that lie on the union's surface and is negative inside
    assert float(NP.crease_sdf(torch.tensor([[0.0, -0.2, 0.0], [-0.5, 0.2, 0.0]], dtype=torch.float64)).max()) < 0
    assert float(NP.crease_sdf(torch.tensor([[0.2, 0.3, 0.1]], dtype=torch.float64))) > 0
    # the probes: four on the floor's top face, four on the wall's inner face, 0.2 .. 0.5 of the slab from the crease
    t, f, _, _ = O.closest_hit(sc["ray_o"], sc["ray_d"], V, F)
    assert (f >= 0).all()
    x = sc["ray_o"] + t[:, None] * sc["ray_d"]
    assert float((x - sc["targets"]).abs().max()) < 1e-6
    ng = EO.geometric_normals(V, F)[f]
    up, right = torch.tensor([0.0, 1, 0], dtype=torch.float64), torch.tensor([1.0, 0, 0], dtype=torch.float64)
    assert torch.allclose(ng[:4], up.expand(4, 3)) and torch.allclose(ng[4:], right.expand(4, 3))
    assert float(NP.crease_sdf(x).abs().max()) < 1e-6
    rec = NP.crease_surface(x, sc["ray_d"])
    assert torch.allclose(rec["normal"], ng)
    floor_from_crease, wall_from_crease = (x[:4, 0] + 0.4) / 0.9, (x[4:, 1] + 0.1) / 0.6
    for s in (floor_from_crease, wall_from_crease):
        assert float(s.min()) > 0.2 - 1e-6 and float(s.max()) < 0.5 + 1e-6
    # every face's normal points away from its box
    NG = EO.geometric_normals(V, F)
    for k in range(24):
        c = V[:8].mean(0) if k < 12 else V[8:].mean(0)
        assert float(torch.dot(NG[k], V[F[k, 0]] - c)) > 0
