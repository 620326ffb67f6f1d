"""CPU: the fp64 oracle of the environment render (tests/_envlight_oracle.py) against closed forms, the Radiance
.hdr reader and the command line's arguments.  The oracle checks never use the product.
"""
import math
import os

import numpy as np
import pytest
import torch

import _envlight_oracle as EO


def tables():
    from iron_amd.renderer_ggx import load_mts_tables
    return load_mts_tables()


def test_uv_convention_on_the_axes():
    d = torch.tensor([[0.0, 0, -1], [1, 0, 0], [0, 0, 1], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=torch.float64)
    u, v = EO.dir_to_uv(d)
    assert torch.allclose(u[:4], torch.tensor([0.0, 0.25, 0.5, 0.75], dtype=torch.float64), atol=1e-15)
    assert torch.allclose(v, torch.tensor([0.5, 0.5, 0.5, 0.5, 0.0, 1.0], dtype=torch.float64), atol=1e-15)
    back = EO.uv_to_dir(u[:4], v[:4])
    assert float((back - d[:4]).abs().max()) <= 1e-15
    # to_world: a map rotated by R shows at R d what the unrotated map shows at d
    img = torch.rand((4, 8, 3), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    c, s = math.cos(0.7), math.sin(0.7)
    R = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
    q = EO._unit(torch.randn((50, 3), generator=torch.Generator().manual_seed(2), dtype=torch.float64))
    assert torch.equal(EO.EnvOracle(img, R).lookup(q @ R.T), EO.EnvOracle(img).lookup(q))


def test_constant_map_has_the_uniform_density():
    env = EO.EnvOracle(torch.full((16, 32, 3), 0.7, dtype=torch.float64))
    g = torch.Generator().manual_seed(3)
    tx, d, p = env.sample(torch.rand((4000, 2), generator=g, dtype=torch.float64))
    q = EO._unit(torch.randn((4000, 3), generator=g, dtype=torch.float64))
    # P(texel) = sin(theta_row) / sum: against sin(theta(dir)) within the row, so 1 / 4 pi only up to the row's height; the exact
    # statement is P(texel) We He / (2 pi^2 sin) with sum_r sin(pi (r + 1/2) / He) = 1 / sin(pi / 2 He)
    for dirs, pdf in ((d, p), (q, env.pdf(q))):
        r = env.texel_of(dirs)[0]
        row = torch.sin(math.pi * (r.double() + 0.5) / 16) * math.sin(math.pi / 32)
        st = torch.sqrt(dirs[:, 0] ** 2 + dirs[:, 2] ** 2)
        assert float((pdf - row * 16 / (2 * math.pi ** 2 * st)).abs().max()) <= 1e-12
    # and 1 / 4 pi in the limit of thin rows: the ratio sin(row centre) / sin(theta) is 1 +- (pi / 2 He) cot(theta), below 1.7e-3
    # for He = 2048 where |d.y| < 0.9 (at the poles themselves the weight's row-centre sine never converges pointwise)
    fine = EO.EnvOracle(torch.ones((2048, 4, 3), dtype=torch.float64))
    away = q[q[:, 1].abs() < 0.9]
    assert away.shape[0] > 3000 and float((fine.pdf(away) * 4 * math.pi - 1).abs().max()) <= 2e-3
    assert float((env.pdf(d) - p).abs().max()) <= 1e-12  # pdf(sample's direction) is the sample's pdf


def test_density_integrates_to_one():
    img = torch.rand((5, 7, 3), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    img[2] = 0.0
    img[0, 3] = 0.0
    env = EO.EnvOracle(img)
    nu, nv = 7 * 40, 5 * 400
    u = (torch.arange(nu, dtype=torch.float64) + 0.5) / nu
    v = (torch.arange(nv, dtype=torch.float64) + 0.5) / nv
    U, V = torch.meshgrid(u, v, indexing="xy")
    d = EO.uv_to_dir(U.reshape(-1), V.reshape(-1))
    dom = 2 * math.pi ** 2 * torch.sin(math.pi * V.reshape(-1)) / (nu * nv)
    total = float((env.pdf(d) * dom).sum())
    print("sum of pdf x solid angle over %d x %d cells: %.12f" % (nv, nu, total))
    assert abs(total - 1) <= 1e-9  # pdf sin(theta) is constant inside a texel: the midpoint rule is exact up to rounding
    tx = env.sample(torch.rand((20000, 2), generator=torch.Generator().manual_seed(5), dtype=torch.float64))[0]
    assert (env.weight[tx[:, 0], tx[:, 1]] > 0).all()
    black = EO.EnvOracle(torch.zeros((3, 4, 3), dtype=torch.float64))
    tb, db, pb = black.sample(torch.rand((10, 2), dtype=torch.float64))
    assert (pb == 0).all() and torch.isfinite(db).all() and (black.pdf(db) == 0).all()


def test_roughplastic_at_l_equals_v_is_the_colocated_head():
    from oracle import iron_ref as R
    g = torch.Generator().manual_seed(6)
    m = 5000
    n = EO._unit(torch.randn((m, 3), generator=g, dtype=torch.float64))
    v = EO._unit(n + 0.9 * EO._unit(torch.randn((m, 3), generator=g, dtype=torch.float64)))
    kd, ks = torch.rand((m, 3), generator=g, dtype=torch.float64), torch.rand((m, 3), generator=g, dtype=torch.float64)
    rough = torch.rand((m,), generator=g, dtype=torch.float64) * 0.9 + 0.02
    mt, md = tables()
    d, s = EO.roughplastic_point(n, v, v, kd, ks, rough, (mt, md))
    ref = R.ggx_colocated(torch.tensor(1.0, dtype=torch.float64), torch.ones((m, 1), dtype=torch.float64), n, v,
                          {"diffuse_albedo": kd, "specular_albedo": ks, "specular_roughness": rough[:, None]}, mt.double(), md.double())
    keep = EO._dot(n, v) > 1e-3
    es = float(((s - ref["specular_rgb"]).abs() / ref["specular_rgb"].abs().clamp_min(1e-300))[keep].max())
    ed = float(((d - ref["diffuse_rgb"]).abs() / ref["diffuse_rgb"].abs().clamp_min(1e-300))[keep].max())
    print("l = v against ggx_colocated: specular max rel %.3e (kFr's rounding: 7.5e-5), diffuse max rel %.3e" % (es, ed))
    assert int(keep.sum()) > 4000
    assert es <= 2e-4 and ed <= 1e-6
    assert abs(float(EO.fresnel_dielectric_pos(torch.tensor(1.0, dtype=torch.float64))) - 0.0386729) <= 1e-7


def test_diffuse_plane_under_a_constant_map():
    """A diffuse-only plane (normal +y, viewed from 40 degrees) under radiance L: the quadrature over the map against the
    one-dimensional integral 2 pi L int f_d(theta) cos sin dtheta of the same diffuse term."""
    mt, md = tables()
    L, rough = 1.3, 0.4
    env = EO.EnvOracle(torch.full((32, 64, 3), L, dtype=torch.float64))
    n = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    v = torch.tensor([math.sin(0.7), math.cos(0.7), 0.0], dtype=torch.float64)
    kd, ks = torch.tensor([0.8, 0.5, 0.2], dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    Vp = torch.tensor([[-9.0, 0, -9], [9, 0, -9], [9, 0, 9], [-9, 0, 9]], dtype=torch.float64)
    Fp = torch.tensor([[0, 2, 1], [0, 3, 2]])
    x = torch.zeros(3, dtype=torch.float64)
    d, s = EO.quadrature(env, x, n, n, v, kd, ks, rough, 0, Vp, Fp, 1e-4, (mt, md), sub=8)
    th = (torch.arange(200000, dtype=torch.float64) + 0.5) / 200000 * (math.pi / 2)
    l = torch.stack([torch.sin(th), torch.cos(th), torch.zeros_like(th)], -1)
    k = th.shape[0]
    fd, _ = EO.roughplastic_point(n[None].expand(k, 3), v[None].expand(k, 3), l, kd[None].expand(k, 3), ks[None].expand(k, 3),
                                  torch.full((k,), rough, dtype=torch.float64), (mt, md))
    closed = 2 * math.pi * L * (fd * torch.sin(th)[:, None]).sum(0) * (math.pi / 2 / k)
    rel = float(((d - closed).abs() / closed).max())
    print("diffuse plane: quadrature %s, one-dimensional integral %s, max rel %.3e" % (d.tolist(), closed.tolist(), rel))
    assert (s == 0).all()
    assert rel <= 2e-3  # the table is piecewise constant in cos: the 256-row midpoint rule resolves its steps to this


def test_random_numbers_are_on_the_odd_24_bit_grid():
    u = EO.env_rand(7, np.arange(1000)[:, None], np.arange(64)[None, :], 1)
    k = u * 2.0 ** 24
    assert ((k == np.rint(k)) & (k.astype(np.int64) % 2 == 1) & (u > 0) & (u < 1)).all()
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    # uniform: the mean and the share below 1/2 within 5 standard errors (sigma 1 / sqrt(12 n) and 1 / (2 sqrt n))
    assert abs(u.mean() - 0.5) < 5 / math.sqrt(12 * u.size) and abs((u < 0.5).mean() - 0.5) < 5 / (2 * math.sqrt(u.size))
    assert not np.array_equal(u, EO.env_rand(8, np.arange(1000)[:, None], np.arange(64)[None, :], 1))
    assert float(EO.env_rand(0, 0, 0, 0)) == float(EO.env_rand(0, 0, 0, 0))


def test_visibility_scenes_are_stable_in_fp32():
    """The scenes of the GPU test: the oracle's fp32 visibility against its fp64 one disagrees only at small margins, and rarely."""
    for name in ("floor", "cube"):
        sc = EO.scene(name)
        x, n, ng, v, face, w = EO.oracle_probe_rays(sc, seed=11)
        v64, margin, _ = EO.visibility(x, n, ng, v, w, face, sc["V"], sc["F"], sc["eps_d"])
        v32, _, _ = EO.visibility(x, n, ng, v, w, face, sc["V"], sc["F"], sc["eps_d"], dtype=torch.float32)
        bad = v64 != v32
        print("%s: %d shadow rays, fp32 against fp64 visibility differs on %d, of which margin >= 1e-4: %d"
              % (name, w.shape[0], int(bad.sum()), int((bad & (margin >= EO.VIS_MARGIN)).sum())))
        assert int((bad & (margin >= EO.VIS_MARGIN)).sum()) == 0
        assert float(bad.double().mean()) <= EO.VIS_SHARE


def test_texel_flips_of_fp32_inputs_stay_under_the_cap():
    for name, img in EO.env_maps().items():
        u = EO.sample_inputs()
        e64, e32 = EO.EnvOracle(img), EO.EnvOracle(img, dtype=torch.float32)
        t64 = e64.sample(u)[0]
        near = e64.boundary_gap <= 4
        print("%s: share of u within 4 fp32 ulps of a CDF boundary %.2e" % (name, float(near.double().mean())))
        assert float(near.double().mean()) <= EO.FLIP_SHARE
        assert torch.equal(t64, e32.sample(u)[0])  # the CDFs are compared in fp64 in both: the choice itself does not depend on dtype


def test_hdr_round_trip(tmp_path):
    from iron_amd.envmap import read_envmap, read_hdr
    g = np.random.default_rng(9)
    img = (g.random((13, 40, 3)) * np.exp2(g.integers(-12, 12, (13, 40, 1)))).astype(np.float32)
    img[3, 5:25] = img[3, 5]      # long runs
    img[4, :] = 0.0               # black pixels: exponent byte 0
    img[5, 7] = [1e4, 0.1, 0.1]   # a hot pixel loses its small channels to the shared exponent
    img[6, :, 1] = 255.6 / 256    # a mantissa that rounds up to 256
    rgbe = EO.encode_rgbe(img)
    for rle in (False, True):
        p = os.path.join(tmp_path, "probe_%d.hdr" % rle)
        EO.write_hdr(p, rgbe, rle)
        got = read_hdr(p)
        assert got.shape == img.shape and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - img) / np.maximum(img.astype(np.float64).max(-1, keepdims=True), 1e-300)
        print("hdr round trip (rle %s): %d bytes, max error / largest channel %.3e (bound 1/256 = %.3e)"
              % (rle, os.path.getsize(p), float(err.max()), 1 / 256))
        assert float(err.max()) <= 1 / 256
        assert (got[4] == 0).all()
        assert np.array_equal(read_envmap(p), got)
    assert os.path.getsize(os.path.join(tmp_path, "probe_1.hdr")) < os.path.getsize(os.path.join(tmp_path, "probe_0.hdr")) + 13 * 4 + 13 * 8
    np.save(os.path.join(tmp_path, "probe.npy"), img)
    assert np.array_equal(read_envmap(os.path.join(tmp_path, "probe.npy")), img)
    with open(os.path.join(tmp_path, "bad.hdr"), "wb") as fp:
        fp.write(b"not a picture")
    from iron_amd._lib import IronError
    with pytest.raises(IronError):
        read_hdr(os.path.join(tmp_path, "bad.hdr"))


def test_render_asset_envmap_arguments():
    from iron_amd import render_asset
    base = ["--mesh", "m.obj", "--textures", "t", "--cam_dict", "c.json", "--out", "o"]
    a = render_asset.parse_args(base)
    assert a.envmap is None and a.light == 20.0 and a.spp_axis == 1
    a = render_asset.parse_args(base + ["--envmap", "probe.hdr", "--n-light", "32", "--n-brdf", "16", "--seed", "5", "--background"])
    assert (a.envmap, a.n_light, a.n_brdf, a.seed, a.background) == ("probe.hdr", 32, 16, 5, True)
    a = render_asset.parse_args(base + ["--envmap", "probe.npy"])
    assert (a.n_light, a.n_brdf, a.seed, a.background) == (64, 64, 0, False)
    for bad in (["--background"], ["--n-light", "8"], ["--envmap", "p.hdr", "--n-light", "0", "--n-brdf", "0"],
                ["--envmap", "p.hdr", "--n-brdf", "-1"]):
        with pytest.raises(SystemExit):
            render_asset.parse_args(base + bad)
    img = np.array([[[0.0, 0.5, 4.0]]], dtype=np.float32)
    assert render_asset.to8b_gamma(img).tolist() == [[[0, int(0.5 ** (1 / 2.2) * 255), 255]]]
