"""CPU: the fp64 oracle of the path integrator (tests/_envpath_oracle.py) against itself (its estimator against its
nested quadrature, exact zeros where no light can be reflected twice), the preconditions of tests/test_gpu_envpath.py from the
oracle alone, and the host-side surface of the feature (command line, refusals).  Never runs a kernel."""
import functools

import pytest
import torch

import _envlight_oracle as EO
import _envpath_oracle as PO

CELLS, SUB = 16, 2  # the nested quadrature's grids here: its refinement change is part of every comparison below


@functools.lru_cache(maxsize=None)
def tables():
    from iron_amd.renderer_ggx import load_mts_tables
    return load_mts_tables()


@functools.lru_cache(maxsize=None)
def hot():
    return EO.EnvOracle(EO.hot_map())


def test_estimator_agrees_with_the_nested_quadrature():
    q = PO.probe_quadrature("cpu", CELLS, SUB)
    quad = q["indirect_diffuse"] + q["indirect_specular"]
    o, d = PO.probe_rays()
    N = 4096
    r = PO.estimate(hot(), PO.scene("corner_face"), "corner_face", tables(), o, d, torch.arange(8) * 37 + 11, N, 2, 9)
    assert r["hit"].all() and (q["face"][:4] < 2).all() and (q["face"][4:] >= 2).all()  # four on the floor, four on the wall
    est = r["indirect_diffuse"] + r["indirect_specular"]
    se = r["values"].std(1, unbiased=True) / N ** 0.5
    z = ((est - quad).abs() - q["change"]).clamp_min(0) / se
    print("estimate / nested quadrature (channel 0) %s; largest deviation beyond the refinement change %.2f standard errors; standard error / "
          "quadrature median %.3e; refinement change / quadrature max %.3e"
          % ([round(float(a), 4) for a in est[:, 0] / quad[:, 0]], float(z.max()), float((se / quad).median()), float((q["change"] / quad).max())))
    assert (se > 0).all() and float(z.max()) <= 5.0
    # the lobes apart: each against its own quadrature, under the total's refinement change
    for key in ("indirect_diffuse", "indirect_specular"):
        assert float((((r[key] - q[key]).abs() - q["change"]).clamp_min(0) / se).max()) <= 5.0, key


def test_inner_quadrature_is_the_direct_quadrature():
    """inner_direct, vectorised over vertices, is EO.quadrature at each of them"""
    q = PO.probe_quadrature("cpu", CELLS, SUB)
    sc, st = PO.scene("corner_face"), q["st0"]
    many = PO.inner_direct(hot(), sc, st, tables(), 2)
    for p in (0, 5):
        one = sum(EO.quadrature(hot(), st["x"][p], st["n"][p], st["ng"][p], st["v"][p], st["kd"][p], st["ks"][p], st["rough"][p],
                                int(st["face"][p]), sc["V"], sc["F"], sc["eps_d"], tables(), sub=2))
        assert float(((many[p] - one).abs() / one).max()) <= 1e-12


@pytest.mark.parametrize("name", PO.ZERO_SCENES)
def test_no_interreflection_is_exactly_zero(name):
    sc = PO.scene(name)
    o, d = EO.scene_rays(sc)
    r = PO.estimate(hot(), sc, name, tables(), o, d, torch.arange(o.shape[0]), 16, 3, PO.SEED)
    assert 100 < int(r["hit"].sum()) < o.shape[0] - 100
    assert (r["indirect_diffuse"] == 0).all() and (r["indirect_specular"] == 0).all() and (r["values"] == 0).all()
    if name == "floor":  # bounce rays from the floor do reach the occluder, whose underside faces away: absorbed
        assert int((r["reached"] >= 2).sum()) > 50 and int((r["reached"] == -1).sum()) > 50
    else:
        assert r["reached"].numel() > 1000 and (r["reached"] == -1).all()


def test_corner_has_interreflections_worth_testing():
    q = PO.probe_quadrature("cpu", CELLS, SUB)
    share = (q["indirect_diffuse"] + q["indirect_specular"] - q["change"]) / q["direct"]
    print("nested quadrature, indirect / direct per probe pixel and channel:\n%s" % share)
    assert int((share.min(1).values >= 0.10).sum()) >= 6


@pytest.mark.parametrize("name,setting", [(n, s) for n in PO.DUMP_SCENES for s in PO.SETTINGS] + [(n, PO.SETTINGS[1]) for n in ("cube", "sphere")])
def test_rays_of_the_gpu_tests_stay_clear_of_edges(name, setting):
    """the caps under which tests/test_gpu_envpath.py may excuse a face or a visibility that fp32 decides the other way"""
    sc = PO.scene(name)
    o, d = EO.scene_rays(sc)
    r = PO.estimate(hot(), sc, name, tables(), o, d, torch.arange(o.shape[0]), setting[0], setting[1], PO.SEED)
    near = float((r["bounce_margin"] < PO.EDGE_MARGIN).double().mean())
    shadow = float((r["shadow_margin"] < EO.VIS_MARGIN).double().mean()) if r["shadow_margin"].numel() else 0.0
    print("%s %s: bounce rays %d, within %g of an edge %.2e; shadow rays %d, within %g: %.2e"
          % (name, setting, r["bounce_margin"].numel(), PO.EDGE_MARGIN, near, r["shadow_margin"].numel(), EO.VIS_MARGIN, shadow))
    assert r["bounce_margin"].numel() > 1000
    assert near <= PO.EDGE_SHARE and shadow <= EO.VIS_SHARE


def test_command_line_and_refusals():
    from iron_amd import _lib, render_asset
    from iron_amd.mesh_render import check_path_args, render_asset_env
    base = "--mesh m.obj --textures t --cam_dict c.json --out o".split()
    a = render_asset.parse_args(base + "--envmap e.npy --max-depth 3 --n-paths 8".split())
    assert (a.max_depth, a.n_paths) == (3, 8)
    a = render_asset.parse_args(base + ["--envmap", "e.npy"])
    assert (a.max_depth, a.n_paths) == (1, 64)  # the default is today's render
    for extra in (["--max-depth", "2"], ["--n-paths", "8"],                                    # need --envmap
                  ["--envmap", "e.npy", "--max-depth", "0"], ["--envmap", "e.npy", "--max-depth", "9"],
                  ["--envmap", "e.npy", "--max-depth", "2", "--n-paths", "0"], ["--envmap", "e.npy", "--max-depth", "2", "--n-paths", "65537"]):
        with pytest.raises(SystemExit):
            render_asset.parse_args(base + extra)
    for kw in (dict(max_depth=0), dict(max_depth=9), dict(max_depth=2.5), dict(max_depth=2, n_paths=0), dict(max_depth=2, n_paths=(1 << 16) + 1)):
        with pytest.raises(_lib.IronError):
            render_asset_env(None, None, None, **kw)  # refused before anything is touched
    check_path_args(1, 1), check_path_args(8, 1 << 16), check_path_args(2, 64, indirect=True)
    with pytest.raises(_lib.IronError):
        check_path_args(1, 64, indirect=True)  # the indirect kernel itself does not run at depth 1
