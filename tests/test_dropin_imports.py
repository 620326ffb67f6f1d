"""CPU: the import lines of the reference's own callers resolve after iron_amd.install_as_models().

tests/golden/reference_import_lines.json (make_import_lines.py: names only, read with `ast`) lists every
`from models.<module> import <names>` of render_surface.py, render_nir.py, render_volume.py, model_volume.py, model_bed.py and
utils/process_routine.py.  Modules this build mirrors must resolve to iron_amd; `models.helper` and `models.dataset`, which it does
not mirror, must keep resolving to the CALLER's files -- install_as_models() lays the mirror over a real `models` package when one
is importable instead of hiding it behind a made-up one.  Also: the three names the earlier build left out (choose_optmizer,
choose_renderer_func, NeRFdual) against the recorded signatures and the reference's constructor arithmetic."""
import importlib
import importlib.util
import inspect
import json
import os
import sys

import pytest
import torch

from _util import GOLDEN

MIRRORED = ("raytracer", "renderer_ggx", "rendering_func", "fields", "embedder", "renderer", "network_conf", "image_losses",
            "export_materials", "export_mesh")
CALLERS_OWN = ("helper", "dataset")


def _lines():
    return json.load(open(os.path.join(GOLDEN, "reference_import_lines.json")))


def _signatures():
    return json.load(open(os.path.join(GOLDEN, "surface_signatures.json")))


def test_fixture_covers_the_callers_and_holds_names_only():
    fx = _lines()
    assert set(fx) == {"render_surface.py", "render_nir.py", "render_volume.py", "model_volume.py", "model_bed.py", "utils/process_routine.py"}
    mods = {m for c in fx.values() for m in c}
    assert mods <= set(MIRRORED) | set(CALLERS_OWN), mods - set(MIRRORED) - set(CALLERS_OWN)
    assert {"network_conf", "fields", "helper", "dataset"} <= mods
    for caller, by_mod in fx.items():
        for mod, names in by_mod.items():
            assert names and all(isinstance(n, str) and n.isidentifier() for n in names), (caller, mod)
    assert {"choose_optmizer", "choose_renderer_func"} <= set(fx["render_surface.py"]["network_conf"])
    assert "NeRFdual" in fx["model_volume.py"]["fields"]


def test_every_reference_import_line_resolves_beside_the_callers_own_modules(tmp_path):
    fx = _lines()
    own = {m: sorted({n for c in fx.values() for n in c.get(m, [])}) for m in CALLERS_OWN}
    pkg = tmp_path / "models"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    for mod, names in own.items():
        (pkg / (mod + ".py")).write_text("".join("%s = ('dummy', %r, %r)\n" % (n, mod, n) for n in names))
    import iron_amd
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, str(tmp_path))
    importlib.invalidate_caches()
    try:
        iron_amd.install_as_models()
        import models
        assert os.path.realpath(os.path.dirname(models.__file__)) == os.path.realpath(str(pkg)), "the caller's package was replaced, not overlaid"
        replayed = 0
        for caller, by_mod in fx.items():
            for mod, names in by_mod.items():
                scope = {}
                exec("from models.%s import %s" % (mod, ", ".join(names)), scope)   # the caller's own statement
                m = sys.modules["models." + mod]
                for n in names:
                    replayed += 1
                    if mod in CALLERS_OWN:
                        assert scope[n] == ("dummy", mod, n), (caller, mod, n)
                    else:
                        assert m is importlib.import_module("iron_amd." + mod), (caller, mod)
                        assert scope[n] is getattr(m, n), (caller, mod, n)
        assert replayed >= 100, replayed
        for mod in CALLERS_OWN:
            assert os.path.realpath(os.path.dirname(sys.modules["models." + mod].__file__)) == os.path.realpath(str(pkg)), mod
    finally:
        sys.path.remove(str(tmp_path))
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved)
        importlib.invalidate_caches()


def test_without_a_models_package_one_is_made_up():
    import iron_amd
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    for k in saved:
        del sys.modules[k]
    try:
        if importlib.util.find_spec("models") is not None:
            pytest.fail("a `models` package is importable from the test environment: this test needs none")
        iron_amd.install_as_models()
        from models.network_conf import choose_optmizer, choose_renderer_func  # noqa: F401
        from models.fields import NeRFdual  # noqa: F401
        assert sys.modules["models"].__path__ == []
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# the comparison rule of tests/test_surface_signatures.py, copied: the reference's parameters first, same names, same order, same
# defaults; the mirror may only append defaulted parameters
def _compatible(ref_params, fn):
    """None if compatible, else a description of the first difference."""
    try:
        mine = list(inspect.signature(fn).parameters.values())
    except (TypeError, ValueError) as e:
        return "no signature: %r" % (e,)
    var_kw = any(p.kind is inspect.Parameter.VAR_KEYWORD for p in mine)
    mine_named = [p for p in mine if p.kind not in (inspect.Parameter.VAR_KEYWORD, inspect.Parameter.VAR_POSITIONAL)]
    for i, rp in enumerate(ref_params):
        if rp["kind"] in ("VAR_KEYWORD", "VAR_POSITIONAL"):
            continue
        if i >= len(mine_named):
            return "missing parameter %s" % rp["name"] if not var_kw else None
        mp = mine_named[i]
        if mp.name != rp["name"]:
            return "parameter %d is %s, reference has %s" % (i, mp.name, rp["name"])
        ref_has_default = rp["default"] is not None
        mine_has_default = mp.default is not inspect._empty
        if ref_has_default and not mine_has_default:
            return "parameter %s lost its default %s" % (rp["name"], rp["default"])
        if ref_has_default and repr(mp.default) != rp["default"]:
            return "parameter %s default %r, reference %s" % (rp["name"], mp.default, rp["default"])
    for mp in mine_named[len([p for p in ref_params if p["kind"] not in ("VAR_KEYWORD", "VAR_POSITIONAL")]):]:
        if mp.default is inspect._empty:
            return "extra parameter %s has no default" % mp.name
    return None


def test_the_three_names_have_the_reference_signatures():
    fx = _signatures()
    from iron_amd import fields, network_conf
    for name in ("choose_optmizer", "choose_renderer_func"):
        assert _compatible(fx["models.network_conf"][name]["params"], getattr(network_conf, name)) is None, name
    for method, params in fx["models.fields"]["NeRFdual"]["methods"].items():
        assert _compatible(params, getattr(fields.NeRFdual, method)) is None, method


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2))


GGX_KEYS = ["color_network", "diffuse_albedo_network", "specular_albedo_network", "specular_roughness_network", "point_light_network"]
COMP_KEYS = GGX_KEYS + ["metallic_network", "dielectric_network", "metallic_eta_network", "metallic_k_network", "dielectric_eta_network"]


def _check_optimizers(opts, nets, keys):
    assert list(opts) == keys
    for k in keys:
        assert type(opts[k]) is torch.optim.Adam
        groups = opts[k].param_groups
        assert len(groups) == 1 and groups[0]["lr"] == (1e-2 if k == "point_light_network" else 1e-4), k
        assert len(groups[0]["params"]) == 1 and groups[0]["params"][0] is nets[k].w, k


def test_choose_optmizer_ggx_and_comp():
    from iron_amd.network_conf import choose_optmizer
    nets = {k: _Tiny() for k in COMP_KEYS + ["env_light_network"]}
    _check_optimizers(choose_optmizer("ggx", [], nets), nets, GGX_KEYS)
    # the ggx branch has no name filter (network_conf.py:708-716)
    _check_optimizers(choose_optmizer("ggx", ["color_network"], nets), nets, GGX_KEYS)
    _check_optimizers(choose_optmizer("comp", [], nets), nets, COMP_KEYS)
    _check_optimizers(choose_optmizer("comp2", network_dict=nets), nets, COMP_KEYS)
    pick = ["point_light_network", "metallic_network", "diffuse_albedo_network"]
    _check_optimizers(choose_optmizer("comp", pick, nets), nets, pick)
    with pytest.raises(KeyError):   # every listed network must be there, as in the reference
        choose_optmizer("ggx", [], {k: nets[k] for k in GGX_KEYS[1:]})


def test_nerfdual_has_the_reference_state_dict():
    """models/fields.py:365-384 for NeRFdual(D=8, W=256, multires=10, multires_view=4, use_viewdirs=True): the embedders give
    input_ch = 3 + 3*2*10 = 63 and input_ch_view = 3 + 3*2*4 = 27; pts_linears[0] is 63 -> 256, pts_linears[i + 1] is 256 -> 256
    except after the skip i = 4, where the input is concatenated again (256 + 63 = 319); views_linears[0] is 27 + 256 -> 128;
    with view directions: feature 256 -> 256, alpha 256 -> 1, rgb 128 -> 3, nir 128 -> 1."""
    from iron_amd import _lib
    from iron_amd.fields import NeRFdual
    want = {}
    for i, w_in in enumerate([63, 256, 256, 256, 256, 319, 256, 256]):
        want["pts_linears.%d" % i] = (256, w_in)
    want.update({"views_linears.0": (128, 283), "feature_linear": (256, 256), "alpha_linear": (1, 256), "rgb_linear": (3, 128),
                 "nir_linear": (1, 128)})
    net = NeRFdual(D=8, W=256, multires=10, multires_view=4, use_viewdirs=True)
    sd = net.state_dict()
    expect = {}
    for k, (o, i) in want.items():
        expect[k + ".weight"] = (o, i)
        expect[k + ".bias"] = (o,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == expect
    # a checkpoint of that layout loads (strict), and the flat head of use_viewdirs=False is the reference's output_linear
    other = NeRFdual(D=8, W=256, multires=10, multires_view=4, use_viewdirs=True)
    other.load_state_dict({k: torch.full_like(v, 0.25) for k, v in sd.items()}, strict=True)
    assert float(other.nir_linear.weight.detach().min()) == 0.25
    flat = NeRFdual().state_dict()
    assert tuple(flat["output_linear.weight"].shape) == (5, 256) and tuple(flat["pts_linears.5.weight"].shape) == (256, 259)
    assert "nir_linear.weight" not in flat and tuple(flat["views_linears.0.weight"].shape) == (128, 259)
    # forward: the reference's triple or IronError, nothing else
    try:
        out = net(torch.zeros(2, 3), torch.zeros(2, 3))
    except _lib.IronError:
        pass
    else:
        assert len(out) == 3
