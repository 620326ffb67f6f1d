"""iron_amd.conf: the two committed settings files (verbatim copies of the reference's confs/womask_iron.conf and
confs/blender01_iron.conf) parse to the types and values pyhocon gives render_volume.py, and a hand-written text covers the
corners of the grammar."""
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name, case="CASE"):
    from iron_amd.conf import parse_file
    return parse_file(os.path.join(GOLDEN, name), case=case)


def test_womask_iron_conf():
    conf = _load("womask_iron.conf", case="dragon")
    assert conf["train.learning_rate"] == 5e-4 and type(conf["train.learning_rate"]) is float
    assert conf.get_float("train.learning_rate") == 5e-4
    assert conf["model.nerf.skips"] == [4] and type(conf["model.nerf.skips"][0]) is int
    assert conf["train.use_white_bkgd"] is False and conf.get_bool("train.use_white_bkgd") is False
    assert conf["model.neus_renderer.up_sample_steps"] == 4 and type(conf["model.neus_renderer.up_sample_steps"]) is int
    assert conf["general.recording"] == ["./", "./models"]
    assert conf["general.base_exp_dir"] == "./exp_stage1/dragon/"
    assert conf.get_string("dataset.render_cameras_name") == "cameras_sphere.npz"
    assert conf.get_int("train.end_iter") == 100001 and conf.get_int("train.batch_size") == 512
    assert conf.get_float("train.warm_up_end", default=0.0) == 5000.0 and type(conf.get_float("train.warm_up_end")) is float
    assert conf.get_float("train.mask_weight") == 0.0 and conf.get_float("train.igr_weight") == 0.1
    assert "folder_name" not in conf["dataset"] and "dataset.folder_name" not in conf and "train.anneal_end" in conf
    assert dict(**conf["model.nerf"]) == {"D": 8, "d_in": 4, "d_in_view": 3, "W": 256, "multires": 10, "multires_view": 4, "output_ch": 4,
                                          "skips": [4], "use_viewdirs": True}
    assert conf["model.nerf"]["use_viewdirs"] is True
    assert dict(**conf["model.sdf_network"]) == {"d_out": 257, "d_in": 3, "d_hidden": 256, "n_layers": 8, "skip_in": [4], "multires": 6,
                                                 "bias": 0.5, "scale": 1.0, "geometric_init": True, "weight_norm": True}
    assert type(conf["model.sdf_network.scale"]) is float
    assert dict(**conf["model.variance_network"]) == {"init_val": 0.3}
    assert conf["model.rendering_network.mode"] == "idr" and conf["model.rendering_network"]["squeeze_out"] is True
    assert dict(**conf["model.neus_renderer"]) == {"n_samples": 64, "n_importance": 64, "n_outside": 32, "up_sample_steps": 4, "perturb": 1.0}
    # the reference writes into the parsed tree (render_volume.py:35)
    conf["dataset.data_dir"] = conf["dataset.data_dir"].replace("dragon", "buddha")
    assert conf["dataset"]["data_dir"] == "./data_nir/buddha/train/"


def test_blender01_iron_conf():
    conf = _load("blender01_iron.conf", case="duck")
    assert conf["dataset.folder_name"] == "blender_0.1" and type(conf["dataset.folder_name"]) is str
    assert "folder_name" in conf["dataset"]
    assert conf["dataset.data_dir"] == "./data_envlight/duck/train/"
    assert conf.get_int("train.val_freq") == 2500
    assert conf["train.learning_rate"] == 5e-4 and conf["model.nerf.skips"] == [4] and conf["train.use_white_bkgd"] is False
    assert conf["model.neus_renderer.up_sample_steps"] == 4 and conf["general.recording"] == ["./", "./models"]


CORNERS = """
# a comment line
outer {
    inner {
        D = 8,
        name = "a quoted, string # kept"   # a comment behind it
        flag = true
        other = false,
    }
    rate = 5e-4
    list = [1,
            2.5,   # inside a list
            three]
    neg=-3
}
plain = ./some/path_0.1/
"""


def test_grammar_corners():
    from iron_amd.conf import ConfError, parse_string
    conf = parse_string(CORNERS)
    assert conf["outer.inner.D"] == 8 and type(conf["outer.inner.D"]) is int          # the trailing comma
    assert conf["outer.inner.name"] == "a quoted, string # kept"
    assert conf["outer.inner.flag"] is True and conf["outer.inner.other"] is False
    assert conf["outer.list"] == [1, 2.5, "three"] and conf["outer.neg"] == -3 and conf["plain"] == "./some/path_0.1/"
    assert conf.get_int("outer.inner.missing", default=7) == 7                        # a nested lookup with a default
    assert conf.get_float("outer.nothing.here", default=0.0) == 0.0
    assert conf.get_string("nowhere", default="x") == "x" and conf.get_bool("outer.inner.none", default=True) is True
    assert conf["outer"].get_float("rate") == 5e-4
    with pytest.raises(ConfError):
        conf.get_int("outer.inner.missing")
    with pytest.raises(ConfError):
        conf.get_int("outer.rate")
    with pytest.raises(ConfError):
        conf.get_bool("outer.neg")
    with pytest.raises(KeyError):
        conf["outer.inner.missing"]


@pytest.mark.parametrize("text, line, word", [
    ("a = 1\nb {\n  c = 2\n\nd = 3\n", 2, "never closed"),           # the unclosed brace is named by its line
    ("a = 1\nb = ${a}\n", 2, "substitution"),
    ("a = 1\n\ninclude \"other.conf\"\n", 3, "include"),
    ("a = [1]\na += [2]\n", 2, "+="),
    ("a = [1,\n 2\n", 1, "never closed"),
    ("a = 1\n}\n", 2, "closing brace"),
    ("a.b = 1\n", 1, "dotted"),
    ("a = \"open\n", 1, "quoted"),
    ("a =\n", 1, "missing"),
])
def test_what_lies_outside_the_grammar_is_an_error_with_its_line(text, line, word):
    from iron_amd.conf import ConfError, parse_string
    with pytest.raises(ConfError) as e:
        parse_string(text)
    assert ("line %d:" % line) in str(e.value) and word in str(e.value), str(e.value)
