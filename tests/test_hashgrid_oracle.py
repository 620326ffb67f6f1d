"""CPU: the hash-grid encoding's definition.  The host layout function reproduces the check values and refuses what is not built;
the fp64 oracle (tests/_hashgrid_oracle.py) agrees with finite differences, with torch autograd of the plain-torch restatement, and
reproduces affine fields; the fp32 emulation of the kernel's fused fraction yields the tolerance constant of the GPU tests."""
import json

import numpy as np
import pytest
import torch

import _hashgrid_oracle as O
from iron_amd import _lib, hashgrid, tcnn_fields

CHECK_RES = [16, 23, 31, 43, 59, 81, 112, 154, 213, 295, 407, 562, 776, 1073, 1482, 2048]
CHECK_SIZE = [4096, 12168, 29792, 79512, 205384] + [524288] * 11
SMALL = (4, 2, 12, 4, 1.5)


def _desc(cfg):
    L, F, log2T, N, b = cfg
    return hashgrid.make_desc(L, F, log2T, N, b)


def test_layout_reproduces_the_check_values():
    levels, n_params = hashgrid.layout(_desc(O.CHECK_CFG))
    assert [lv["res"] for lv in levels] == CHECK_RES
    assert [lv["size"] for lv in levels] == CHECK_SIZE
    assert n_params == 6098120
    assert [lv["dense"] for lv in levels] == [True] * 5 + [False] * 11
    assert [lv["offset"] for lv in levels] == list(np.cumsum([0] + CHECK_SIZE[:-1]))


@pytest.mark.parametrize("cfg", sorted({c[1] for c in O.CASES}) + [SMALL, (32, 1, 24, 1, 1.0), (3, 2, 24, 256, 1.0)])
def test_layout_matches_the_oracle(cfg):
    levels, n_params = hashgrid.layout(_desc(cfg))
    want, want_n = O.levels_of(cfg)
    assert n_params == want_n
    for a, b in zip(levels, want):
        assert a == b


@pytest.mark.parametrize("key,value", [("n_levels", 0), ("n_levels", 33), ("n_features_per_level", 3), ("n_features_per_level", 16),
                                       ("log2_hashmap_size", 25), ("log2_hashmap_size", 0), ("base_resolution", 0),
                                       ("per_level_scale", 0.5), ("per_level_scale", float("nan")), ("n_levels", 2.5)])
def test_descriptor_refuses_out_of_range_values(key, value):
    kw = dict(n_levels=4, n_features_per_level=2, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.5)
    kw[key] = value
    with pytest.raises(_lib.IronError, match=key):
        hashgrid.HashEncoding(**kw)


def test_layout_function_validates_on_its_own():
    lib = _lib.load()
    d = _desc(SMALL)
    d.n_features_per_level = 3
    assert lib.iron_hashgrid_layout(d, None, None) == _lib.IRON_ERR_BAD_ARG
    d = _desc(SMALL)
    d.per_level_scale = 4.0
    d.n_levels = 32                                    # 4^31 * 4: far past what fp32 cell arithmetic resolves
    assert lib.iron_hashgrid_layout(d, None, None) == _lib.IRON_ERR_RANGE
    with pytest.raises(_lib.IronError, match="per_level_scale"):
        hashgrid.layout(d)
    assert lib.iron_hashgrid_encode(_desc(SMALL), None, 4, None, None, None, None) == _lib.IRON_ERR_BAD_ARG   # before any device work
    t = _lib.load_train()
    assert t.iron_hashgrid_backward(_desc(SMALL), None, 4, None, None, None, None, None, 0, None) == _lib.IRON_ERR_BAD_ARG
    assert t.iron_hashgrid_backward_workspace_bytes(_desc(SMALL), 16) >= 8 * 2 * hashgrid.layout(_desc(SMALL))[1]
    assert t.iron_hashgrid_backward_backward_workspace_bytes(d, 16) == 0


@pytest.mark.parametrize("key,value", [("interpolation", "Smoothstep"), ("otype", "DenseGrid"), ("type", "Tiled"), ("table_dtype", "float16"),
                                       ("n_dims_to_encode", 2), ("stochastic_interpolation", True)])
def test_config_refuses_each_unsupported_key(key, value):
    cfg = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4,
           "per_level_scale": 1.5}
    assert hashgrid.parse_encoding_config(dict(cfg, interpolation="Linear", type="Hash")) == {k: cfg[k] for k in hashgrid.ENCODING_KEYS}
    cfg[key] = value
    with pytest.raises(_lib.IronError, match=key):
        hashgrid.parse_encoding_config(cfg)
    del cfg[key]
    del cfg["n_levels"]
    if key != "otype":
        with pytest.raises(_lib.IronError, match="n_levels"):
            hashgrid.parse_encoding_config(cfg)


def _small_inputs(cfg, n, seed, away=None):
    rng = np.random.default_rng(seed)
    levels, P = O.levels_of(cfg)
    x = rng.random((n, 3))
    if away is not None:      # keep every pos at least `away` from a face, on every level
        ok = np.ones(n, bool)
        for lv in levels:
            pos = x * lv["scale"] + 0.5
            ok &= (np.abs(pos - np.rint(pos)) > away).all(axis=1)
        x = x[ok]
    table = rng.random((P, cfg[1])) * 0.2 - 0.1
    return x, table, rng


def test_oracle_jacobian_is_the_central_difference_of_its_features():
    x, table, _ = _small_inputs(SMALL, 300, 1, away=1e-3)
    assert x.shape[0] > 200
    e = O.encode(SMALL, x, table)
    h = 1e-6     # h * scale < 1e-3: both sides stay in the cell; the features are trilinear there, so the difference is exact up to rounding
    for d in range(3):
        dx = np.zeros(3)
        dx[d] = h
        fd = (O.encode(SMALL, x + dx, table)["y"] - O.encode(SMALL, x - dx, table)["y"]) / (2 * h)
        assert np.abs(fd - e["J"][:, :, d]).max() <= 1e-9 * max(1.0, np.abs(e["J"]).max())
    # clamped axes: zero columns, and the features of the clamped point
    xo = x.copy()
    xo[:, 0], xo[:, 2] = -0.25, 1.5
    eo = O.encode(SMALL, xo, table)
    assert not eo["J"][:, :, 0].any() and not eo["J"][:, :, 2].any() and eo["J"][:, :, 1].any()
    assert np.array_equal(eo["y"], O.encode(SMALL, np.clip(xo, 0, 1), table)["y"])


@pytest.mark.parametrize("cfg", [SMALL, (2, 4, 4, 16, 2.0), (1, 1, 14, 16, 1.0)])
def test_oracle_gradients_equal_autograd_of_the_restatement(cfg):
    x, table, rng = _small_inputs(cfg, 200, 2, away=1e-6)
    n, width = x.shape[0], cfg[0] * cfg[1]
    dy, g = rng.random((n, width)) * 2 - 1, rng.random((n, 3)) * 2 - 1
    xt = torch.tensor(x, requires_grad=True)
    tt = torch.tensor(table, requires_grad=True)
    dyt = torch.tensor(dy, requires_grad=True)
    y = O.restate(cfg, xt, tt)
    e = O.encode(cfg, x, table)
    assert np.abs(y.detach().numpy() - e["y"]).max() <= 1e-15
    d_x, d_table = torch.autograd.grad(y, (xt, tt), dyt, create_graph=True)
    b = O.backward(cfg, x, table, dy)
    assert np.abs(d_x.detach().numpy() - b["d_x"]).max() <= 1e-12 * np.abs(b["d_x"]).max()
    assert np.abs(d_table.detach().numpy() - b["d_table"]).max() <= 1e-13 * np.abs(b["d_table"]).max()
    assert b["count"].sum() == 8 * n * cfg[0]
    d_dy, d_table2 = torch.autograd.grad(d_x, (dyt, tt), torch.tensor(g))
    bb = O.backward_backward(cfg, x, table, dy, g)
    assert np.abs(d_dy.numpy() - bb["d_dy"]).max() <= 1e-12 * np.abs(bb["d_dy"]).max()
    assert np.abs(d_table2.numpy() - bb["d_table"]).max() <= 1e-12 * np.abs(bb["d_table"]).max()
    assert (np.abs(bb["d_table"]) <= bb["mag"] * (1 + 1e-12)).all() and (np.abs(b["d_table"]) <= b["mag"] * (1 + 1e-12)).all()


def test_affine_fields_are_reproduced_on_a_dense_level():
    cfg = (1, 4, 19, 16, 1.0)                        # one dense level: scale 15, res 16
    (lv,), P = O.levels_of(cfg)
    assert lv["dense"] and lv["scale"] == 15.0
    A = np.array([[0.3, -1.1, 0.7], [2.0, 0.0, -0.5], [0.0, 0.0, 0.0], [-0.25, 0.5, 1.5]])
    c0 = np.array([0.1, -0.2, 0.3, 0.0])
    table = np.zeros((P, 4))
    r = lv["res"]
    k = np.arange(r ** 3)
    nodes = np.stack([k % r, (k // r) % r, k // (r * r)], axis=1)      # node (c0, c1, c2) sits at pos = c: x = (c - 0.5) / scale
    table[:r ** 3] = ((nodes - 0.5) / lv["scale"]) @ A.T + c0
    x = np.random.default_rng(3).random((500, 3)) * (1.0 - 1.0 / lv["scale"])      # away from the wrapped top face
    e = O.encode(cfg, x, table)
    assert np.abs(e["y"] - (x @ A.T + c0)).max() <= 1e-13
    assert np.abs(e["J"] - A[None]).max() <= 1e-11
    y32, J32 = O.emulate_fp32(cfg, x.astype(np.float32), table.astype(np.float32))
    assert np.abs(y32 - (x.astype(np.float32).astype(np.float64) @ A.T + c0)).max() <= 1e-5
    # the wrapped face: x = 1 reads coordinate res, which the dense index folds onto another row -- as tiny-cuda-nn does
    idx, _, _, _ = O.corner_walk(lv, np.array([[1.0, 0.2, 0.2]]))
    assert idx[0, 1] == (16 + 3 * 16 + 3 * 256) % lv["size"] == idx[0, 0] + 1


def test_fixed_point_unit_leaves_room_for_every_contribution():
    for bound in (1e-30, 3e-5, 0.1, 1.0, 1.5, 7e4, 3e30):
        for n in (1, 2, 63, 4099, 1 << 20, (1 << 31) - 1):
            unit = hashgrid.grad_unit(bound, n)
            f32 = float(np.float32(bound))
            assert unit == 2.0 ** round(np.log2(unit))
            assert 8 * n * (f32 / unit + 0.5) < 2.0 ** 63
            assert 8 * n * (f32 / unit) >= 2.0 ** 59          # and wastes at most three bits
    assert hashgrid.grad_unit(0.0, 100) == 1.0


def test_json_reader_and_field_construction(tmp_path):
    conf = {"encoding": {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4,
                         "per_level_scale": 1.5, "interpolation": "Linear"},
            "network": {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 2}}
    p = tmp_path / "sdf.json"
    p.write_text(json.dumps(conf))
    got = tcnn_fields.read_config(str(p))
    assert got["encoding"] == {k: conf["encoding"][k] for k in hashgrid.ENCODING_KEYS}
    assert got["network"] == {"activation": "Softplus", "n_neurons": 32, "n_hidden_layers": 2}
    torch.manual_seed(0)
    f = tcnn_fields.TCNNSDF(str(p), n_outputs_dims=5)
    enc = f.sdf_encoding
    assert enc.n_output_dims == 8 and enc.params.dtype == torch.float32 and enc.params.numel() == 2 * O.levels_of(SMALL)[1]
    top = float(enc.params.detach().abs().max())
    assert 0.9e-4 < top <= 1e-4 and float(enc.params.detach().min()) < 0
    lin = [m for m in f.sdf_network if isinstance(m, torch.nn.Linear)]
    assert [tuple(m.weight.shape) for m in lin] == [(32, 8), (32, 32), (5, 32)] and all(m.bias is None for m in lin)
    assert sum(isinstance(m, torch.nn.Softplus) for m in f.sdf_network) == 2
    torch.manual_seed(0)
    again = tcnn_fields.TCNNSDF(str(p), n_outputs_dims=5)
    assert torch.equal(again.sdf_encoding.params, enc.params)          # torch's generator
    with pytest.raises(_lib.IronError):                                  # no CPU path
        f(torch.zeros(4, 3))
    for block, key, value in [("network", "activation", "Sine"), ("network", "output_activation", "ReLU"), ("network", "n_neurons", 0),
                              ("network", "otype", "MegaMLP"), ("network", "feedback", 1), ("encoding", "interpolation", "Smoothstep")]:
        bad = json.loads(json.dumps(conf))
        bad[block][key] = value
        p.write_text(json.dumps(bad))
        with pytest.raises(_lib.IronError, match=key):
            tcnn_fields.TCNNSDF(str(p))
    p.write_text(json.dumps({"encoding": conf["encoding"]}))
    with pytest.raises(_lib.IronError, match="network"):
        tcnn_fields.read_config(str(p))


def test_install_as_models_registers_the_field_module():
    import sys
    import iron_amd
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    try:
        iron_amd.install_as_models()
        from models.tcnn_fields import TCNNSDF
        assert TCNNSDF is tcnn_fields.TCNNSDF
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_fp32_emulation_of_the_fused_fraction_yields_the_tolerance_constant():
    """The kernel's arithmetic, emulated in numpy fp32 on the GPU tests' own inputs, against the oracle: the largest
    |error| / (eps32 S) is what K doubles.  Also the finding behind the fused form: the fraction taken as pos - floor(pos) from the
    rounded fp32 pos is three orders of magnitude worse on the check configuration."""
    worst_y = worst_j = 0.0
    for name, cfg, n, kind in O.CASES:
        c = O.case_inputs(name)
        e = O.encode(cfg, c["x"], c["table"])
        y, J = O.emulate_fp32(cfg, c["x"], c["table"])
        ry = np.abs(y - e["y"]) / (O.EPS32 * np.maximum(e["Sy"], 1e-300))
        keep = np.broadcast_to(~np.repeat(e["near"], cfg[1], axis=1)[:, :, None], J.shape)
        rj = (np.abs(J - e["J"]) / (O.EPS32 * np.maximum(e["SJ"], 1e-300)))[keep]
        assert np.isfinite(ry).all() and np.isfinite(rj).all()
        worst_y, worst_j = max(worst_y, float(ry.max())), max(worst_j, float(rj.max()) if rj.size else 0.0)
        if kind == "uniform":
            assert e["near"].mean() <= 0.01, (name, e["near"].mean())     # measured: 0.05 % overall, 0.22 % at the finest level
        if name == "check_uniform":
            print("fused:   max |dy| %.2e  max |dJ| %.2e" % (np.abs(y - e["y"]).max(), np.abs(J - e["J"]).max()))
            assert np.abs(y - e["y"]).max() <= 5e-8 and np.abs(J - e["J"]).max() <= 2e-4        # measured 2.0e-8, 8.0e-5
            yu, Ju = O.emulate_fp32(cfg, c["x"], c["table"], fused=False)
            print("unfused: max |dy| %.2e  max |dJ| %.2e" % (np.abs(yu - e["y"]).max(), np.abs(Ju - e["J"]).max()))
            assert np.abs(yu - e["y"]).max() >= 5e-6                                                # measured 1.3e-5
    print("largest ratio: features %.3f, Jacobian %.3f" % (worst_y, worst_j))
    assert max(worst_y, worst_j) <= O.K_MEASURED_RATIO * 1.001
    assert max(worst_y, worst_j) >= O.K_MEASURED_RATIO * 0.9       # the constant is the measurement, not a round number above it
