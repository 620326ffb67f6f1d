"""CPU: the fp64 oracle of the fused hash-grid field evaluation (tests/_hashfield_oracle.py) is pinned to a plain-torch fp64
restatement; an fp32 emulation of the kernel's arithmetic yields the GPU tests' tolerance constant; the exclusion caps hold for the
oracle alone; iron_hashgrid_field_check validates shapes on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import _hashfield_oracle as H
import _hashgrid_oracle as O
from iron_amd import _lib, hashgrid

NAMES = [c[0] for c in O.CASES]
_TORCH_ACT = {"ReLU": torch.relu, "Softplus": torch.nn.functional.softplus, "None": lambda z: z}


def _worst(err, tol):
    r = err / np.maximum(tol, 1e-300)
    r[(tol == 0) & (err == 0)] = 0
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_plain_torch_fp64_restatement(name):
    """O.restate in double, the head in double, torch.autograd.grad for the gradient: 1e-12 relative on every case and head.  Points
    within 4 ulp32 of a face or outside the cube are compared too: both sides take the cell of floor(pos) and clamp."""
    c, _ = H.case_encoding(name)
    for (_, head, n_out, act) in [k for k in H.combos() if k[0] == name]:
        W = H.case_weights(name, head, n_out)
        ref = H.reference(name, head, n_out, act)
        x = torch.from_numpy(c["x"].astype(np.float64)).requires_grad_(True)
        h = O.restate(c["cfg"], x, torch.from_numpy(c["table"].astype(np.float64)))
        for l, w in enumerate(W):
            h = h @ torch.from_numpy(w.astype(np.float64)).T
            if l < len(W) - 1:
                h = _TORCH_ACT[act](h)
        (g,) = torch.autograd.grad(h[:, 0].sum(), x)
        out, g = h.detach().numpy(), g.numpy()
        assert np.abs(out - ref["out"]).max() <= 1e-12 * max(np.abs(ref["out"]).max(), 1e-300), (name, head, n_out, act)
        assert np.abs(g - ref["grad"]).max() <= 1e-12 * max(np.abs(ref["grad"]).max(), 1e-300), (name, head, n_out, act)


def _emulation_combos():
    """every (case, head); the activation rotates, ReLU on every head of the check configuration"""
    out = []
    for ci, name in enumerate(NAMES):
        for hi, head in enumerate(H.HEADS):
            acts = {H.ACTS[(ci + hi) % 3]} | ({"ReLU"} if name == "check_mixed" else set())
            out += [k for k in H.combos(acts) if k[0] == name and k[1] == head]
    return out


def test_fp32_emulation_of_the_head_yields_the_tolerance_constant():
    worst_v, worst_g, worst_at = 0.0, 0.0, None
    for (name, head, n_out, act) in _emulation_combos():
        c, _ = H.case_encoding(name)
        ref = H.reference(name, head, n_out, act)
        out, g = H.emulate_head(c["cfg"], c["x"], c["table"], H.case_weights(name, head, n_out), act)
        # what the evaluation of Softplus may err by (F, the library's bounds) is taken off first: the constant scales the chains
        rv = _worst(np.maximum(np.abs(out - ref["out"]) - O.EPS32 * ref["F_out"], 0.0), O.EPS32 * ref["S_out"])
        keep = ~(ref["near"] | ref["kink"])
        rg = _worst(np.maximum(np.abs(g - ref["grad"]) - O.EPS32 * ref["F_grad"], 0.0)[keep], O.EPS32 * ref["S_grad"][keep])
        if max(rv, rg) > max(worst_v, worst_g):
            worst_at = (name, head, n_out, act)
        worst_v, worst_g = max(worst_v, rv), max(worst_g, rg)
    print("   fp32 emulation of the head: worst |err| / (eps32 S): value %.4f, gradient %.4f, at %s" % (worst_v, worst_g, worst_at))
    assert max(worst_v, worst_g) <= H.C_MEASURED_RATIO * 1.001
    assert max(worst_v, worst_g) >= H.C_MEASURED_RATIO * 0.9       # the constant is the measurement, not a round number above it


def test_softplus_constants_cover_the_fp32_expressions():
    z = np.linspace(-30.0, 30.0, 200001).astype(np.float32)
    h = H.act32("Softplus", z)
    exact = H.act("Softplus", z.astype(np.float64))
    assert (np.abs(h - exact) <= H.C_SP * O.EPS32 * np.abs(exact)).all()
    d = H.dact32_from_h("Softplus", h)
    dexact = H.dact("Softplus", z.astype(np.float64))
    assert (np.abs(d - dexact) <= H.C_SPG * O.EPS32 * np.abs(dexact)).all()


@pytest.mark.parametrize("name", NAMES)
def test_exclusion_caps_hold_for_the_oracle(name):
    """ReLU: the points with a hidden pre-activation within its own tolerance of the kink number at most max(2, 1 % of n), for every
    head; the near-face share of the uniform cases stays as DESIGN §27 states (at most 1 % of the (point, level) pairs)."""
    c, enc = H.case_encoding(name)
    n = c["x"].shape[0]
    for (_, head, n_out, act) in [k for k in H.combos({"ReLU"}) if k[0] == name]:
        ref = H.reference(name, head, n_out, act)
        k = int(ref["kink"].sum())
        print("   %s %s: %d of %d points near a kink (%.3f %%)" % (name, head, k, n, 100.0 * k / n))
        assert k <= max(2, n // 100)
    if O.CASES[NAMES.index(name)][3] == "uniform":
        assert enc["near"].mean() <= 0.01


def _desc(cfg, neurons, hidden, n_out, act=1):
    d = _lib.iron_hashgrid_field_desc()
    d.encoding = hashgrid.make_desc(*cfg)
    d.n_neurons, d.n_hidden_layers, d.n_out, d.activation = neurons, hidden, n_out, act
    return d


def test_field_check_accepts_every_case_and_refuses_out_of_range_shapes():
    lib = _lib.load()
    for (name, head, n_out, _) in H.combos({"ReLU"}):
        cfg = O.case_inputs(name)["cfg"]
        n = C.c_int64(-1)
        assert lib.iron_hashgrid_field_check(C.byref(_desc(cfg, head[0], head[1], n_out)), C.byref(n)) == _lib.IRON_OK
        assert n.value == sum(w.size for w in H.case_weights(name, head, n_out))
        assert lib.iron_hashgrid_field_pack_bytes(C.byref(_desc(cfg, head[0], head[1], n_out))) % 16 == 0
    cfg = O.CHECK_CFG
    for bad in (_desc(cfg, 48, 2, 1), _desc(cfg, 64, 0, 1), _desc(cfg, 64, 5, 1), _desc(cfg, 64, 2, 17), _desc((32, 8, 14, 16, 1.1), 64, 2, 1)):
        assert lib.iron_hashgrid_field_check(C.byref(bad), None) == _lib.IRON_ERR_RANGE
        assert lib.iron_hashgrid_field_pack_bytes(C.byref(bad)) == 0
    assert lib.iron_hashgrid_field_check(C.byref(_desc(cfg, 64, 2, 1, act=7)), None) == _lib.IRON_ERR_BAD_ARG


def test_field_refuses_unsupported_heads_by_name(tmp_path):
    import json
    from iron_amd import tcnn_fields
    conf = {"encoding": {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 4,
                         "per_level_scale": 1.5},
            "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 48, "n_hidden_layers": 2}}
    p = tmp_path / "f.json"
    p.write_text(json.dumps(conf))
    f = tcnn_fields.TCNNSDF(str(p))
    keys = set(f.state_dict().keys())
    assert not f.fused_supported()
    with pytest.raises(_lib.IronError, match="CUDA"):
        f.eval_fused(torch.zeros(4, 3))
    with pytest.raises(_lib.IronError, match="n_neurons"):
        f.as_callable(0.5, 0.5)
    conf["network"]["n_neurons"] = 64
    p.write_text(json.dumps(conf))
    g = tcnn_fields.TCNNSDF(str(p))
    assert g.fused_supported() and set(g.state_dict().keys()) == keys
