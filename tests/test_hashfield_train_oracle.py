"""CPU: the fp64 oracle of the fused training backward (tests/_hashfield_train_oracle.py) is pinned to fp64 torch.autograd on the
plain-torch restatement (create_graph=True, then backward()); an fp32 emulation in the defined orders, slot cut and fp64 slot sum
included, yields the GPU tests' tolerance constant; the zeroed rows stay under §28's cap; the host-only entry points of the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

import _hashfield_oracle as H
import _hashfield_train_oracle as T
import _hashgrid_oracle as O
from iron_amd import _lib, hashgrid

NAMES = [c[0] for c in O.CASES]
_TORCH_ACT = {"ReLU": torch.relu, "Softplus": torch.nn.functional.softplus, "None": lambda z: z}


def _worst(err, tol):
    r = err / np.maximum(tol, 1e-300)
    r[(tol == 0) & (err == 0)] = 0
    return float(r.max()) if r.size else 0.0


def _autograd(cfg, x, table, W, act, d_out, d_g, a3):
    """loss = sum d_out out + sum d_g (a dout_0 / dx) on O.restate plus an fp64 head -> ybar, e, the weight gradients, d_table"""
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    tt = torch.from_numpy(np.asarray(table, np.float64)).requires_grad_(True)
    Wt = [torch.from_numpy(np.asarray(w, np.float64)).requires_grad_(True) for w in W]
    y = O.restate(cfg, xt, tt)
    h = y
    for l, w in enumerate(Wt):
        h = h @ w.T
        if l < len(Wt) - 1:
            h = _TORCH_ACT[act](h)
    (g,) = torch.autograd.grad(h[:, 0].sum(), xt, create_graph=True)
    (e,) = torch.autograd.grad(h[:, 0].sum(), y, retain_graph=True)
    loss = (h * torch.from_numpy(d_out.astype(np.float64))).sum() + (g * torch.from_numpy(d_g.astype(np.float64) * np.asarray(a3)[None])).sum()
    (ybar,) = torch.autograd.grad(loss, y, retain_graph=True)
    loss.backward()
    return ybar.numpy(), e.numpy(), [w.grad.numpy() for w in Wt], tt.grad.numpy()


def _pin(name, head, n_out, act, ref, tab, want):
    def close(a, b, what):
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (name, head, n_out, act, what)
    ybar, e, Wg, d_table = want
    close(ref["ybar"][0], ybar, "ybar")
    close(ref["e"][0], e, "e")
    for l, w in enumerate(Wg):
        close(ref["Wbar"][l][0], w, "Wbar_%d" % l)
    close(tab["d_table"], d_table, "d_table")


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_fp64_autograd_on_the_restatement(name):
    c, _ = H.case_encoding(name)
    for (_, head, n_out, act) in [k for k in T.combos() if k[0] == name]:
        d_out, d_g, _, _ = T.case_adjoints(name, head, n_out, act)
        ref = T.reference(name, head, n_out, act)
        tab = T.table_reference(c["cfg"], c["x"], c["table"], ref)
        _pin(name, head, n_out, act, ref, tab,
             _autograd(c["cfg"], c["x"], c["table"], H.case_weights(name, head, n_out), act, d_out, d_g, (1.0, 1.0, 1.0)))


def test_oracle_with_an_affine_map_equals_autograd():
    name, head, n_out, act = "check_mixed", (32, 2), 3, "Softplus"
    c, _ = H.case_encoding(name)
    a3 = (0.5, 0.5, 0.5)
    x = (c["x"].astype(np.float64) * 0.5 + 0.5).astype(np.float32)
    d_out, d_g, _, _ = T.case_adjoints(name, head, n_out, act)
    W = H.case_weights(name, head, n_out)
    ref = T.backward(c["cfg"], x, c["table"], W, act, d_out, d_g, a3)
    _pin(name, head, n_out, act, ref, T.table_reference(c["cfg"], x, c["table"], ref), _autograd(c["cfg"], x, c["table"], W, act, d_out, d_g, a3))


def _emulation_combos():
    """every combination the pin test uses: case x head x activation"""
    return T.combos()


def test_fp32_emulation_in_the_defined_orders_yields_the_tolerance_constant():
    worst = {"ybar": 0.0, "e": 0.0, "Wbar": 0.0}
    at = {}
    for (name, head, n_out, act) in _emulation_combos():
        c, _ = H.case_encoding(name)
        d_out, d_g, _, _ = T.case_adjoints(name, head, n_out, act)
        ref = T.reference(name, head, n_out, act)
        ybar, e, Wbar = T.emulate(c["cfg"], c["x"], c["table"], H.case_weights(name, head, n_out), act, d_out, d_g)
        keep = ~H.reference(name, head, n_out, act)["kink"]          # e does not see the adjoints: kink rows are left out of it

        def ratio(got, q, rows=slice(None)):
            return _worst(np.maximum(np.abs(got - q[0]) - O.EPS32 * q[2], 0.0)[rows], (O.EPS32 * q[1])[rows])

        r = {"ybar": ratio(ybar, ref["ybar"]), "e": ratio(e, ref["e"], keep),
             "Wbar": max(ratio(Wbar[l], ref["Wbar"][l]) for l in range(len(Wbar)))}
        for k in r:
            if r[k] > worst[k]:
                worst[k], at[k] = r[k], (name, head, n_out, act)
    for k in worst:                                     # each quantity has its own constant: twice its own largest ratio
        print("   fp32 emulation of the training backward: %s worst |err| / (eps32 S) = %.4f at %s" % (k, worst[k], at[k]))
        assert worst[k] <= T.C_TRAIN_MEASURED_RATIO[k] * 1.001
        assert worst[k] >= T.C_TRAIN_MEASURED_RATIO[k] * 0.9           # the constant is the measurement, not a round number above it


@pytest.mark.parametrize("name", NAMES)
def test_zeroed_rows_stay_under_the_cap(name):
    n = O.case_inputs(name)["x"].shape[0]
    for (_, head, n_out, act) in [k for k in T.combos() if k[0] == name]:
        d_out, d_g, kinks, _ = T.case_adjoints(name, head, n_out, act)
        assert kinks <= max(2, n // 100), (name, head, act, kinks)
        assert int((~d_out.any(axis=1)).sum()) == kinks


def _desc(cfg, neurons, hidden, n_out, act=1):
    d = _lib.iron_hashgrid_field_desc()
    d.encoding = hashgrid.make_desc(*cfg)
    d.n_neurons, d.n_hidden_layers, d.n_out, d.activation = neurons, hidden, n_out, act
    return d


def test_host_only_entry_points():
    lib = _lib.load_train()
    for n in (0, 1, 63, 64, 65, 4099, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 26):
        assert lib.iron_hashgrid_field_train_slot(n) == T.slot_points(n), n
        assert T.slot_points(n) % 64 == 0 and -(-n // T.slot_points(n)) <= 1024
    for (name, head, n_out, act) in T.combos():
        d = _desc(O.case_inputs(name)["cfg"], head[0], head[1], n_out, _lib.IRON_FIELD_ACT[act])
        assert lib.iron_hashgrid_field_train_check(C.byref(d)) == _lib.IRON_OK
        assert lib.iron_hashgrid_field_train_pack_bytes(C.byref(d)) % 16 == 0 and lib.iron_hashgrid_field_train_pack_bytes(C.byref(d)) > 0
        assert lib.iron_hashgrid_field_backward_workspace_bytes(C.byref(d), 4099) > 0
    cfg = O.CHECK_CFG
    wide = (16, 8, 14, 16, 1.3)                                        # L F = 128
    for bad in (_desc(cfg, 128, 2, 1), _desc(cfg, 48, 2, 1), _desc(cfg, 64, 5, 1), _desc(wide, 64, 4, 1, act=2)):
        assert lib.iron_hashgrid_field_train_check(C.byref(bad)) == _lib.IRON_ERR_RANGE
        assert lib.iron_hashgrid_field_train_pack_bytes(C.byref(bad)) == 0
        assert lib.iron_hashgrid_field_backward_workspace_bytes(C.byref(bad), 64) == 0
    assert lib.iron_hashgrid_field_train_check(C.byref(_desc(wide, 64, 4, 1, act=1))) == _lib.IRON_OK      # ReLU: three rows per neuron
    assert lib.iron_hashgrid_field_train_check(C.byref(_desc(cfg, 64, 4, 1, act=2))) == _lib.IRON_OK
