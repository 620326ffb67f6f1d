"""GPU: iron_hashgrid_backward_pair (csrc/hashgrid_train.hip) -- the table gradient of both orders in one pass --
against the fp64 oracle sum O.backward(dy1) + O.backward_backward(dy2, g) and against the two existing entry points, on every case
of O.CASES (n in {1, 63, 64, 65, 257, 4099}; F in {1, 2, 4, 8}; dense and hashed levels; nodes, faces and clamped points).

Tolerances, per entry, none of them measured on the kernel:
    oracle      count unit_l + K eps32 (mag1 + mag2): §27's form.  One contribution per (point, corner) is rounded to the level's unit
                2^e, e = grad_unit_exp(fl32(max |dy1| + bound2_l), n) with bound2_l the second-order bound as the oracle forms it;
                K eps32 times the sum of the term magnitudes covers the fp32 weights and the one conversion to fp32.
    two calls   the three kernels share wgt_o and c_o bit for bit, so the exact contributions agree and only the roundings differ:
                half a unit per contribution on either side, count (unit_pair + unit_1 + unit_2,l) / 2, plus the conversion of each
                of the three results to fp32, (eps32 / 2) (|d1| + |d2| + |pair|).
With dy2 = 0 and g = 0 (or dy1 = 0) the bound, the unit and every rounded contribution are those of the one-order call: bitwise equal."""
import functools

import numpy as np
import pytest
import torch

import _hashgrid_oracle as O
from iron_amd import hashgrid

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in O.CASES]
KE = O.K * O.EPS32


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs (dy2: the rows of dy in reverse order, scaled), the oracle's two table gradients (computed once, left alone), devices"""
    c = dict(O.case_inputs(name))
    c["dy2"] = (np.float32(0.37) * c["dy"][::-1]).astype(np.float32).copy()
    cfg = c["cfg"]
    ref = dict(first=O.backward(cfg, c["x"], c["table"], c["dy"]), second=O.backward_backward(cfg, c["x"], c["table"], c["dy2"], c["g"]))
    dev = {k: torch.from_numpy(c[k]).cuda() for k in ("x", "table", "dy", "dy2", "g")}
    L, F, log2T, N, b = cfg
    return c, ref, dev, hashgrid.HashEncoding(L, F, log2T, N, b)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _worst(err, tol):
    r = err / np.maximum(tol, 1e-300)
    r[(tol == 0) & (err == 0)] = 0
    return float(r.max()) if r.size else 0.0


def _pair(e, dev, **kw):
    return hashgrid.backward_pair(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], dev["dy2"], dev["g"], **kw)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("name", NAMES)
def test_pair_matches_the_oracle_sum_and_the_two_calls(name):
    c, ref, dev, e = _case(name)
    cfg, n = c["cfg"], c["x"].shape[0]
    got = _np(_pair(e, dev))
    r1, r2 = ref["first"], ref["second"]
    assert (r1["count"] == r2["count"]).all()
    lvl = O.level_of_entry(cfg)
    m1 = np.float32(np.abs(c["dy"]).max())
    unit = np.array([hashgrid.grad_unit(float(m1 + np.float32(b2)), n) for b2 in r2["bound"]])[lvl][:, None]
    count = r1["count"][:, None]
    tol = count * unit + KE * (r1["mag"] + r2["mag"])
    err = np.abs(got - (r1["d_table"] + r2["d_table"]))
    print("   %s: pair d_table worst ratio to the oracle %.3f (up to %d contributions per entry)" % (name, _worst(err, tol), int(count.max())))
    assert (err <= tol).all()
    assert not got[r1["count"] == 0].any()
    d1 = _np(hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], want_x=False)[0])
    d2 = _np(hashgrid.backward_backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy2"], dev["g"], want_dy=False)[1])
    u1 = hashgrid.grad_unit(float(m1), n)
    u2 = np.array([hashgrid.grad_unit(b2, n) for b2 in r2["bound"]])[lvl][:, None]
    tol2 = 0.5 * count * (unit + u1 + u2) + 0.5 * O.EPS32 * (np.abs(d1) + np.abs(d2) + np.abs(got))
    err2 = np.abs(got - (d1 + d2))
    print("   %s: pair against the two calls, worst ratio %.3f" % (name, _worst(err2, tol2)))
    assert (err2 <= tol2).all()


@pytest.mark.parametrize("name", ["check_uniform", "hashed_tiny_table", "hashed_f8_nodes", "steep_f4"])
def test_pair_is_bitwise_reproducible_order_free_and_written_whole(name):
    c, _, dev, e = _case(name)
    n = c["x"].shape[0]
    first = _pair(e, dev)
    assert not torch.isnan(first).any()
    nan = torch.full((e.n_params, c["cfg"][1]), float("nan"), device="cuda")
    for _ in range(2):
        assert torch.equal(_bits(_pair(e, dev, d_table_out=nan.clone())), _bits(first))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).cuda()
    moved = {k: (dev[k][perm].contiguous() if k != "table" else dev[k]) for k in dev}
    assert torch.equal(_bits(_pair(e, moved)), _bits(first))


@pytest.mark.parametrize("name", ["check_mixed", "hashed_tiny_table", "one_level_f4", "equal_levels_f8"])
def test_one_order_alone_has_the_bits_of_its_own_entry_point(name):
    c, _, dev, e = _case(name)
    zero_dy, zero_g = torch.zeros_like(dev["dy"]), torch.zeros_like(dev["g"])
    only_first = hashgrid.backward_pair(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], zero_dy, zero_g)
    want = hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], want_x=False)[0]
    assert torch.equal(_bits(only_first), _bits(want))
    only_second = hashgrid.backward_pair(e.desc, e.n_params, dev["x"], dev["table"], zero_dy, dev["dy2"], dev["g"])
    want = hashgrid.backward_backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy2"], dev["g"], want_dy=False)[1]
    assert torch.equal(_bits(only_second), _bits(want))


def test_non_finite_input_is_loud_and_no_points_give_zeros():
    c, _, dev, e = _case("one_level_f4")
    for key, at in (("dy", (3, 1)), ("dy2", (64, 0)), ("g", (0, 2))):
        bad = dict(dev)
        bad[key] = dev[key].clone()
        bad[key][at] = float("inf") if key != "g" else float("nan")
        assert torch.isnan(_pair(e, bad)).all(), key
    none = {k: (dev[k][:0] if k != "table" else dev[k]) for k in dev}
    nan = torch.full((e.n_params, c["cfg"][1]), float("nan"), device="cuda")
    assert not _pair(e, none, d_table_out=nan).any()
    assert not torch.isnan(_pair(e, dev)).any()              # the workspace of the loud calls leaves nothing behind
