"""GPU: the fused training backward of the hash-grid field (iron_amd/csrc/hashgrid_field_train.hip; TCNNSDF.fused_training; DESIGN.md
§29) against the fp64 oracle of tests/_hashfield_train_oracle.py on the inputs of _hashgrid_oracle.CASES (n = 1, 63, 64, 65, 257,
4099) and slices of check_uniform of C - 1, C, C + 1 and 2 C + 1 points, C = iron_hashgrid_field_train_slot(n).

Tolerances (none measured on the kernel): ybar, e and every weight gradient eps32 (C_TRAIN[quantity] S + F) with the oracle's scales
(signed-Jacobian scales for ybar and e; each quantity's constant is twice its own emulation's worst ratio); the table
count unit_l + K eps32 mag + what the tolerances of ybar and e let through the scatter, unit_l the pair scatter's unit formed from the
maxima of the kernel's own ybar and e.  Rows of d_out and d_g are zero at points within tolerance of a ReLU kink, rows of d_g at points
within 4 ulp32 of a face (T.case_adjoints); e does not see the adjoints and is compared away from kinks.
The pair scatter's own tests are tests/test_gpu_hashgrid_pair.py."""
import functools

import numpy as np
import pytest
import torch

import _hashfield_oracle as H
import _hashfield_train_oracle as T
import _hashgrid_oracle as O
from iron_amd import _lib, hashgrid, tcnn_fields
from test_gpu_hashfield import make_field

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in O.CASES]
KE = O.K * O.EPS32


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _worst(err, tol):
    r = err / np.maximum(tol, 1e-300)
    r[(tol == 0) & (err == 0)] = 0
    return float(r.max()) if r.size else 0.0


@functools.lru_cache(maxsize=None)
def _field(name, head, n_out, act):
    c, _ = H.case_encoding(name)
    return make_field(c["cfg"], head, act, n_out, c["table"], H.case_weights(name, head, n_out))


def _run(field, p, d_out, d_g, scale=None, offset=None, want_table=True):
    """iron_hashgrid_field_backward on numpy inputs -> torch (d_weights, d_table, ybar, e)"""
    desc = field._train_desc()
    dev = field.sdf_encoding.params.device
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return tcnn_fields.field_backward(desc, t(p), field.sdf_encoding.params.detach(), field._fused_packed(desc, dev),
                                      field._train_packed(desc, dev), t(d_out), t(d_g), scale=scale, offset=offset, want_table=want_table,
                                      want_rows=True)


def _compare(tag, cfg, x, table, ref, got, keep_e, vp_max):
    """every quantity against the oracle; prints the worst ratio per quantity"""
    d_weights, d_table, ybar, e = got
    n = x.shape[0]
    worst = {}
    for key, val, rows in (("ybar", ybar, slice(None)), ("e", e, keep_e)):
        err, tl = np.abs(_np(val) - ref[key][0]), T.tol(ref[key], key)
        worst[key] = _worst(err[rows], tl[rows])
        assert (err <= tl)[rows].all(), (tag, key, worst[key])
    flat, S, worst["Wbar"] = _np(d_weights), 0, 0.0
    for l, q in enumerate(ref["Wbar"]):
        err, tl = np.abs(flat[S:S + q[0].size].reshape(q[0].shape) - q[0]), T.tol(q, "Wbar")
        worst["Wbar"] = max(worst["Wbar"], _worst(err, tl))
        assert (err <= tl).all(), (tag, "Wbar_%d" % l, worst["Wbar"])
        S += q[0].size
    assert S == flat.size
    if d_table is not None:
        tab = T.table_reference(cfg, x, table, ref)
        levels, _ = O.levels_of(cfg)
        m1, m2 = np.float32(np.abs(ybar.cpu().numpy()).max()), np.float32(np.abs(e.cpu().numpy()).max())
        bound = [np.float32(m1 + (np.float32(3.0) * np.float32(vp_max)) * np.float32(lv["scale"]) * m2) for lv in levels]
        unit = np.array([hashgrid.grad_unit(float(b), n) for b in bound])[O.level_of_entry(cfg)][:, None]
        tl = tab["count"][:, None] * unit + KE * tab["mag"] + tab["through"]
        err = np.abs(_np(d_table).reshape(tab["d_table"].shape) - tab["d_table"])
        worst["table"] = _worst(err, tl)
        assert (err <= tl).all(), (tag, "d_table", worst["table"])
        assert not _np(d_table).reshape(tab["d_table"].shape)[tab["count"] == 0].any()
    print("   %s: worst |err| / tol: %s" % (tag, ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("head", T.HEADS, ids=lambda h: "%dx%d" % h)
@pytest.mark.parametrize("name", NAMES)
def test_backward_matches_the_oracle(name, head):
    c, _ = H.case_encoding(name)
    for (_, _, n_out, act) in [k for k in T.combos() if k[0] == name and k[1] == head]:
        d_out, d_g, _, _ = T.case_adjoints(name, head, n_out, act)
        ref = T.reference(name, head, n_out, act)
        got = _run(_field(name, head, n_out, act), c["x"], d_out, d_g)
        _compare("%s %s %s n_out %d" % (name, head, act, n_out), c["cfg"], c["x"], c["table"], ref, got,
                 ~H.reference(name, head, n_out, act)["kink"], np.abs(ref["vp"]).max())


VARIANT_COMBOS = [("check_mixed", (32, 2), "Softplus"), ("steep_f4", (64, 4), "ReLU"), ("hashed_tiny_table", (16, 1), "None"),
                  ("equal_levels_f8", (64, 2), "Softplus")]


@pytest.mark.parametrize("variant", ["no_d_out", "no_d_g", "affine_map"])
@pytest.mark.parametrize("name,head,act", VARIANT_COMBOS)
def test_absent_adjoints_and_the_affine_map(name, head, act, variant):
    n_out = [k for k in T.combos({act}) if k[0] == name and k[1] == head][0][2]
    c, enc = H.case_encoding(name)
    d_out, d_g, _, _ = T.case_adjoints(name, head, n_out, act)
    field, W = _field(name, head, n_out, act), H.case_weights(name, head, n_out)
    keep = ~H.reference(name, head, n_out, act)["kink"]
    if variant == "affine_map":
        # the field sees x = 0.5 p + 0.5; p = 2 x - 1 is exact in fp32 wherever x is a multiple of 2^-24, so round x there first
        x = (np.round(c["x"].astype(np.float64) * 2.0 ** 23) / 2.0 ** 23).astype(np.float32)
        p = (2.0 * x.astype(np.float64) - 1.0).astype(np.float32)
        assert ((p.astype(np.float64) * 0.5 + 0.5) == x).all()
        near = O.encode(c["cfg"], x, c["table"])["near"].any(axis=1)
        kink = H.evaluate(c["cfg"], x, c["table"], W, act)["kink"]
        d_out, d_g = d_out.copy(), d_g.copy()
        d_out[kink] = 0.0
        d_g[kink | near] = 0.0
        assert int(kink.sum()) <= max(2, x.shape[0] // 100)
        ref = T.backward(c["cfg"], x, c["table"], W, act, d_out, d_g, (0.5, 0.5, 0.5))
        got = _run(field, p, d_out, d_g, scale=0.5, offset=0.5)
        keep = ~kink
    else:
        x = c["x"]
        zo, zg = (np.zeros_like(d_out), d_g) if variant == "no_d_out" else (d_out, np.zeros_like(d_g))
        ref = T.backward(c["cfg"], x, c["table"], W, act, zo, zg, enc=enc)
        got = _run(field, x, None if variant == "no_d_out" else d_out, None if variant == "no_d_g" else d_g)
    _compare("%s %s %s %s" % (name, head, act, variant), c["cfg"], x, c["table"], ref, got, keep, np.abs(ref["vp"]).max())


@pytest.mark.parametrize("head,act", [((64, 2), "ReLU"), ((32, 2), "Softplus")])
def test_slices_at_the_slot_edges_match_the_oracle(head, act):
    name = "check_uniform"
    n_out = [k for k in T.combos({act}) if k[0] == name and k[1] == head][0][2]
    c, _ = H.case_encoding(name)
    d_out, d_g, _, _ = T.case_adjoints(name, head, n_out, act)
    field, W = _field(name, head, n_out, act), H.case_weights(name, head, n_out)
    kink = H.reference(name, head, n_out, act)["kink"]
    for first in (0, 1000):
        Cn = _lib.load_train().iron_hashgrid_field_train_slot(4099)
        for k in (Cn - 1, Cn, Cn + 1, 2 * Cn + 1):
            rows = slice(first, first + k)
            assert _lib.load_train().iron_hashgrid_field_train_slot(k) == Cn
            ref = T.backward(c["cfg"], c["x"][rows], c["table"], W, act, d_out[rows], d_g[rows])
            got = _run(field, c["x"][rows], d_out[rows], d_g[rows])
            _compare("%s %s rows %d..%d" % (head, act, first, first + k), c["cfg"], c["x"][rows], c["table"], ref, got, ~kink[rows],
                     np.abs(ref["vp"]).max())


def test_slots_of_two_point_tiles_match_the_oracle():
    """n = 65 537: C(n) = 128, so with 64 points per tile every slot carries its accumulator tiles from one point tile to the next
    (at n <= 65 536 a slot is one tile there).  One dense level keeps the oracle cheap; Softplus: no kinks, every buffer in use."""
    cfg, head, n_out, act, n = (1, 4, 14, 16, 1.0), (32, 2), 3, "Softplus", 65537
    assert _lib.load_train().iron_hashgrid_field_train_slot(n) == 128
    rng = np.random.default_rng(99)
    _, P = O.levels_of(cfg)
    x = rng.random((n, 3)).astype(np.float32)
    table = (rng.random((P, cfg[1])) * 0.2 - 0.1).astype(np.float32)
    d_out = (rng.random((n, n_out)) * 2 - 1).astype(np.float32)
    d_g = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    d_g[O.encode(cfg, x, table)["near"].any(axis=1)] = 0.0
    W = H.head_weights(cfg[0] * cfg[1], head[0], head[1], n_out, seed=4242)
    ref = T.backward(cfg, x, table, W, act, d_out, d_g)
    got = _run(make_field(cfg, head, act, n_out, table, W), x, d_out, d_g)
    _compare("65537 points %s %s" % (head, act), cfg, x, table, ref, got, slice(None), np.abs(ref["vp"]).max())


def _slot_sum64(parts):
    """fixed_sum::slot_sum<64> over parts [slots, n_weights] (fp64): thread t adds slots t, t + 64, ..; then the halving tree"""
    v = np.zeros((64,) + parts.shape[1:])
    for i in range(parts.shape[0]):
        v[i % 64] = v[i % 64] + parts[i]
    s = 32
    while s > 0:
        v[:s] = v[:s] + v[s:2 * s]
        s //= 2
    return v[0]


@pytest.mark.parametrize("name,head,act", [("check_uniform", (64, 2), "ReLU"), ("hashed_tiny_table", (32, 2), "Softplus")])
def test_reproducible_order_free_and_rows_and_slots_independent(name, head, act):
    n_out = [k for k in T.combos({act}) if k[0] == name and k[1] == head][0][2]
    c, _ = H.case_encoding(name)
    d_out, d_g, _, _ = T.case_adjoints(name, head, n_out, act)
    field = _field(name, head, n_out, act)
    x, n = c["x"], c["x"].shape[0]
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    first = _run(field, x, d_out, d_g)
    again = _run(field, x, d_out, d_g)
    for a, b in zip(first, again):
        assert torch.equal(bits(a), bits(b))
    perm = np.random.default_rng(5).permutation(n)
    moved = _run(field, x[perm], d_out[perm], d_g[perm])
    assert torch.equal(bits(moved[1]), bits(first[1]))                       # d_table: any order of the points
    assert torch.equal(bits(moved[2]), bits(first[2][torch.from_numpy(perm).cuda()]))
    rows = np.array(sorted({0, 1, 63, 64, 65, 127, 128, 2000, n - 2, n - 1}))
    sub = _run(field, x[rows], d_out[rows], d_g[rows], want_table=False)
    at = torch.from_numpy(rows).cuda()
    assert torch.equal(bits(sub[2]), bits(first[2][at])) and torch.equal(bits(sub[3]), bits(first[3][at]))
    # a slot's partial depends on its own points alone: d_weights is the fixed-order fp64 sum of the single-slot calls' d_weights
    Cn = _lib.load_train().iron_hashgrid_field_train_slot(n)
    parts = np.stack([_np(_run(field, x[s:s + Cn], d_out[s:s + Cn], d_g[s:s + Cn], want_table=False)[0]) for s in range(0, n, Cn)])
    want = _slot_sum64(parts).astype(np.float32)
    assert np.array_equal(want.view(np.int32), first[0].cpu().numpy().view(np.int32))


# ---- module level ----
def _masked_loss(field, x, keep_v, keep_g):
    sdf, feat, grad = field.get_all(x.clone(), is_training=True)
    loss = ((sdf[:, 0] ** 2) * keep_v).mean() + (feat.sum(dim=-1) * keep_v).mean() + 0.1 * (((grad.norm(dim=-1) - 1.0) ** 2) * keep_g).mean()
    return loss, sdf, feat, grad


def _grads(field):
    return [field.sdf_encoding.params.grad.clone()] + [p.grad.clone() for p in field.sdf_network.parameters()]


def test_module_gradients_match_the_oracle_and_the_flag_switches_back():
    name, head, n_out, act = "check_mixed", (32, 2), 3, "Softplus"
    c, enc = H.case_encoding(name)
    W = H.case_weights(name, head, n_out)
    field = make_field(c["cfg"], head, act, n_out, c["table"], W)
    hr = H.reference(name, head, n_out, act)
    x = torch.from_numpy(c["x"]).cuda()
    keep_v = torch.from_numpy((~hr["kink"]).astype(np.float32)).cuda()
    keep_g = torch.from_numpy((~(hr["kink"] | hr["near"])).astype(np.float32)).cuda()
    assert not field.fused_training and field.fused_training_supported() and "fused_training" not in field.state_dict()
    field.zero_grad()
    _masked_loss(field, x, keep_v, keep_g)[0].backward()
    plain = _grads(field)

    field.fused_training = True
    field.zero_grad()
    loss, sdf, feat, grad = _masked_loss(field, x, keep_v, keep_g)
    out_f, grad_f = field.eval_fused(x, gradient=True)
    assert torch.equal(sdf, out_f[:, :1]) and torch.equal(feat, out_f[:, 1:]) and torch.equal(grad, grad_f)     # the forward IS eval_fused
    assert torch.equal(field(x), out_f) and torch.equal(field.sdf(x), out_f[:, :1]) and torch.equal(field.gradient(x.clone()), grad_f)
    d_sdf, d_feat, d_g = torch.autograd.grad(loss, (sdf, feat, grad), retain_graph=True)      # the adjoints the backward receives
    loss.backward()
    fused = _grads(field)
    d_out = torch.cat([d_sdf, d_feat], dim=1).cpu().numpy()
    ref = T.backward(c["cfg"], c["x"], c["table"], W, act, d_out, d_g.cpu().numpy(), enc=enc)
    assert not d_out[hr["kink"]].any() and not d_g.cpu().numpy()[hr["kink"] | hr["near"]].any()
    for l, q in enumerate(ref["Wbar"]):
        err, tl = np.abs(_np(fused[1 + l]) - q[0]), T.tol(q, "Wbar")
        print("   module: Wbar_%d worst |err| / tol %.3f" % (l, _worst(err, tl)))
        assert (err <= tl).all()
    tab = T.table_reference(c["cfg"], c["x"], c["table"], ref)
    got = _run(field, c["x"], d_out, d_g.cpu().numpy())
    assert torch.equal(got[1].view(-1), fused[0].view(-1))                   # the module hands the table gradient through untouched
    _compare("module check_mixed", c["cfg"], c["x"], c["table"], ref, got, ~hr["kink"], np.abs(ref["vp"]).max())
    for a, b in zip(plain, fused):                                           # and the two paths agree as two fp32 computations do
        assert float((a.double() - b.double()).norm() / b.double().norm()) <= 1e-4

    field.fused_training = False
    field.zero_grad()
    _masked_loss(field, x, keep_v, keep_g)[0].backward()
    for a, b in zip(plain, _grads(field)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_an_optimiser_step_reaches_the_next_fused_step():
    name, head, n_out, act = "one_level_f4", (16, 1), 1, "ReLU"
    c, _ = H.case_encoding(name)
    n_out = [k for k in T.combos({act}) if k[0] == name and k[1] == head][0][2]
    field = make_field(c["cfg"], head, act, n_out, c["table"], H.case_weights(name, head, n_out))
    field.fused_training = True
    x = torch.from_numpy(c["x"]).cuda()
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    before = field(x).detach().clone()
    sdf, _, grad = field.get_all(x.clone())
    ((sdf ** 2).mean() + ((grad.norm(dim=-1) - 1.0) ** 2).mean()).backward()
    opt.step()
    after = field(x)
    assert not torch.equal(after, before) and torch.equal(after, field.eval_fused(x))
    fresh = make_field(c["cfg"], head, act, n_out, field.sdf_encoding.params.detach().cpu().numpy(),
                       [m.weight.detach().cpu().numpy() for m in field.sdf_network if isinstance(m, torch.nn.Linear)])
    fresh.fused_training = True
    for f in (field, fresh):
        f.zero_grad()
        sdf, _, grad = f.get_all(x.clone())
        ((sdf ** 2).mean() + ((grad.norm(dim=-1) - 1.0) ** 2).mean()).backward()
    for a, b in zip(_grads(field), _grads(fresh)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_refusals():
    c, _ = H.case_encoding("one_level_f4")
    field = make_field(c["cfg"], (16, 1), "ReLU", 1)
    field.fused_training = True
    x = torch.from_numpy(c["x"]).cuda()
    with pytest.raises(_lib.IronError, match="CUDA"):
        field(x.cpu())
    with pytest.raises(_lib.IronError, match="float32"):
        field(x.double())
    with pytest.raises(_lib.IronError, match="leaf"):
        field.get_all(x.clone().requires_grad_(True) * 1.0)
    with pytest.raises(_lib.IronError, match="leaf"):
        field((x.clone().requires_grad_(True) * 1.0))
    with torch.no_grad():
        assert torch.equal(field(x), field.eval_fused(x))
    sdf, _, grad = field.get_all(x.clone())
    with pytest.raises(_lib.IronError, match="second backward"):
        torch.autograd.grad(((grad.norm(dim=-1) - 1.0) ** 2).mean() + sdf.mean(), list(field.parameters()), create_graph=True)
    wide = make_field(c["cfg"], (128, 3), "ReLU", 1)
    assert wide.fused_supported() and not wide.fused_training_supported()
    wide.fused_training = True
    with pytest.raises(_lib.IronError, match="n_neurons"):
        wide(x)
    d = field._train_desc()
    none = tcnn_fields.field_backward(d, x[:0], field.sdf_encoding.params.detach(), field._fused_packed(d, x.device),
                                      field._train_packed(d, x.device), None, None)
    assert not none[0].any() and not none[1].any()


def test_the_sphere_fit_with_the_fused_step(tmp_path):
    import test_gpu_hashgrid_fit as fit_mod
    results = {}
    for fused in (False, True):
        field = fit_mod.make_field(tmp_path / ("fit%d.json" % fused)).cuda()
        field.fused_training = fused

        def f(x, field=field):
            sdf, _, grad = field.get_all(x, is_training=True)
            return sdf, grad

        results[fused] = fit_mod.fit(list(field.parameters()), f, torch.device("cuda"))
    (p0, p1), (f0, f1) = results[False], results[True]
    print("   sphere fit, %d steps: fused %.3e -> %.3e (1 / %.0f); plain %.3e -> %.3e (1 / %.0f)"
          % (fit_mod.STEPS, f0, f1, f0 / f1, p0, p1, p0 / p1))
    assert f1 <= f0 / 10.0
