"""GPU: csrc/hashgrid.hip and csrc/hashgrid_train.hip against the fp64 oracle (tests/_hashgrid_oracle.py) on the inputs of O.CASES:
n in {1, 63, 64, 65, 257, 4099}, L in {1, 2, 16}, F in {1, 2, 4, 8}, log2T in {4, 14, 19}, b in {1, 1.3819, 2}, N in {2, 16}; uniform
points and the mixed set (grid nodes of a random level, faces and edges, exact 0 and 1, -0.25 and 1.5).

Per entry |gpu - oracle64| <= K eps32 S, S the oracle's sum of term magnitudes and K = 5.3 (twice the 2.65 the CPU emulation of the
kernel's arithmetic shows on these inputs; tests/test_hashgrid_oracle.py).  The per-point sums with no emulation (d_x, d_dy) use the
forward bound of their fp32 chain, O.chain_bound.  (Point, level) pairs within 4 ulp32 of a cell face are left out of the Jacobian
comparisons only; there J must match one of the one-sided oracle values.  Table gradients: per entry, the number of contributions
times the fixed-point unit plus K eps32 times the sum of their magnitudes; and they are bitwise reproducible, bitwise invariant
under a permutation of the points, and written whole."""
import functools
import json

import numpy as np
import pytest
import torch

import _hashgrid_oracle as O
from iron_amd import _lib, hashgrid, tcnn_fields

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in O.CASES]
KE = O.K * O.EPS32


def _enc(cfg):
    L, F, log2T, N, b = cfg
    return hashgrid.HashEncoding(L, F, log2T, N, b)


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs, oracle results (computed once, left alone) and the device tensors of one case"""
    c = O.case_inputs(name)
    cfg = c["cfg"]
    ref = dict(enc=O.encode(cfg, c["x"], c["table"]), bwd=O.backward(cfg, c["x"], c["table"], c["dy"]),
               bb=O.backward_backward(cfg, c["x"], c["table"], c["dy"], c["g"]))
    dev = {k: torch.from_numpy(c[k]).cuda() for k in ("x", "table", "dy", "g")}
    e = _enc(cfg)
    return c, ref, dev, e


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _worst(err, tol):
    r = err / np.maximum(tol, 1e-300)
    r[(tol == 0) & (err == 0)] = 0
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_features_and_jacobian_match_the_oracle(name):
    c, ref, dev, e = _case(name)
    cfg, F = c["cfg"], c["cfg"][1]
    y, J = hashgrid.encode(e.desc, e.n_params, dev["x"], dev["table"], jacobian=True)
    y_only = hashgrid.encode(e.desc, e.n_params, dev["x"], dev["table"])
    assert torch.equal(y, y_only)
    r = ref["enc"]
    ey = np.abs(_np(y) - r["y"])
    print("   %s: features worst |err| / (K eps32 S) = %.3f" % (name, _worst(ey, KE * r["Sy"])))
    assert (ey <= KE * r["Sy"]).all()
    near = np.repeat(r["near"], F, axis=1)                       # [n, L F]
    eJ = np.abs(_np(J) - r["J"])
    ok = eJ <= KE * r["SJ"]
    print("   %s: Jacobian worst ratio away from faces %.3f; %.3f %% of the pairs near a face" %
          (name, _worst(eJ[~near], (KE * r["SJ"])[~near]), 100.0 * r["near"].mean()))
    assert ok[~near].all()
    if c["x"].shape[0] > 0 and O.CASES[NAMES.index(name)][3] == "uniform":
        assert r["near"].mean() <= 0.01
    if near.any():                                               # one of the one-sided values, per (point, level)
        match = np.zeros(r["near"].shape, bool)
        for side in range(8):
            s = O.encode(cfg, c["x"], c["table"], side=side)
            good = (np.abs(_np(J) - s["J"]) <= KE * s["SJ"]).all(axis=2)         # [n, L F]
            match |= good.reshape(good.shape[0], cfg[0], F).all(axis=2)
        assert match[r["near"]].all()
    live = (c["x"] >= 0) & (c["x"] <= 1)
    assert not _np(J)[~np.broadcast_to(live[:, None, :], J.shape)].any()         # clamped axes: zero columns


@pytest.mark.parametrize("name", NAMES)
def test_backward_matches_the_oracle(name):
    c, ref, dev, e = _case(name)
    cfg = c["cfg"]
    L, F = cfg[0], cfg[1]
    n = c["x"].shape[0]
    d_table, d_x = hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"])
    r = ref["bwd"]
    unit = hashgrid.grad_unit(float(np.abs(c["dy"]).max()), n)
    tol = r["count"][:, None] * unit + KE * r["mag"]
    et = np.abs(_np(d_table) - r["d_table"])
    print("   %s: d_table worst ratio %.3f (unit 2^%d, up to %d contributions per entry)" %
          (name, _worst(et, tol), int(np.log2(unit)), int(r["count"].max())))
    assert (et <= tol).all()
    untouched = r["count"] == 0
    assert not _np(d_table)[untouched].any() and not np.signbit(d_table.cpu().numpy()[untouched]).any()
    away = ~ref["enc"]["near"].any(axis=1)                       # d_x sums J over the levels: points near a face on any level are left out
    ex = np.abs(_np(d_x) - r["d_x"])
    tx = O.chain_bound(8 * L * F) * O.EPS32 * r["S_dx"]
    print("   %s: d_x worst ratio %.3f of the chain bound (%d of %d points compared)" % (name, _worst(ex[away], tx[away]), away.sum(), n))
    assert (ex[away] <= tx[away]).all()
    only_x = hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], want_table=False)[1]
    assert torch.equal(only_x, d_x)


@pytest.mark.parametrize("name", NAMES)
def test_backward_backward_matches_the_oracle(name):
    c, ref, dev, e = _case(name)
    cfg = c["cfg"]
    L, F = cfg[0], cfg[1]
    n = c["x"].shape[0]
    d_dy, d_table = hashgrid.backward_backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], dev["g"])
    r = ref["bb"]
    near = np.repeat(ref["enc"]["near"], F, axis=1)
    ed = np.abs(_np(d_dy) - r["d_dy"])
    td = O.chain_bound(24) * O.EPS32 * r["S_ddy"]
    print("   %s: d_dy worst ratio %.3f of the chain bound" % (name, _worst(ed[~near], td[~near])))
    assert (ed[~near] <= td[~near]).all()
    lvl = O.level_of_entry(cfg)
    unit = np.array([hashgrid.grad_unit(b, n) for b in r["bound"]])[lvl]
    tol = r["count"][:, None] * unit[:, None] + KE * r["mag"]
    et = np.abs(_np(d_table) - r["d_table"])
    print("   %s: second-order d_table worst ratio %.3f" % (name, _worst(et, tol)))
    assert (et <= tol).all()
    assert not _np(d_table)[r["count"] == 0].any()


@pytest.mark.parametrize("name", ["check_uniform", "hashed_tiny_table", "hashed_f8_nodes", "steep_f4"])
def test_table_gradients_are_bitwise_reproducible_and_order_free(name):
    c, _, dev, e = _case(name)
    n = c["x"].shape[0]
    first = hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], want_x=False)[0]
    second_order = hashgrid.backward_backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], dev["g"], want_dy=False)[1]
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).cuda()
    xp, dyp, gp = dev["x"][perm].contiguous(), dev["dy"][perm].contiguous(), dev["g"][perm].contiguous()
    nan = torch.full((e.n_params, c["cfg"][1]), float("nan"), device="cuda")
    for _ in range(2):
        again = hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], want_x=False, d_table_out=nan.clone())[0]
        assert torch.equal(again.view(torch.int32), first.view(torch.int32))           # runs, and whole-written over NaN
        again2 = hashgrid.backward_backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], dev["g"], want_dy=False,
                                            d_table_out=nan.clone())[1]
        assert torch.equal(again2.view(torch.int32), second_order.view(torch.int32))
    moved = hashgrid.backward(e.desc, e.n_params, xp, dev["table"], dyp, want_x=False)[0]
    assert torch.equal(moved.view(torch.int32), first.view(torch.int32))
    moved2 = hashgrid.backward_backward(e.desc, e.n_params, xp, dev["table"], dyp, gp, want_dy=False)[1]
    assert torch.equal(moved2.view(torch.int32), second_order.view(torch.int32))
    assert not torch.isnan(first).any() and not torch.isnan(second_order).any()


def test_non_finite_gradients_are_loud():
    c, _, dev, e = _case("one_level_f4")
    dy = dev["dy"].clone()
    dy[3, 1] = float("inf")
    assert torch.isnan(hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dy, want_x=False)[0]).all()
    zero = hashgrid.backward(e.desc, e.n_params, dev["x"][:0], dev["table"], dev["dy"][:0], want_x=False)[0]
    assert not zero.any()


@pytest.mark.parametrize("name", ["check_mixed", "equal_levels_f8", "hashed_tiny_table"])
def test_every_row_equals_the_row_computed_alone(name):
    c, _, dev, e = _case(name)
    n = c["x"].shape[0]
    y, J = hashgrid.encode(e.desc, e.n_params, dev["x"], dev["table"], jacobian=True)
    d_x = hashgrid.backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], want_table=False)[1]
    d_dy = hashgrid.backward_backward(e.desc, e.n_params, dev["x"], dev["table"], dev["dy"], dev["g"], want_table=False)[0]
    rows = sorted({0, 1, 62, 63, 64, 65, 255, 256, n // 2, n - 2, n - 1} & set(range(n)))
    for i in rows:
        xi, dyi, gi = dev["x"][i:i + 1].contiguous(), dev["dy"][i:i + 1].contiguous(), dev["g"][i:i + 1].contiguous()
        yi, Ji = hashgrid.encode(e.desc, e.n_params, xi, dev["table"], jacobian=True)
        assert torch.equal(yi[0], y[i]) and torch.equal(Ji[0], J[i])
        assert torch.equal(hashgrid.backward(e.desc, e.n_params, xi, dev["table"], dyi, want_table=False)[1][0], d_x[i])
        assert torch.equal(hashgrid.backward_backward(e.desc, e.n_params, xi, dev["table"], dyi, gi, want_table=False)[0][0], d_dy[i])


# ---- autograd through TCNNSDF ----
FIELD_CFG = (6, 2, 12, 4, 1.5)


def _field(tmp_path, activation="Softplus", n_out=3, cfg=FIELD_CFG, n_neurons=32):
    L, F, log2T, N, b = cfg
    conf = {"encoding": {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": log2T, "base_resolution": N,
                         "per_level_scale": b},
            "network": {"otype": "FullyFusedMLP", "activation": activation, "output_activation": "None", "n_neurons": n_neurons,
                        "n_hidden_layers": 2}}
    p = tmp_path / "field.json"
    p.write_text(json.dumps(conf))
    torch.manual_seed(11)
    f = tcnn_fields.TCNNSDF(str(p), n_outputs_dims=n_out)
    with torch.no_grad():
        f.sdf_encoding.params.uniform_(-0.1, 0.1)          # the +-1e-4 start would leave every gradient through the table tiny
    return f.cuda()


def _restated_grads(field, x, eik_weight):
    """The same loss on the plain-torch restatement in fp64 on the device -> gradients of the table and of every head weight."""
    import copy
    head = copy.deepcopy(field.sdf_network).double()
    table = field.sdf_encoding.params.detach().double().requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    out = head(O.restate(FIELD_CFG, x64, table))
    loss = (out[:, :1] ** 2).mean() + out[:, 1:].mean()
    if eik_weight:
        (nrm,) = torch.autograd.grad(out[:, :1].sum(), x64, create_graph=True)
        loss = loss + eik_weight * ((nrm.norm(dim=-1) - 1.0) ** 2).mean()
    loss.backward()
    return float(loss.detach()), [table.grad] + [p.grad for p in head.parameters()]


@pytest.mark.parametrize("eik_weight", [0.0, 0.1])
def test_first_order_and_eikonal_gradients_on_the_field(tmp_path, eik_weight):
    """loss.backward() after torch.autograd.grad(y, x, create_graph=True), the reference's pattern, against the fp64 restatement.
    Tolerance: rel-L2 1e-4 per tensor.  The fp32 path rounds at eps32 / 2 = 6e-8 per operation; a gradient entry passes through
    some 30 of them (three layers forward, backward and double backward) and is a sum over 500 points of terms that cancel to a few
    per cent of their magnitude, so 30 x 6e-8 x ~50 = 1e-4 bounds the relative error of the tensor's norm."""
    field = _field(tmp_path)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(500, 3, generator=g) * 0.98 + 0.01).cuda()
    want_loss, want = _restated_grads(field, x, eik_weight)
    field.zero_grad()
    if eik_weight:
        sdf, feat, nrm = field.get_all(x.clone(), is_training=True)
        loss = (sdf ** 2).mean() + feat.mean() + eik_weight * ((nrm.norm(dim=-1) - 1.0) ** 2).mean()
    else:
        out = field(x)
        loss = (out[:, :1] ** 2).mean() + out[:, 1:].mean()
    loss.backward()
    assert abs(float(loss.detach()) - want_loss) <= 1e-5 * abs(want_loss)
    got = [field.sdf_encoding.params.grad] + [p.grad for p in field.sdf_network.parameters()]
    for k, (a, b) in enumerate(zip(got, want)):
        rel = float((a.double() - b).norm() / b.norm())
        print("   eik_weight %.1f tensor %d: rel-L2 %.2e (norm %.3e)" % (eik_weight, k, rel, float(b.norm())))
        assert rel <= 1e-4, (k, rel)


def test_field_interface_and_refusals(tmp_path):
    field = _field(tmp_path)
    x = torch.rand(4, 5, 3, generator=torch.Generator().manual_seed(1)).cuda()
    assert field(x).shape == (4, 5, 3) and field.sdf(x).shape == (4, 5, 1) and field.sdf_hidden_appearance(x).shape == (4, 5, 3)
    flat = x.reshape(-1, 3).clone()
    sdf, feat, nrm = field.get_all(flat, is_training=False)
    assert sdf.shape == (20, 1) and feat.shape == (20, 2) and nrm.shape == (20, 3)
    assert not sdf.requires_grad and not feat.requires_grad and not nrm.requires_grad and flat.requires_grad
    grad = field.gradient(x.reshape(-1, 3).clone())
    assert grad.requires_grad and torch.equal(grad.detach(), nrm)
    y, J = field.sdf_encoding.jacobian(flat.detach())
    assert J.shape == (20, 12, 3) and torch.equal(y, field.sdf_encoding(flat.detach()))
    # a leaf x that requires grad is fine; an x with a history is refused under create_graph, where its term would go missing
    leaf = flat.detach().clone().requires_grad_(True)
    mid = leaf * 1.0
    out = field.sdf_encoding(mid)
    (d_mid,) = torch.autograd.grad(out.sum(), mid, retain_graph=True)            # first order through a non-leaf: supported
    assert torch.equal(d_mid, torch.autograd.grad(field.sdf_encoding(leaf).sum(), leaf)[0])
    with pytest.raises(NotImplementedError, match="create_graph"):
        torch.autograd.grad(out.sum(), mid, create_graph=True)
    with pytest.raises(_lib.IronError, match="CUDA"):
        field.sdf_encoding(flat.detach().cpu())
    with pytest.raises(_lib.IronError, match="float32"):
        field.sdf_encoding(flat.detach().double())


def test_a_plane_held_by_one_dense_level_traces_like_the_analytic_plane(tmp_path):
    """sdf = n.p - c stored at the nodes of one dense level (trilinear interpolation reproduces an affine field), traced through
    SDFCallable against the analytic callable: equal masks, hit distances within sdf_threshold / cos(ray, plane normal).  World
    [-1, 1]^3 maps to [0, 0.9]^3, below the level's wrapped top face (x > 1 - 1 / scale)."""
    from iron_amd import scenes
    from iron_amd.raytracer import Camera, RayTracer, SDFCallable, intersect_sphere
    field = _field(tmp_path, activation="None", n_out=1, cfg=(1, 1, 19, 16, 1.0), n_neurons=16)
    (lv,) = field.sdf_encoding.levels
    assert lv["dense"] and lv["scale"] == 15.0
    nrm, off = np.array([0.36, 0.48, 0.8]), 0.1
    r = lv["res"]
    k = np.arange(r ** 3)
    nodes = np.stack([k % r, (k // r) % r, k // (r * r)], axis=1)
    world = ((nodes - 0.5) / lv["scale"]) / 0.45 - 1.0
    table = np.zeros(lv["size"])
    table[:r ** 3] = world @ nrm - off
    with torch.no_grad():
        field.sdf_encoding.params.copy_(torch.from_numpy(table.astype(np.float32)))
        lin = [m for m in field.sdf_network if isinstance(m, torch.nn.Linear)]
        for m in lin:
            m.weight.zero_()
            m.weight[0, 0] = 1.0                                  # the head passes feature 0 through
    K, W2C = scenes.fixture_camera_matrices(48, 48)
    cam = Camera(48, 48, K.cuda(), W2C.cuda())
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(o, d, 1.0)
    nt = torch.tensor(nrm, dtype=torch.float32, device="cuda")
    tr = RayTracer()
    got = tr(SDFCallable(lambda x: field.sdf((x + 1.0) * 0.45)[..., 0]), o, d, near, far, hit)
    want = tr(SDFCallable(lambda x: x @ nt - off), o, d, near, far, hit)
    torch.cuda.synchronize()
    both = want["convergent_mask"]
    print("   plane: %d of %d rays converge" % (int(both.sum()), both.numel()))
    assert int(both.sum()) >= 200
    assert torch.equal(got["convergent_mask"], both)
    cos = (d @ nt).abs()[both]
    gap = (got["distance"][both] - want["distance"][both]).abs()
    print("   plane: worst distance gap x cos / sdf_threshold = %.3f" % float((gap * cos / tr.sdf_threshold).max()))
    assert (gap <= tr.sdf_threshold / cos).all()


def test_the_input_gradient_does_not_run_the_table_scatter(tmp_path, monkeypatch):
    """torch.autograd.grad(y, x) discards the table gradient, so the scatter must not run there; loss.backward() runs it once per
    order."""
    field = _field(tmp_path)
    calls = []
    real_b, real_bb = hashgrid.backward, hashgrid.backward_backward

    def spy_b(*a, **k):
        calls.append(("backward", k.get("want_table", True), k.get("want_x", True)))
        return real_b(*a, **k)

    def spy_bb(*a, **k):
        calls.append(("backward_backward", k.get("want_dy", True), k.get("want_table", True)))
        return real_bb(*a, **k)

    monkeypatch.setattr(hashgrid, "backward", spy_b)
    monkeypatch.setattr(hashgrid, "backward_backward", spy_bb)
    x = torch.rand(100, 3, generator=torch.Generator().manual_seed(2)).cuda()
    sdf, _, nrm = field.get_all(x, is_training=True)
    assert calls == [("backward", False, True)]
    del calls[:]
    ((sdf ** 2).mean() + ((nrm.norm(dim=-1) - 1.0) ** 2).mean()).backward()
    assert ("backward_backward", True, True) in calls and ("backward", True, False) in calls
    assert sum(c[0] == "backward" and c[1] for c in calls) == 1 and sum(c[0] == "backward_backward" for c in calls) == 1
    with torch.no_grad():
        del calls[:]
        field(x.detach())
        assert calls == []
