"""GPU: the fused hash-grid field evaluation (iron_amd/csrc/hashgrid_field.hip; TCNNSDF.eval_fused / as_callable) against the fp64
oracle of tests/_hashfield_oracle.py on the inputs of _hashgrid_oracle.CASES and the heads of _hashfield_oracle.HEADS:
|gpu - oracle| <= eps32 (C_HEAD S + F) per row and output.  A workgroup takes 64 points (two 32-column MFMA tiles),
32 where the stages of 64 would not fit in 64 KiB of LDS: the prefix sizes 31 .. 65 of check_uniform sit on both tiles' edges."""
import functools
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import _hashfield_oracle as H
import _hashgrid_oracle as O
from iron_amd import _lib, tcnn_fields

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in O.CASES]
PREFIXES = (1, 31, 32, 33, 63, 64, 65, 257)
_TMP = tempfile.TemporaryDirectory()


def make_field(cfg, head, act, n_out, table=None, weights=None):
    L, F, log2T, N, b = cfg
    conf = {"encoding": {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": log2T, "base_resolution": N,
                         "per_level_scale": b},
            "network": {"otype": "FullyFusedMLP", "activation": act, "output_activation": "None", "n_neurons": head[0],
                        "n_hidden_layers": head[1]}}
    fd, path = tempfile.mkstemp(suffix=".json", dir=_TMP.name)
    with os.fdopen(fd, "w") as f:
        json.dump(conf, f)
    field = tcnn_fields.TCNNSDF(path, n_outputs_dims=n_out)
    with torch.no_grad():
        if table is not None:
            field.sdf_encoding.params.copy_(torch.from_numpy(table).reshape(-1))
        if weights is not None:
            lin = [m for m in field.sdf_network if isinstance(m, torch.nn.Linear)]
            for m, w in zip(lin, weights):
                m.weight.copy_(torch.from_numpy(w))
    return field.cuda()


@functools.lru_cache(maxsize=None)
def _setup(name, head, n_out, act):
    """inputs, the oracle's results (computed once, left alone), the field and x on the device"""
    c, _ = H.case_encoding(name)
    field = make_field(c["cfg"], head, act, n_out, c["table"], H.case_weights(name, head, n_out))
    return c, H.reference(name, head, n_out, act), field, torch.from_numpy(c["x"]).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _worst(err, tol):
    r = err / np.maximum(tol, 1e-300)
    r[(tol == 0) & (err == 0)] = 0
    return float(r.max()) if r.size else 0.0


def _combos(name, head):
    return [k for k in H.combos() if k[0] == name and k[1] == head]


@pytest.mark.parametrize("head", H.HEADS, ids=lambda h: "%dx%d" % h)
@pytest.mark.parametrize("name", NAMES)
def test_values_and_gradients_match_the_oracle(name, head):
    """Values: every row and output, all three activations, no point left out.  Gradients: per component; points near a ReLU kink and
    points with a level near a face are left out under the caps (printed and asserted); axes outside [0, 1] are exactly zero."""
    for (_, _, n_out, act) in _combos(name, head):
        c, ref, field, x = _setup(name, head, n_out, act)
        n = x.shape[0]
        out = field.eval_fused(x)
        out_g, grad = field.eval_fused(x, gradient=True)
        assert out.shape == (n, n_out) and grad.shape == (n, 3) and not out.requires_grad and not grad.requires_grad
        assert torch.equal(out, out_g)                                           # the value does not depend on asking for the gradient
        ev = np.abs(_np(out) - ref["out"])
        print("   %s %s %s n_out %d: value worst |err| / tol = %.3f" % (name, head, act, n_out, _worst(ev, H.tol(ref, "out"))))
        assert (ev <= H.tol(ref, "out")).all()
        left = ref["near"] | ref["kink"]
        eg = np.abs(_np(grad) - ref["grad"])
        print("   %s %s %s: gradient worst |err| / tol = %.3f; left out: %d near a kink, %d with a level near a face, of %d" %
              (name, head, act, _worst(eg[~left], H.tol(ref, "grad")[~left]), int(ref["kink"].sum()), int(ref["near"].sum()), n))
        assert (eg <= H.tol(ref, "grad"))[~left].all()
        assert int(ref["kink"].sum()) <= max(2, n // 100)
        if O.CASES[NAMES.index(name)][3] == "uniform":
            assert H.case_encoding(name)[1]["near"].mean() <= 0.01               # (point, level) pairs, as DESIGN §27 states
        live = (c["x"] >= 0) & (c["x"] <= 1)
        assert not _np(grad)[~live].any()
        if name == "check_uniform":                                              # the edges of the 32-column tile and of the point tile
            for k in PREFIXES:
                o_k, g_k = field.eval_fused(x[:k], gradient=True)
                assert torch.equal(o_k, out[:k]) and torch.equal(g_k, grad[:k])


@pytest.mark.parametrize("name,head,act", [("check_mixed", (64, 2), "ReLU"), ("check_uniform", (128, 3), "Softplus"),
                                           ("hashed_f8_nodes", (16, 1), "None"), ("steep_f4", (64, 4), "ReLU")])
def test_runs_are_reproducible_and_rows_independent(name, head, act):
    n_out = [k for k in _combos(name, head) if k[3] == act][0][2]
    c, ref, field, x = _setup(name, head, n_out, act)
    n = x.shape[0]
    out, grad = field.eval_fused(x, gradient=True)
    out2, grad2 = field.eval_fused(x, gradient=True)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).cuda()
    out_p, grad_p = field.eval_fused(x[perm], gradient=True)
    assert torch.equal(out_p, out[perm]) and torch.equal(grad_p, grad[perm])
    assert torch.equal(field.eval_fused(x[perm]), out[perm])
    for i in (0, n // 2, n - 1):
        o1, g1 = field.eval_fused(x[i:i + 1], gradient=True)
        assert torch.equal(o1, out[i:i + 1]) and torch.equal(g1, grad[i:i + 1])
    # a NaN row leaves the other rows' bits alone
    xn = x.clone()
    xn[n // 3] = float("nan")
    on, gn = field.eval_fused(xn, gradient=True)
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[n // 3] = False
    assert torch.equal(on[keep], out[keep]) and torch.equal(gn[keep], grad[keep])
    # empty input
    oe, ge = field.eval_fused(x[:0], gradient=True)
    assert oe.shape == (0, n_out) and ge.shape == (0, 3)
    assert field.eval_fused(x[:0].reshape(0, 2, 3)).shape == (0, 2, n_out)


@pytest.mark.parametrize("scale", [0.5, 0.25, 2.0])
def test_affine_map_equals_mapping_the_points_first(scale):
    """A power-of-two scale makes p * scale exact, so fma(p, scale, offset) and p * scale + offset round once, to the same bits."""
    c, ref, field, x = _setup("check_mixed", (64, 2), 3, "ReLU")
    offset = (0.3, -0.0625, 0.1234567)
    off = torch.tensor(offset, dtype=torch.float32, device="cuda")
    p = (x - off) / scale                                                         # lands near the case's points, clamped ones included
    mapped = p * scale + off
    out, grad = field.eval_fused(p, gradient=True, scale=scale, offset=offset)
    want, wgrad = field.eval_fused(mapped, gradient=True)
    assert torch.equal(out, want)
    assert torch.equal(grad, wgrad * scale)
    assert torch.equal(field.eval_fused(p, scale=scale, offset=offset), want)
    o1, g1 = field.eval_fused(x, gradient=True, scale=1.0, offset=0.0)
    o0, g0 = field.eval_fused(x, gradient=True)
    assert torch.equal(o1, o0) and torch.equal(g1, g0)
    o3 = field.eval_fused(p, scale=(scale, scale, scale), offset=off)            # three numbers / a tensor are the same map
    assert torch.equal(o3, want)


@pytest.mark.parametrize("act", H.ACTS)
def test_fused_agrees_with_the_plain_path_and_leaves_it_alone(act):
    """A consistency check (the oracle is the yardstick): the plain path sums in an order of the GEMM library's choosing, for which
    the first-order bound eps32 (S + F) holds whatever the order; the fused side has its own tolerance."""
    name, head = "check_uniform", (64, 2)
    n_out = [k for k in _combos(name, head) if k[3] == act][0][2]
    c, ref, field, x = _setup(name, head, n_out, act)
    keys = list(field.state_dict().keys())
    with torch.no_grad():
        before = field.sdf(x)
    out, grad = field.eval_fused(x, gradient=True)
    with torch.no_grad():
        after = field.sdf(x)
    assert torch.equal(before, after)
    sdf, feat, g = field.get_all(x.clone(), is_training=False)
    both_v = H.tol(ref, "out") + O.EPS32 * (ref["S_out"] + ref["F_out"])
    both_g = H.tol(ref, "grad") + O.EPS32 * (ref["S_grad"] + ref["F_grad"])
    assert (np.abs(_np(out[:, :1]) - _np(before)) <= both_v[:, :1]).all()
    assert (np.abs(_np(out) - _np(torch.cat([sdf, feat], dim=1))) <= both_v).all()
    left = ref["near"] | ref["kink"]
    assert (np.abs(_np(grad) - _np(g)) <= both_g)[~left].all()
    assert list(field.state_dict().keys()) == keys


def test_packed_weights_follow_an_optimiser_step():
    c, _ = H.case_encoding("check_mixed")
    head, n_out, act = (32, 2), 3, "Softplus"
    field = make_field(c["cfg"], head, act, n_out, c["table"], H.case_weights("check_mixed", head, n_out))
    keys = list(field.state_dict().keys())
    x = torch.from_numpy(c["x"]).cuda()
    first = field.eval_fused(x)
    opt = torch.optim.Adam(field.sdf_network.parameters(), lr=1e-2)
    field.sdf(x).square().sum().backward()
    opt.step()
    W = [m.weight.detach().cpu().numpy() for m in field.sdf_network if isinstance(m, torch.nn.Linear)]
    ref = H.evaluate(c["cfg"], c["x"], c["table"], W, act)
    out, grad = field.eval_fused(x, gradient=True)
    assert not torch.equal(out, first)
    assert (np.abs(_np(out) - ref["out"]) <= H.tol(ref, "out")).all()
    assert (np.abs(_np(grad) - ref["grad"]) <= H.tol(ref, "grad"))[~ref["near"]].all()
    assert list(field.state_dict().keys()) == keys


def test_refusals():
    c, ref, field, x = _setup("check_mixed", (64, 2), 3, "ReLU")
    with pytest.raises(_lib.IronError, match="CUDA"):
        field.eval_fused(x.cpu())
    with pytest.raises(_lib.IronError, match="float32"):
        field.eval_fused(x.half())
    with pytest.raises(_lib.IronError, match="3 coordinates"):
        field.eval_fused(x[:, :2].contiguous())
    odd = make_field(c["cfg"], (48, 2), "ReLU", 1)
    assert field.fused_supported() and not odd.fused_supported()
    with pytest.raises(_lib.IronError, match="n_neurons"):
        odd.eval_fused(x)
    with torch.no_grad():
        assert odd.sdf(x).shape == (x.shape[0], 1)                               # the plain path still serves it


def test_fused_callable_traces_the_fitted_sphere(tmp_path):
    from iron_amd import scenes
    from iron_amd.raytracer import Camera, RayTracer, intersect_sphere
    from test_gpu_hashgrid_fit import fit, make_field as make_fit_field
    field = make_fit_field(tmp_path / "fit.json").cuda()

    def f(p):
        sdf, _, g = field.get_all(p, is_training=True)
        return sdf, g

    fit(list(field.parameters()), f, torch.device("cuda"), steps=30)
    K, W2C = scenes.fixture_camera_matrices(32, 32)
    cam = Camera(32, 32, K.cuda(), W2C.cuda())
    o, d, _ = cam.get_rays(cam.get_uv())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(o, d, 1.0)
    tr = RayTracer()
    sdf = field.as_callable(0.5, 0.5)
    got = tr(sdf, o, d, near, far, hit)
    again = tr(sdf, o, d, near, far, hit)
    torch.cuda.synchronize()
    conv = got["convergent_mask"]
    print("   fitted sphere through the fused callable: %d of %d rays converge" % (int(conv.sum()), conv.numel()))
    assert int(conv.sum()) > 0
    at = field.eval_fused(got["points"][conv], scale=0.5, offset=0.5)[:, 0]
    assert torch.equal(at, got["sdf"][conv].reshape(-1))
    for k in got:
        if torch.is_tensor(got[k]):
            assert torch.equal(got[k], again[k]), k
