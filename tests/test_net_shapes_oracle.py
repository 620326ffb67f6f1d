"""CPU half of the network-shape matrix (tests/_nets.py): no GPU.

- G19 pins the fp64 oracle (oracle/iron_ref.py, neus_ref.py) to the reference's own modules at every shape that computes, with
  generalise()d parameters (tests/golden/make_golden_shapes.py), and the product's constructors + generalise() to the same state.
- Sensitivity guards: on the GPU tests' own inputs, putting any weight group the geometric init zeroes (or ties) back to its init
  value -- or swapping sin and cos at the skip layer -- moves the oracle's output by >= 50x the tolerance
  tests/test_gpu_net_shapes.py applies to it.  So those tests cannot pass a kernel that drops or misplaces such a group.
- The Python-side refusals that need no device.
"""
import numpy as np
import pytest
import torch

from iron_amd import _lib
from iron_amd.fields import NeRF, RenderingNetwork, SDFNetwork
from oracle import iron_ref as R
from oracle import neus_ref as NR

import _nets as N
from _util import golden, state_hash

TOL_SDF, TOL_GRAD = 1e-5, 2e-5       # tests/test_gpu_net_shapes.py: SDF values / get_all gradients
MARGIN = 50.0


def _key(*parts):
    return "__".join(p.replace("/", ".") for p in parts)


@pytest.fixture(scope="module")
def g19():
    return golden("g19_shapes.npz")


@pytest.mark.parametrize("name", list(N.SDF_SHAPES))
def test_g19_sdf_oracle(g19, name):
    kw = N.sdf_kw(name)
    net = N.build(SDFNetwork, kw, name)
    assert state_hash({"sdf_network": net}) == str(g19[_key("hash", "sdf", name)])
    x = torch.from_numpy(g19[_key("sdf", name, "x")])
    sd, spec = N.sd64(net), N.sdf_spec(kw)
    cols = [c for c in (0, 1, 2, 128, 256) if c < kw["d_out"]]
    out = R.sdf_forward(sd, spec, x)[:, cols].numpy()
    _, _, grad = R.sdf_get_all(sd, spec, x)
    assert N.rel(out, g19[_key("sdf", name, "out")]) <= 1e-12
    assert N.rel(grad.numpy(), g19[_key("sdf", name, "grad")]) <= 1e-12


@pytest.mark.parametrize("name", list(N.RENDER_SHAPES))
def test_g19_render_oracle(g19, name):
    kw = N.RENDER_SHAPES[name]
    net = N.build(RenderingNetwork, kw, name)
    assert state_hash({"net": net}) == str(g19[_key("hash", "render", name)])
    pts, nrm, view, feat = (v.double() for v in N.render_inputs(24, N.seed_of(name) + 2))
    use_view = kw["mode"] in ("idr", "no_normal")
    out = R.rendering_forward(N.sd64(net), N.render_spec(kw), pts, nrm, view if use_view else None, feat).numpy()
    assert N.rel(out, g19[_key("render", name, "out")]) <= 1e-12


@pytest.mark.parametrize("name", list(N.NERF_SHAPES))
def test_g19_nerf_oracle(g19, name):
    kw = N.nerf_kw(name)
    net = N.build(NeRF, kw, name)
    assert state_hash({"net": net}) == str(g19[_key("hash", "nerf", name)])
    pts, views = (v.double() for v in N.nerf_inputs(24, N.seed_of(name) + 2))
    alpha, rgb = NR.nerf_forward(N.sd64(net), N.nerf_spec(kw), pts, views)
    assert N.rel(alpha.numpy(), g19[_key("nerf", name, "alpha")]) <= 1e-12
    assert N.rel(rgb.numpy(), g19[_key("nerf", name, "rgb")]) <= 1e-12


# ---- sensitivity guards ---------------------------------------------------------------------------------------------------------
def _folded(sd, n_lin):
    """lin{l}.weight_g / weight_v -> lin{l}.weight (the effective weight), so that groups of columns can be reset in place."""
    out = {}
    for l in range(n_lin):
        w, b = R.effective_weight(sd, l)
        out["lin%d.weight" % l], out["lin%d.bias" % l] = w.clone(), b.clone()
    return out


def _skip_pe_cols(sd, skip, pe=39):
    """Columns of the skip layer's sin and cos inputs (PE layout: x, then sin(2^k x), cos(2^k x) per level k)."""
    off = sd["lin%d.weight" % skip].shape[1] - pe
    sin = [off + 3 + 6 * k + i for k in range(6) for i in range(3)]
    cos = [c + 3 for c in sin]
    return sin, cos


def _variants(name, sd, kw):
    n_lin = kw["n_layers"] + 1
    flat = _folded(sd, n_lin)
    v = {}
    d = dict(flat)
    for l in range(1, n_lin - 1):
        d["lin%d.bias" % l] = torch.zeros_like(d["lin%d.bias" % l])
    v["hidden biases 1..n-2 = 0"] = d
    d = dict(flat)
    d["lin0.bias"] = torch.zeros_like(d["lin0.bias"])
    v["lin0.bias = 0"] = d
    if kw["weight_norm"]:
        d = dict(sd)
        for l in range(n_lin):
            d["lin%d.weight_g" % l] = sd["lin%d.weight_v" % l].norm(dim=1, keepdim=True)
        v["weight_g = |v|"] = d
    if kw["skip_in"]:
        skip = kw["skip_in"][0]
        sin, cos = _skip_pe_cols(flat, skip)
        for what, cols in (("sin", sin), ("cos", cos)):
            d = dict(flat)
            w = d["lin%d.weight" % skip].clone()
            w[:, cols] = 0
            d["lin%d.weight" % skip] = w
            v["skip %s columns = 0" % what] = d
        d = dict(flat)
        w = d["lin%d.weight" % skip].clone()
        w[:, sin], w[:, cos] = flat["lin%d.weight" % skip][:, cos], flat["lin%d.weight" % skip][:, sin]
        d["lin%d.weight" % skip] = w
        v["skip sin <-> cos"] = d
    return v


@pytest.mark.parametrize("name", ["prod", "n4_skip2", "n16_skip8", "n8_nown"])
def test_sdf_init_groups_matter(name):
    """Each weight group the geometric init zeroes or ties, put back, must move the sdf AND its gradient (on the inputs the GPU
    test uses) by >= 50x the GPU test's tolerance: the GPU parity tests would see a kernel that loses it."""
    kw = N.sdf_kw(name)
    net = N.build(SDFNetwork, kw, name)
    sd, spec = N.sd64(net), N.sdf_spec(kw)
    x = N.sdf_inputs(4099, N.seed_of(name) + 1, kw["scale"]).double()   # tests/test_gpu_net_shapes.py: _sdf_case
    y0, _, g0 = R.sdf_get_all(sd, spec, x)
    for what, sd2 in _variants(name, sd, kw).items():
        y, _, g = R.sdf_get_all(sd2, spec, x)
        ry, rg = N.rel(y.numpy(), y0.numpy()), N.rel(g.numpy(), g0.numpy())
        print("%-10s %-26s sdf moves %.2e  gradient moves %.2e" % (name, what, ry, rg))
        assert ry >= MARGIN * TOL_SDF, (name, what, ry)
        assert rg >= MARGIN * TOL_GRAD, (name, what, rg)


# ---- refusals without a device --------------------------------------------------------------------------------------------------
def test_python_side_refusals():
    with pytest.raises(_lib.IronError):
        SDFNetwork(d_in=4, d_out=257, d_hidden=256, n_layers=8, skip_in=[4], multires=6)._desc()
    with pytest.raises(_lib.IronError):
        SDFNetwork(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=[2, 4], multires=6)._desc()
    with pytest.raises(_lib.IronError):
        RenderingNetwork(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=8, skip_in=[2, 4], multires=10,
                         multires_view=4)._desc()
    for name in N.SDF_SHAPES:   # every listed shape describes itself without complaint (the device decides the rest)
        torch.manual_seed(0)
        SDFNetwork(**N.sdf_kw(name))._desc()
    for kw in N.RENDER_SHAPES.values():
        RenderingNetwork(**kw)._desc()
    for name in N.NERF_SHAPES:
        NeRF(**N.nerf_kw(name))._desc()


def test_generalise_is_deterministic_and_moves_every_parameter():
    kw = N.sdf_kw("prod")
    a, b = N.build(SDFNetwork, kw, "prod"), N.build(SDFNetwork, kw, "prod")
    torch.manual_seed(N.seed_of("prod"))
    init = SDFNetwork(**kw)
    for (k, p), q, r in zip(a.named_parameters(), b.parameters(), init.parameters()):
        assert torch.equal(p, q), k
        assert not torch.equal(p, r), k
    a.requires_grad_(False)
    for l in range(1, 8):
        assert float(getattr(a, "lin%d" % l).bias.abs().min()) > 0
        v, g = getattr(a, "lin%d" % l).weight_v, getattr(a, "lin%d" % l).weight_g
        assert float((g[:, 0] / v.norm(dim=1) - 1).abs().max()) > 0.1
    sin, cos = _skip_pe_cols({"lin4.weight": a.lin4.weight_v}, 4)
    assert float(a.lin4.weight_v[:, sin + cos].abs().min()) > 0
