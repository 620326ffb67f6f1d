"""Networks off the geometric init, and the network shapes the kernels accept, as data shared by tests/test_net_shapes_oracle.py,
tests/test_gpu_net_shapes.py and tests/golden/make_golden_shapes.py.

The geometric init (iron_amd/fields.py: SDFNetwork) zeroes every hidden bias of the SDF net and the skip layer's sin/cos
columns, and sets weight_g = |v| row by row; the scenes only perturb lin0's PE columns.  generalise() moves every parameter
off those values, so that a kernel which dropped or misplaced one of them computes a different function.  It works on the
product's modules and on the reference's alike (same parameter names), so both sides end with bit-identical parameters.
"""
from __future__ import annotations

import numpy as np
import torch

# sigma of the weight noise / bias draws.  The SDF's are small enough that the perturbed sphere keeps a zero level set (the
# trace tests assert a minimum hit fraction); the material and NeRF nets have no such constraint.
SDF_SIGMA, SDF_SIGMA_B = 0.01, 0.01
NET_SIGMA, NET_SIGMA_B = 0.02, 0.05


def _kind(net) -> str:
    if hasattr(net, "pts_linears"):
        return "nerf"
    if hasattr(net, "embed_fn_fine"):
        return "sdf"
    return "render"


@torch.no_grad()
def generalise(net, seed: int, sigma: float = None, sigma_b: float = None):
    """In place, deterministically: weight (weight_v) += N(0, sigma) -- every column, the PE columns of layer 0 and of the skip
    layer included; bias += N(0, sigma_b) (so every zero-initialised bias becomes a draw, the SDF's output bias stays near
    its -0.5); weight_g *= exp(U(-1/2, 1/2)), so that g != |v| and the weight-norm fold matters.  Returns `net`."""
    sdf = _kind(net) == "sdf"
    sigma = (SDF_SIGMA if sdf else NET_SIGMA) if sigma is None else sigma
    sigma_b = (SDF_SIGMA_B if sdf else NET_SIGMA_B) if sigma_b is None else sigma_b
    gen = torch.Generator().manual_seed(seed)
    params = dict(net.named_parameters())
    for name in sorted(params):
        p = params[name]
        if name.endswith("weight_g"):
            p.mul_(torch.exp(torch.rand(p.shape, generator=gen) - 0.5).to(p.dtype))
        elif name.endswith("weight_v") or name.endswith("weight"):
            p.add_((sigma * torch.randn(p.shape, generator=gen)).to(p.dtype))
        elif name.endswith("bias"):
            p.add_((sigma_b * torch.randn(p.shape, generator=gen)).to(p.dtype))
        else:
            raise KeyError(name)
    if sdf:
        _recentre(net)
    return net


@torch.no_grad()
def _recentre(net) -> None:
    """Shift the SDF's output bias so that the median distance on the init's sphere (radius 0.5 in scaled coordinates) is 0
    again: the convex softplus turns zero-mean bias noise and rescaled rows into a positive offset that grows with depth and
    would otherwise leave no surface.  fp64, through the oracle, from the parameters alone (identical on both sides)."""
    from oracle import iron_ref as R
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    n_lin = net.num_layers - 1
    spec = R.SDFSpec(d_out=getattr(net, "lin%d" % (n_lin - 1)).out_features, n_layers=n_lin - 1, skip_in=tuple(net.skip_in),
                     multires=(net.lin0.in_features - 3) // 6, scale=float(net.scale))
    d = torch.nn.functional.normalize(torch.randn(256, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64), dim=-1)
    med = R.sdf_forward(sd, spec, d * (0.5 / spec.scale))[:, 0].median()
    b = getattr(net, "lin%d" % (n_lin - 1)).bias
    b[0] = b[0] - (med * spec.scale).to(b.dtype)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# constructor keyword arguments (the reference's and the product's constructors take the same ones)
SDF_BASE = dict(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=(4,), multires=6, bias=0.5, scale=1.0, geometric_init=True,
                weight_norm=True)

# shapes iron_net_create accepts and every SDF entry point computes ("prod" is the reference's network, the one S0..S3 use)
SDF_SHAPES = {
    "prod": {},
    "n2": dict(n_layers=2, skip_in=()),
    "n4_skip2": dict(n_layers=4, skip_in=(2,)),
    "n6_skip5": dict(n_layers=6, skip_in=(5,)),
    "n8_noskip": dict(skip_in=()),
    "n8_dout1": dict(d_out=1),
    "n8_nown": dict(weight_norm=False),
    "n8_scale2": dict(scale=2.0),
    "n16_skip8": dict(n_layers=16, skip_in=(8,)),
}
SDF_NO_BACKWARD = ("n8_scale2",)          # iron_amd/autograd.py: the SDF backward supports scale = 1 only
SDF_REFUSED = {                           # iron_net_create refuses these
    "multires4": dict(multires=4),
    "skip1": dict(skip_in=(1,)),
    "skip_at_output": dict(skip_in=(8,)),
}

# (mode, PE) pairs that k_material is instantiated for (iron_amd/csrc/shade.hip: launch_material), at their production shape
RENDER_FAMILIES = {
    "idr_0_4": dict(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=4, multires_view=4, squeeze_out=True),
    "nvd_6": dict(d_feature=256, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=4, multires=6, multires_view=-1,
                  squeeze_out=False, output_bias=0.4, output_scale=0.1),
    "po_6": dict(d_feature=256, mode="points_only", d_in=3, d_out=1, d_hidden=256, n_layers=4, multires=6, multires_view=-1,
                 squeeze_out=False),
    "idr_10_4_skip": dict(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=8, skip_in=(4,), multires=10,
                          multires_view=4, squeeze_out=True),
}


def _render_variants():
    out = {}
    for fam, base in RENDER_FAMILIES.items():
        skip = bool(base.get("skip_in"))
        var = {"prod": {}, "n8": dict(n_layers=8), "n12": dict(n_layers=12), "nown": dict(weight_norm=False),
               "squeeze1p7": dict(squeeze_out=True, squeeze_out_scale=1.7)}
        if not skip:
            var["n1"] = dict(n_layers=1)
        else:
            var["skip1"] = dict(skip_in=(1,))
            var["skip7"] = dict(skip_in=(7,))        # n - 2 for the 8-layer net (9 linear layers)
        for d_out in (1, 2, 3):
            if d_out != base["d_out"]:
                var["dout%d" % d_out] = dict(d_out=d_out)
        for name, kw in var.items():
            if name == "n8" and base["n_layers"] == 8:
                continue
            out["%s/%s" % (fam, name)] = dict(base, **kw)
    return out


RENDER_SHAPES = _render_variants()
RENDER_REFUSED = {
    "no_normal": dict(d_feature=256, mode="no_normal", d_in=6, d_out=3, d_hidden=256, n_layers=4, multires_view=4),
    "idr_6_4": dict(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=4, multires=6, multires_view=4),
    "nvd_0": dict(d_feature=256, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=4, multires_view=-1),
    "nvd_6_view4": dict(d_feature=256, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=4, multires=6, multires_view=4),
    "skip_at_output": dict(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=4, skip_in=(4,), multires=10,
                           multires_view=4),
}

NERF_BASE = dict(D=8, W=256, d_in=4, d_in_view=3, multires=10, multires_view=4, output_ch=4, skips=[4], use_viewdirs=True)
NERF_SHAPES = {
    "prod": {},
    "D2": dict(D=2, skips=[]),
    "D8_noskip": dict(skips=[]),
    "D14_skip12": dict(D=14, skips=[12]),
}
NERF_REFUSED = {"pe6_4": dict(multires=6), "pe10_2": dict(multires_view=2)}


def sdf_kw(name: str) -> dict:
    return dict(SDF_BASE, **(SDF_SHAPES.get(name) or SDF_REFUSED.get(name) or {}))


def nerf_kw(name: str) -> dict:
    return dict(NERF_BASE, **(NERF_SHAPES.get(name) or NERF_REFUSED.get(name) or {}))


def seed_of(name: str) -> int:
    """A stable per-shape seed (construction and generalise())."""
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9000


def build(cls, kw: dict, name: str):
    """cls(**kw) under a per-shape seed, then generalise()d with it."""
    torch.manual_seed(seed_of(name))
    return generalise(cls(**kw), seed_of(name))


# ---- oracle specs ----------------------------------------------------------------------------------------------------------------
def sdf_spec(kw: dict):
    from oracle import iron_ref as R
    return R.SDFSpec(d_in=kw["d_in"], d_out=kw["d_out"], d_hidden=kw["d_hidden"], n_layers=kw["n_layers"], skip_in=tuple(kw["skip_in"]),
                     multires=kw["multires"], scale=float(kw["scale"]))


def render_spec(kw: dict):
    from oracle import iron_ref as R
    keys = ("d_feature", "mode", "d_in", "d_out", "d_hidden", "n_layers", "multires", "multires_view", "squeeze_out",
            "squeeze_out_scale", "output_bias", "output_scale")
    sp = R.RenderSpec(**{k: kw[k] for k in keys if k in kw})
    sp.skip_in = tuple(kw.get("skip_in", ()))
    return sp


def nerf_spec(kw: dict):
    from oracle import neus_ref as N
    return N.NerfSpec(D=kw["D"], W=kw["W"], d_in=kw["d_in"], d_in_view=kw["d_in_view"], multires=kw["multires"],
                      multires_view=kw["multires_view"], skips=tuple(kw["skips"]))


def sd64(module) -> dict:
    """The module's state as fp64 CPU tensors (the oracle's operands)."""
    return {k: v.detach().cpu().double().clone() for k, v in module.state_dict().items()}


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def sdf_inputs(n: int, seed: int, scale: float = 1.0) -> torch.Tensor:
    """Points in the unit ball's bounding box, denser near the zero level set (radius ~0.5 / scale)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * (0.5 + 0.1 * torch.randn(n, 1, generator=g))
    half = n // 2
    x[:half] = d[:half]
    return x / scale if scale != 1.0 else x


def render_inputs(n: int, seed: int):
    """points, normals, view dirs, features (the shapes RenderingNetwork.forward takes)."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g) * 1.2 - 0.6
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    view = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    feat = torch.randn(n, 256, generator=g) * 0.3
    return pts, nrm, view, feat


def nerf_inputs(n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 4, generator=g) * 2 - 1
    views = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return pts, views


def relu_kink_rows(sd, spec, points, normals, view_dirs, feats, eps: float = 1e-6) -> torch.Tensor:
    """Rows of a material-net batch whose forward passes within `eps` (relative to the size of the sum's terms) of a ReLU kink in
    some layer: there fp32 rounding decides which side of the kink a kernel lands on, and the gradient of that whole unit flips.
    Mirrors oracle/iron_ref.py rendering_forward, fp64."""
    from oracle import iron_ref as R
    if spec.multires > 0:
        points = R.positional_encoding(points, spec.multires)
    if spec.multires_view > 0 and spec.mode not in ("no_view_dir", "points_only"):
        view_dirs = R.positional_encoding(view_dirs, spec.multires_view)
    parts = {"idr": [points, view_dirs, normals, feats], "no_view_dir": [points, normals, feats], "points_only": [points, feats]}
    inp = torch.cat(parts[spec.mode], dim=-1)
    h, bad = inp, torch.zeros(inp.shape[0], dtype=torch.bool)
    for l in range(spec.n_linear - 1):
        w, b = R.effective_weight(sd, l)
        if l in spec.skip_in:
            h = torch.cat([h, inp], dim=-1) / np.sqrt(2)
        z = torch.nn.functional.linear(h, w, b)
        bad |= (z.abs() < eps * (h.abs() @ w.abs().T + b.abs())).any(dim=1)
        h = torch.relu(z)
    return bad


# ---- comparison --------------------------------------------------------------------------------------------------------------
def rel(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def row_rel(a, b) -> float:
    """Worst row: max_i |a_i - b_i| / rms_i |b_i| -- a bad tile of rows cannot hide in an L2 norm over the whole batch."""
    a = np.asarray(a, dtype=np.float64).reshape(len(b), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    rms = np.sqrt(np.mean(np.sum(b * b, axis=1)))
    return float(np.max(np.linalg.norm(a - b, axis=1)) / max(rms, 1e-30))


_rel = rel


def _compare_param_grads(module, leaf_sd, tol, tag, tol_for=None):
    """tol_for: {parameter-name prefix: tolerance} overrides for individual tensors (every other tensor is held to `tol`)."""
    worst = 0.0
    base_tol = tol
    for name, p in module.named_parameters():
        tol = base_tol
        for prefix, t_ in (tol_for or {}).items():
            if name.startswith(prefix):
                tol = t_
        assert p.grad is not None, name
        ref = leaf_sd[name].grad
        if ref is None:  # torch found no path to this parameter (e.g. the last bias from a gradient-only loss): ours must be 0
            assert float(p.grad.abs().max()) == 0.0, (tag, name)
            p.grad = None
            continue
        r = _rel(p.grad.cpu().numpy(), ref.numpy())
        if name.endswith("weight_g") and r > tol:
            # d/dg_i = <dW_i, v_i/|v_i|> is a projection of the effective-weight gradient dW (what the GEMMs produce) that can cancel
            # by orders of magnitude (lin0 of the PE-10 colour net: |d/dg| ~ 1e-3 |dW_i|), so its own norm is the wrong yardstick:
            # the split-fp16 GEMM carries 2^-22 per operand, relative to dW.  |dW_i| = |d/dv_i| |v_i| / g_i up to that projection.
            v = dict(module.named_parameters())[name.replace("weight_g", "weight_v")].detach().cpu()
            gv = leaf_sd[name.replace("weight_g", "weight_v")].grad
            dw_rows = gv.norm(dim=1, keepdim=True) * v.norm(dim=1, keepdim=True) / dict(module.named_parameters())[name].detach().cpu().abs()
            r = float(((p.grad.cpu() - ref).abs() / dw_rows.clamp_min(1e-30)).max())
        # a parameter whose gradient is pure rounding noise (e.g. zero-initialised PE columns' norm direction) is compared in
        # absolute terms against the largest gradient of the network
        if r > worst:
            worst = r
            _compare_param_grads.last = "%s |ref| %.2e" % (name, float(ref.norm()))
        assert r <= tol or float(ref.abs().max()) <= 1e-9, (tag, name, r)
        p.grad = None
    return worst
