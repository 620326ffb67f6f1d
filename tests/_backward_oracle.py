"""Per-point fp64 oracle of the three layer-wise backward passes (iron_sdf_backward, iron_render_backward, iron_nerf_backward), and
the embedded batches tests/test_gpu_backward_rows.py runs them on.  Shared with tests/test_backward_oracle.py (CPU).

Embedding: every backward is linear in its upstream gradient, so a batch of n rows whose upstream is exactly zero outside a small
live set S must produce the oracle's gradient of the rows of S alone -- one row's error is then not diluted by the n - |S| others,
and the oracle costs |S| rows however large n is.  Row i of a batch takes row i % POOL of a fixed pool of inputs and upstream
gradients, so a live position names its operands whatever n is.

Floors (DESIGN 24's fp32-floor rule): F = the SAME oracle evaluated in fp32 against its fp64 evaluation on the same live rows, per
parameter tensor (L2 over the tensor) and per row for input gradients.  A result passes when its error is within
max(MARGIN x F, TOL_PARAM x |reference|): margin 4 over the floor, and never tighter than the bound the whole-batch tests already
apply (tests/test_gpu_net_shapes.py: TOL_PARAM) -- a handful of rows does not sample the spread of fp32 roundings, so F alone can
come out far below what fp32 arithmetic guarantees.  weight_g keeps the yardstick of _nets._compare_param_grads.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import iron_ref as R
from oracle import neus_ref as NR
from oracle import train_ref as T

import _nets as N

TOL_PARAM = 2e-5      # tests/test_gpu_net_shapes.py
MARGIN = 4.0
POOL = 2048           # distinct input / upstream rows
KINK_CAP = 0.02       # share of a live set that may be left out as ReLU-kink rows
SDF_CHUNK, RENDER_CHUNK = 65536, 131072   # csrc/train.hip: kSdfChunk, kRenderChunk / kNerfChunk

# the smallest sizes at which each route is taken (gemm_rm's gate is 256 ROWS: 128 points with tangent rows, 256 without)
SDF_TANGENT_SIZES = (1, 127, 128, 129, 161)
SDF_PLAIN_SIZES = (255, 256, 257, 321)
NET_SIZES = (1, 255, 256, 257, 321)
SDF_CHUNK_EXTRA = (0, 1, 128, 129)
RENDER_CHUNK_EXTRA = (1, 257)
SDF_TANGENT_PARTS, SDF_PLAIN_PARTS = ("g", "sfg", "e"), ("s", "f", "sf")

SDF_NETS = ("prod", "n2", "n4_skip2", "n8_dout1", "n8_nown", "alt")
RENDER_NETS = ("idr_0_4/prod", "nvd_6/prod", "po_6/prod", "idr_10_4_skip/prod", "alt")
ALT_WIDTHS = (256, 128, 256, 320, 256)    # hidden widths of the "alt" nets: fused (5..8 column tiles) and unfused layers alternate


@dataclass
class Net:
    kind: str                       # "sdf" | "render" | "nerf"
    name: str
    sd: Dict[str, torch.Tensor]     # fp32 CPU state dict (the oracle's names)
    spec: object
    layers: List[Tuple[str, bool]]  # (state-dict prefix, weight-normed) in the C entry's layer order
    meta: dict = field(default_factory=dict)
    seed: int = 0

    def param_names(self):
        out = []
        for p, wn in self.layers:
            out += [p + ".weight_g", p + ".weight_v", p + ".bias"] if wn else [p + ".weight", p + ".bias"]
        return out


def _lin_layers(sd, n):
    return [("lin%d" % l, ("lin%d.weight_v" % l) in sd) for l in range(n)]


def _alt_state(kind: str, seed: int):
    """A weight-normed net whose hidden widths are ALT_WIDTHS, built without a module (iron_net_create serves 256-wide nets only;
    the C backward entries take any layer table).  Softplus net: pre-activations of spread ~0.1, so that sigma'' is alive; ReLU
    net: He init, skip layer 2."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    if kind == "sdf":
        d0, outs, skip = 39, list(ALT_WIDTHS) + [257], None
    else:
        d0, outs, skip = 3 + 27 + 3 + 256, list(ALT_WIDTHS) + [3], 2
    prev = d0
    for l, out in enumerate(outs):
        fan = prev + (d0 if l == skip else 0)
        if kind == "sdf":
            s = 0.1 / math.sqrt(fan * (0.5 if l == 0 else 0.02))   # inputs of rms ~0.7 (PE) / ~0.14 (softplus of N(0, 0.1))
        else:
            s = math.sqrt(2.0 / fan)
        v = torch.randn(out, fan, generator=g) * s
        sd["lin%d.weight_v" % l] = v
        sd["lin%d.weight_g" % l] = (v.norm(dim=1, keepdim=True) * torch.exp(torch.rand(out, 1, generator=g) - 0.5))
        sd["lin%d.bias" % l] = torch.randn(out, generator=g) * (0.03 if kind == "sdf" else 0.05)
        prev = out
    return sd, len(outs), skip


_nets: Dict[Tuple[str, str], Net] = {}


def net_of(kind: str, name: str) -> Net:
    if (kind, name) in _nets:
        return _nets[(kind, name)]
    seed = N.seed_of(kind + name)
    if kind == "sdf" and name == "alt":
        sd, nl, _ = _alt_state("sdf", seed)
        spec = R.SDFSpec(d_out=257, n_layers=nl - 1, skip_in=(), multires=6)
        net = Net("sdf", name, sd, spec, _lin_layers(sd, nl), dict(multires=6, skip=-1, d_out=257), seed)
    elif kind == "render" and name == "alt":
        sd, nl, skip = _alt_state("render", seed)
        spec = R.RenderSpec(d_feature=256, mode="idr", d_out=3, n_layers=nl - 1, multires=0, multires_view=4, squeeze_out=True)
        spec.skip_in = (skip,)
        net = Net("render", name, sd, spec, _lin_layers(sd, nl), dict(skip=skip), seed)
    elif kind == "sdf":
        from iron_amd.fields import SDFNetwork
        kw = N.sdf_kw(name)
        sd = {k: v.detach().clone() for k, v in N.build(SDFNetwork, kw, name).state_dict().items()}
        spec = N.sdf_spec(kw)
        net = Net("sdf", name, sd, spec, _lin_layers(sd, spec.n_linear),
                  dict(multires=kw["multires"], skip=kw["skip_in"][0] if kw["skip_in"] else -1, d_out=kw["d_out"]), seed)
    elif kind == "render":
        from iron_amd.fields import RenderingNetwork
        kw = N.RENDER_SHAPES[name]
        sd = {k: v.detach().clone() for k, v in N.build(RenderingNetwork, kw, name).state_dict().items()}
        spec = N.render_spec(kw)
        net = Net("render", name, sd, spec, _lin_layers(sd, spec.n_linear), dict(skip=spec.skip_in[0] if spec.skip_in else -1), seed)
    else:
        from iron_amd.fields import NeRF
        kw = N.nerf_kw(name)
        sd = {k: v.detach().clone() for k, v in N.build(NeRF, kw, name).state_dict().items()}
        spec = N.nerf_spec(kw)
        layers = [("pts_linears.%d" % i, False) for i in range(spec.D)] + [("alpha_linear", False), ("feature_linear", False),
                                                                          ("views_linears.0", False), ("rgb_linear", False)]
        net = Net("nerf", name, sd, spec, layers, dict(skip=spec.skips[0] if spec.skips else -1), seed)
    _nets[(kind, name)] = net
    return net


# ---- the pool: inputs and upstream gradients, POOL rows each --------------------------------------------------------------------
_pools = {}


def pool_of(net: Net):
    """(inputs, upstream): tuples / dict of fp32 CPU tensors with POOL rows."""
    key = (net.kind, net.name)
    if key in _pools:
        return _pools[key]
    g = torch.Generator().manual_seed(net.seed + 7)
    if net.kind == "sdf":
        ins = (N.sdf_inputs(POOL, net.seed + 1),)
        up = {"s": torch.randn(POOL, 1, generator=g), "f": torch.randn(POOL, net.meta["d_out"] - 1, generator=g) * 0.1,
              "g": torch.randn(POOL, 3, generator=g)}
    elif net.kind == "render":
        ins = N.render_inputs(POOL, net.seed + 1)
        up = {"o": torch.randn(POOL, net.spec.d_out, generator=g)}
    else:
        ins = N.nerf_inputs(POOL, net.seed + 1)
        up = {"a": torch.randn(POOL, 1, generator=g), "r": torch.randn(POOL, 3, generator=g)}
    _pools[key] = (ins, up)
    return _pools[key]


def nerf_kink_rows(sd, spec, pts, views, eps: float = 1e-6) -> torch.Tensor:
    """relu_kink_rows for the NeRF (mirrors oracle/neus_ref.py nerf_forward, fp64)."""
    x = R.positional_encoding(pts, spec.multires) if spec.multires > 0 else pts
    v = R.positional_encoding(views, spec.multires_view) if spec.multires_view > 0 else views
    bad = torch.zeros(x.shape[0], dtype=torch.bool)

    def lin(h, key):
        w, b = sd[key + ".weight"], sd[key + ".bias"]
        z = F.linear(h, w, b)
        return z, (z.abs() < eps * (h.abs() @ w.abs().T + b.abs())).any(dim=1)

    h = x
    for i in range(spec.D):
        z, k = lin(h, "pts_linears.%d" % i)
        bad |= k
        h = torch.relu(z)
        if i in spec.skips:
            h = torch.cat([x, h], -1)
    feat = F.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
    _, k = lin(torch.cat([feat, v], -1), "views_linears.0")
    return bad | k


_kinks = {}


def kink_pool(net: Net) -> torch.Tensor:
    """[POOL] bool: pool rows with an fp64 pre-activation within relu_kink_rows' eps of 0 (all False for the softplus net)."""
    key = (net.kind, net.name)
    if key not in _kinks:
        ins, _ = pool_of(net)
        sd = {k: v.double() for k, v in net.sd.items()}
        if net.kind == "sdf":
            _kinks[key] = torch.zeros(POOL, dtype=torch.bool)
        elif net.kind == "render":
            use_view = net.spec.mode in ("idr", "no_normal")
            _kinks[key] = N.relu_kink_rows(sd, net.spec, ins[0].double(), ins[1].double(), ins[2].double() if use_view else None, ins[3].double())
        else:
            _kinks[key] = nerf_kink_rows(sd, net.spec, ins[0].double(), ins[1].double())
    return _kinks[key]


# ---- live sets --------------------------------------------------------------------------------------------------------------------
def live_set(n: int, block: int, chunk: Optional[int] = None) -> List[int]:
    """At most 8 rows: 0, n - 1, 31, 32, the first and last row of the last partial block (`block` rows: 32 points when the rows are
    paired with tangent rows, 64 otherwise), the last row of chunk 0 and the first of chunk 1."""
    cand = [0, n - 1, 31, 32]
    if n % block:
        cand += [(n - 1) // block * block, n - 1]
    if chunk is not None:
        cand += [chunk - 1, chunk]
        if (n - chunk) % block:
            cand += [chunk + (n - chunk - 1) // block * block]
    out = []
    for r in cand:
        if 0 <= r < n and r not in out:
            out.append(r)
    assert len(out) <= 8, out
    return out


def drop_kinks(net: Net, live: Sequence[int]) -> Tuple[List[int], int]:
    kp = kink_pool(net)
    keep = [r for r in live if not bool(kp[r % POOL])]
    return keep, len(live) - len(keep)


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def eikonal_cotangent(net: Net, rows: Sequence[int]) -> torch.Tensor:
    """d/dg of sum (|g| - 1)^2 at the fp64 oracle's gradient of the given pool rows, rounded to fp32: the eikonal loss as a fixed
    cotangent, so that the device and the oracle are handed the same upstream."""
    ins, _ = pool_of(net)
    x = ins[0][[r % POOL for r in rows]].double()
    _, _, g = R.sdf_get_all({k: v.double() for k, v in net.sd.items()}, net.spec, x)
    nrm = g.norm(dim=-1, keepdim=True)
    return (2 * (nrm - 1) * g / nrm).float()


def embed(net: Net, n: int, live: Sequence[int], parts: str):
    """The batch of n rows: inputs (tuple of [n, .] fp32), upstream (dict part -> [n, .] fp32 or None), exactly zero off `live`.
    parts: SDF any of "s", "f", "g" or "e" (the eikonal cotangent in the gradient slot); render "o"; NeRF any of "a", "r"."""
    ins, up = pool_of(net)
    idx = torch.arange(n) % POOL
    batch_in = tuple(t[idx].contiguous() for t in ins)
    lv = torch.tensor(list(live), dtype=torch.long)
    out = {}
    for key in ("s", "f", "g") if net.kind == "sdf" else (("o",) if net.kind == "render" else ("a", "r")):
        src = key if key in parts else ("e" if key == "g" and "e" in parts else None)
        if src is None or (key == "f" and net.meta["d_out"] == 1):
            out[key] = None
            continue
        u = torch.zeros((n, up[key].shape[1]))
        u[lv] = eikonal_cotangent(net, live) if src == "e" else up[key][lv % POOL]
        out[key] = u
    return batch_in, out


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def oracle(net: Net, batch_in, upstream, live: Sequence[int], dtype=torch.float64):
    """Gradients of sum_{i in live} <upstream_i, output_i> in `dtype`, evaluated on the live rows alone:
    ({parameter name: gradient or None}, [per-row input gradients [|live|, .] or None, in input order])."""
    lv = list(live)
    sd = T.leaf_state({k: v.to(dtype) for k, v in net.sd.items()})
    ins = [t[lv].to(dtype) for t in batch_in]
    up = {k: (None if v is None else v[lv].to(dtype)) for k, v in upstream.items()}
    in_grads = []
    if net.kind == "sdf":
        y, f, g = T.sdf_get_all_train(sd, net.spec, ins[0])
        loss = 0
        if up["s"] is not None:
            loss = loss + (y * up["s"]).sum()
        if up["f"] is not None:
            loss = loss + (f * up["f"]).sum()
        if up["g"] is not None:
            loss = loss + (g * up["g"]).sum()
    elif net.kind == "render":
        leaves = [t.requires_grad_(True) for t in ins]
        use_view = net.spec.mode in ("idr", "no_normal")
        out = R.rendering_forward(sd, net.spec, leaves[0], leaves[1], leaves[2] if use_view else None, leaves[3])
        loss = (out * up["o"]).sum()
    else:
        a, r = NR.nerf_forward(sd, net.spec, ins[0], ins[1])
        loss = 0
        if up["a"] is not None:
            loss = loss + (a * up["a"]).sum()
        if up["r"] is not None:
            loss = loss + (r * up["r"]).sum()
    loss.backward()
    if net.kind == "render":
        in_grads = [None if t.grad is None else t.grad.detach() for t in leaves]
    return {k: (None if sd[k].grad is None else sd[k].grad.detach()) for k in net.param_names()}, in_grads


def oracle_per_point(net: Net, batch_in, upstream, live, dtype=torch.float64):
    """The per-point contributions: oracle() of each live row on its own."""
    return [oracle(net, batch_in, upstream, [r], dtype) for r in live]


@dataclass
class Expect:
    ref: Dict[str, Optional[torch.Tensor]]
    floor: Dict[str, float]
    in_ref: list
    in_floor: list          # per input: [|live|] per-row floors, or None
    f32: Dict[str, Optional[torch.Tensor]]

    def bound(self, name: str) -> float:
        return max(MARGIN * self.floor[name], TOL_PARAM * float(self.ref[name].norm()))


def expect(net: Net, batch_in, upstream, live) -> Expect:
    r64, i64 = oracle(net, batch_in, upstream, live, torch.float64)
    r32, i32 = oracle(net, batch_in, upstream, live, torch.float32)
    floor = {k: (0.0 if v is None else float((r32[k].double() - v).norm())) for k, v in r64.items()}
    in_floor = [None if v is None else (i32[j].double() - v).norm(dim=1) for j, v in enumerate(i64)]
    return Expect(r64, floor, i64, in_floor, r32)


def _dw_rows(net: Net, name: str, ex: Expect) -> torch.Tensor:
    """|dW_i| per output row for a weight_g tensor (the yardstick of _nets._compare_param_grads)."""
    vn = name.replace("weight_g", "weight_v")
    v, g = net.sd[vn].double(), net.sd[name].double()
    return (ex.ref[vn].norm(dim=1, keepdim=True) * v.norm(dim=1, keepdim=True) / g.abs()).clamp_min(1e-300)


def compare_params(net: Net, got: Dict[str, torch.Tensor], ex: Expect, tag) -> Tuple[float, float, str]:
    """Asserts every parameter gradient in `got` within its floor of ex.ref.  Returns (worst error / bound, worst error / F, the
    tensor of that worst error / F)."""
    worst, worst_f, who = 0.0, 0.0, ""
    for name in net.param_names():
        ref, g = ex.ref[name], got[name].double()
        assert torch.isfinite(g).all(), (tag, name, "non-finite")
        if ref is None:   # no path to this parameter (the last bias under a gradient-only loss): exactly zero
            assert float(g.abs().max()) == 0.0, (tag, name, "expected exactly 0")
            continue
        err, bound = float((g - ref).norm()), ex.bound(name)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if name.endswith("weight_g") and ratio > 1:
            rows = _dw_rows(net, name, ex)
            r_dev = float(((g - ref).abs() / rows).max())
            r_f32 = float(((ex.f32[name].double() - ref).abs() / rows).max())
            ratio = r_dev / max(MARGIN * r_f32, TOL_PARAM)
        worst = max(worst, ratio)
        if ex.floor[name] > 0 and err / ex.floor[name] > worst_f:
            worst_f, who = err / ex.floor[name], "%s (error %.1e of |ref|, F %.1e of |ref|)" % (name, err / float(ref.norm()), ex.floor[name] / float(ref.norm()))
        assert ratio <= 1.0, (tag, name, "error %.3e bound %.3e floor %.3e |ref| %.3e" % (err, bound, ex.floor[name], float(ref.norm())))
    return worst, worst_f, who


def compare_rows(got: torch.Tensor, ref: torch.Tensor, floor: torch.Tensor, live, tag) -> float:
    """Per-row input gradients: every live row within max(MARGIN x its floor, TOL_PARAM x |its reference|), every other row exactly
    zero.  `got` is the whole [n, .] output."""
    g = got.double()
    assert torch.isfinite(g).all(), (tag, "non-finite")
    lv = torch.tensor(list(live), dtype=torch.long)
    dead = torch.ones(g.shape[0], dtype=torch.bool)
    dead[lv] = False
    assert float(g[dead].abs().max()) == 0.0 if bool(dead.any()) else True, (tag, "a dead row is not exactly zero")
    err = (g[lv] - ref).norm(dim=1)
    bound = torch.maximum(MARGIN * floor, TOL_PARAM * ref.norm(dim=1))
    ratio = err / bound.clamp_min(1e-300)
    assert float(ratio.max()) <= 1.0, (tag, "row", int(lv[int(ratio.argmax())]), float(ratio.max()))
    return float(ratio.max())


# ---- activation probe ----------------------------------------------------------------------------------------------------------
PROBE_FUSED_WIDTHS, PROBE_UNFUSED_WIDTHS = (256, 217, 129), (128, 300)
PROBE_X = (1.0, 1.0, 0.0)              # the live point: every first-layer row is (a, -a, c), so <row, x> = 0 EXACTLY and z = bias
PROBE_V = (1.0, -0.5, 0.25)            # the live point's gradient cotangent: zdot = 1.5 a + 0.25 c != 0
PROBE_D_SDF = 0.7


def _f32(v):
    return np.float32(v)


def softplus_strata() -> np.ndarray:
    """Hidden pre-activations z (fp32) whose 100 z are: 0, +-0.5, +-5, +-15, 19.9; the two fp32 neighbours of 20, 25 and 60 (in z:
    nextafter of fp32(t / 100) to both sides); -20, -60; and -87 .. -104, where exp(100 z) and the epilogue's u underflow."""
    z = [_f32(t / 100.0) for t in (0.0, 0.5, -0.5, 5.0, -5.0, 15.0, -15.0, 19.9)]
    for t in (20.0, 25.0, 60.0):
        c = _f32(t / 100.0)
        z += [np.nextafter(c, _f32(-1)), np.nextafter(c, _f32(1))]
    z += [_f32(t / 100.0) for t in (-20.0, -60.0, -87.0, -88.8, -90.0, -95.0, -100.0, -104.0)]
    return np.asarray(z, dtype=np.float32)


def relu_strata() -> Tuple[np.ndarray, np.ndarray]:
    """(z, asserted): +-1e-3 and +-1 are asserted; +-2^-126 (one ulp-scale step from the kink) are excluded as kinks."""
    z = np.asarray([1e-3, -1e-3, 1.0, -1.0], dtype=np.float32)
    return z, np.float32(2.0 ** -126)


def probe_layers(width: int, rot: int, relu: bool):
    """Two plain nn.Linear layers 3 -> width -> 1 whose hidden pre-activation of column j AT THE LIVE POINT is a set value:
    softplus: stratum (j + rot) % 22, so that over rot = 0 .. 21 every column -- every 32-column tile and the ragged last one --
    meets every stratum; relu: the four asserted values in turn, with column j % 64 == 63 (1.3 % .. 1.6 % of the columns, under
    KINK_CAP) at +-2^-126.  Returns (W0 [width, 3], b0, W1 [1, width], b1, z [width], asserted [width] bool), fp32."""
    g = torch.Generator().manual_seed(100 * width + rot + (7 if relu else 0))
    a = torch.randint(16, 65, (width,), generator=g).float() / 64.0          # dyadic: exact in the fp16 high piece
    c = torch.randint(16, 65, (width,), generator=g).float() / 64.0
    sgn = torch.where(torch.rand(width, generator=g) < 0.5, -1.0, 1.0)
    W0 = torch.stack([sgn * a, -sgn * a, sgn * c], dim=1)
    j = np.arange(width)
    if relu:
        zs, tiny = relu_strata()
        z = zs[(j + rot) % len(zs)].copy()
        kink = (j % 64) == 63
        z[kink] = np.where((j[kink] // 64 + rot) % 2 == 0, tiny, -tiny)
        asserted = ~kink
    else:
        zs = softplus_strata()
        z = zs[(j + rot) % len(zs)].copy()
        asserted = np.ones(width, dtype=bool)
    W1 = (torch.randn(1, width, generator=g) * 0.5)
    W1 = torch.where(W1.abs() < 0.05, torch.full_like(W1, 0.05), W1)
    return W0, torch.from_numpy(z.copy()), W1, torch.tensor([0.1]), torch.from_numpy(z.copy()), torch.from_numpy(asserted)


def probe_reference(W0, b0, W1, b1, relu: bool, tangent: bool, dtype):
    """torch autograd on the live point alone: F.softplus(beta = 100) to second order (loss = d_sdf y + <v, dy/dx>), or relu to first
    order (loss = d_out y; also dL/dx).  Returns {"w0", "b0", "w1", "b1"[, "x"]} gradients."""
    p = [t.to(dtype).clone().requires_grad_(True) for t in (W0, b0, W1, b1)]
    x = torch.tensor([PROBE_X], dtype=dtype, requires_grad=True)
    z = F.linear(x, p[0], p[1])
    h = torch.relu(z) if relu else F.softplus(z, beta=100.0)
    y = F.linear(h, p[2], p[3])
    loss = PROBE_D_SDF * y.sum()
    if tangent:
        (gx,) = torch.autograd.grad(y.sum(), x, create_graph=True)
        loss = loss + (gx * torch.tensor([PROBE_V], dtype=dtype)).sum()
    loss.backward()
    out = {"w0": p[0].grad, "b0": p[1].grad, "w1": p[2].grad, "b1": p[3].grad}
    if relu:
        out["x"] = x.grad
    return {k: (torch.zeros_like(q) if v is None else v.detach()) for (k, v), q in zip(out.items(), p + [x])}


def probe_bounds(W0, W1, ref64, ref32, tangent: bool):
    """Per hidden column j: d_bias bound 4 x max(F_j, 2^-22 (|abar_j| + 25 |zdot_j adotbar_j|)), abar = d_sdf W1_j, adotbar = W1_j
    (the tangent output's cotangent is 1), zdot = <W0_j, v>; 2^-22 is the split product's per-operand figure, 25 the peak of
    s2 = 100 s1 (1 - s1).  d_weight row j = zbar_j x + tbar_j v with |x|, |v| <= 1 and tbar = s1 adotbar, |s1| <= 1: the same bound
    plus 2^-22 |adotbar_j| for the tangent row's term."""
    abar = (PROBE_D_SDF * W1[0]).double().abs()
    adot = W1[0].double().abs() if tangent else torch.zeros_like(abar)
    zdot = (W0.double() @ torch.tensor(PROBE_V, dtype=torch.float64)).abs()
    split = 2.0 ** -22 * (abar + 25.0 * zdot * adot)
    fb = (ref32["b0"].double() - ref64["b0"]).abs()
    fw = (ref32["w0"].double() - ref64["w0"]).abs().max(dim=1).values
    return MARGIN * torch.maximum(fb, split), MARGIN * torch.maximum(fw, split + 2.0 ** -22 * adot)


# ---- operand scale ------------------------------------------------------------------------------------------------------------
SCALE_KS = (0, 8, 16, 24, 32, 36)
SCALE_A, SCALE_ROW_A, SCALE_ROW_B, SCALE_COL_A, SCALE_COL_B = 1.0e3, 3, 40, 5, 100
TOL_FWD = 1e-5     # tests/test_gpu_net_shapes.py: TOL_SDF, the accepted error of the recomputed hidden activations


def gemm_scale(amax: float) -> float:
    """gemm_h2.h: gemm_scale_for -- the power of two that brings amax into [2^13, 2^14)."""
    _, e = math.frexp(amax)
    return math.ldexp(1.0, 14 - e)


def scale_bound(h64: torch.Tensor, h32: torch.Tensor, d: float, amax: float) -> torch.Tensor:
    """|dW[c_B, i] - d h_i| allowed for one product d x h_i formed under the scale of `amax` (derivation: the docstring of
    tests/test_gpu_backward_rows.py::test_operand_scale)."""
    s = gemm_scale(amax)
    ah = h64.abs()
    rep_d = max(2.0 ** -22 * s * d, 2.0 ** -36)                       # representation error of s d in (hi, lo)
    rep_h = torch.clamp(2.0 ** -22 * ah, min=2.0 ** -36)             # of h_i (unscaled)
    split = (ah * rep_d + s * d * rep_h) / s + (2.0 ** -22 + 4 * 2.0 ** -24) * d * ah
    fwd = d * torch.clamp(MARGIN * (h32.double() - h64).abs(), min=TOL_FWD * float(ah.max()))
    return split + fwd
