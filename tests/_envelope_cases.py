"""Networks and inputs that probe the numeric envelope of the default (split-fp16, "h2") core row by row, shared by
tests/test_envelope_oracle.py (CPU: the builders' conditions, the yardstick on the reference's own fp32 run) and
tests/test_gpu_envelope_entries.py (GPU: every entry that runs a network on the h2 core), csrc/envelope.hip, DESIGN.md 3.1b.

The probe.  One hidden neuron j of one layer is given a pre-activation z_j that is an ordinary fp32 number on every row and leaves
fp16's range (65 504) on some of them: in layer 0 z_j = G (x_0 - p) with G = 6e4 (the folded weight itself is an fp16 number, so the
h2 stream is built), in a deeper layer an existing row scaled up.  The next layer's column j is set to ordinary random values of
about 1e-6, so that the neuron contributes O(0.1) like any other.  The strata of a row come from the fp64 oracle's z_j:

    quiet   z_j < -0.5               softplus / relu give (about) 0: nothing excuses the h2 core there
    large   1 <= z_j < 65 504        in range; 22 mantissa bits of the activation, fp16's subnormal quantum of the tiny weights
    band    65 504 <= z_j < 65 520   rounds to 65 504: either outcome is allowed
    dirty   z_j >= 65 520            no fp16 split: the row must be loud
    other   -0.5 <= z_j < 1          (a handful of rows at most) held like quiet

The yardstick.  |kernel - fp64| <= 4 x floor + 1e-7 per output block, floor = max |reference fp32 - fp64| over the first 300 rows of
the case's draw.  On the large stratum (and on finite values of band and dirty rows, where the same activation is present) the floor
is max(fp32 floor, split floor), the split floor being the fp64 oracle's own response, row by row, to (i) the probe's downstream
column moved by 2^-22 |w| + 2^-35 and (ii) the probe's activation moved by 2^-22 relative (as a change of G): what 22 bits and the
subnormal quantum can cost, from the oracle alone.  The two responses are added: both errors are present in the same product.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

import _nets

F16_MAX = 65504.0       # largest fp16 number
F16_OVER = 65520.0      # first value that rounds to infinity
G_PROBE = 6.0e4
COL_SCALE = 1.0e-6
POOL = 640              # rows of a case's draw (arrangements pick from them); the floor comes from the first FLOOR_ROWS
FLOOR_ROWS = 300
EPS22 = 2.0 ** -22
Q35 = 2.0 ** -35
CUT_GUARD = 0.05        # no row of a draw lies this close to a stratum cut: 2^-22 * 65 520 = 0.016 is what the h2 split moves z_j by

STRATA = ("quiet", "large", "band", "dirty", "other")


# ---- parameters as the oracle and the product both read them -------------------------------------------------------------------
def _effective(lin) -> torch.Tensor:
    """fp64 folded weight [out, in] of a product layer (weight-normed or plain)."""
    if hasattr(lin, "weight_v"):
        v, g = lin.weight_v.detach().double(), lin.weight_g.detach().double().reshape(-1, 1)
        return g * v / v.norm(dim=1, keepdim=True)
    return lin.weight.detach().double().clone()


@torch.no_grad()
def _set_effective(lin, W: torch.Tensor) -> None:
    """Make W the layer's folded weight: weight_v := W, weight_g := its row norms (plain layer: weight := W)."""
    if hasattr(lin, "weight_v"):
        lin.weight_v.copy_(W.to(lin.weight_v.dtype))
        lin.weight_g.copy_(W.norm(dim=1, keepdim=True).to(lin.weight_g.dtype).reshape(lin.weight_g.shape))
    else:
        lin.weight.copy_(W.to(lin.weight.dtype))


def max_folded_weight(net) -> float:
    m = 0.0
    for mod in net.modules():
        if hasattr(mod, "weight_v") or (isinstance(mod, torch.nn.Linear)):
            m = max(m, float(_effective(mod).abs().max()))
    return m


@torch.no_grad()
def _set_column(lin, j: int, seed: int, zero: bool) -> None:
    """Folded column j of `lin` := N(0, 1) * 1e-6 (or exactly 0); every other column keeps its folded value."""
    W = _effective(lin)
    col = torch.randn(W.shape[0], generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * COL_SCALE
    W[:, j] = 0.0 if zero else col
    _set_effective(lin, W)


@torch.no_grad()
def _set_row(lin, j: int, row: torch.Tensor, bias: float) -> None:
    """Folded row j of `lin` := row (fp64), bias_j := bias; the other rows are not touched."""
    if hasattr(lin, "weight_v"):
        lin.weight_v[j] = row.to(lin.weight_v.dtype)
        lin.weight_g.reshape(-1)[j] = row.norm().to(lin.weight_g.dtype)
    else:
        lin.weight[j] = row.to(lin.weight.dtype)
    lin.bias[j] = bias


# ---- the oracle, per kind: {block: [n, k] tensor of the dtype of its operands} ------------------------------------------------
def _sd(net, dtype):
    return {k: v.detach().cpu().to(dtype).clone() for k, v in net.state_dict().items()}


def oracle_blocks(kind: str, sd: dict, spec, inputs, dtype) -> Dict[str, torch.Tensor]:
    from oracle import iron_ref as R
    from oracle import neus_ref as N
    ins = [None if t is None else t.to(dtype) for t in inputs]
    if kind == "sdf":
        s, f, g = R.sdf_get_all(sd, spec, ins[0])
        return {"sdf": s, "feature": f, "gradient": g}
    if kind == "render":
        return {"out": R.rendering_forward(sd, spec, ins[0], ins[1], ins[2], ins[3])}
    if kind == "nerf":
        a, c = N.nerf_forward(sd, spec, ins[0], ins[1])
        return {"alpha": a, "rgb": c}
    raise ValueError(kind)


def hidden_preact(kind: str, sd: dict, spec, inputs, layer: int) -> torch.Tensor:
    """fp64 pre-activations [n, width] of hidden layer `layer` (sdf / render nets; the oracle's forward up to there)."""
    from oracle import iron_ref as R
    ins = [None if t is None else t.double() for t in inputs]
    if kind == "sdf":
        inp = R.positional_encoding(ins[0] * spec.scale, spec.multires) if spec.multires > 0 else ins[0] * spec.scale
        act = R.softplus100
    elif kind == "render":
        pts = R.positional_encoding(ins[0], spec.multires) if spec.multires > 0 else ins[0]
        view = ins[2]
        if spec.multires_view > 0 and spec.mode not in ("no_view_dir", "points_only"):
            view = R.positional_encoding(view, spec.multires_view)
        parts = {"idr": [pts, view, ins[1], ins[3]], "no_view_dir": [pts, ins[1], ins[3]], "points_only": [pts, ins[3]]}
        inp = torch.cat(parts[spec.mode], dim=-1)
        act = torch.relu
    else:
        raise ValueError(kind)
    h = inp
    for l in range(layer + 1):
        w, b = R.effective_weight(sd, l)
        if l in spec.skip_in:
            h = torch.cat([h, inp], dim=-1) / np.sqrt(2)
        z = torch.nn.functional.linear(h, w, b)
        if l == layer:
            return z
        h = act(z)
    raise AssertionError


# ---- a case ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    kind: str                       # "sdf" | "render" | "nerf"
    net: torch.nn.Module            # the product's module, CPU
    spec: object
    inputs: Tuple                   # CPU fp32 tensors of POOL rows (None where the mode takes none)
    stratum: np.ndarray             # [POOL] of STRATA
    z: np.ndarray                   # [POOL] the oracle's probe pre-activation (nan: the case has no single probe)
    loud: bool                      # R4: dirty rows must come back non-finite (layer-0 probe cases)
    uses: Tuple[str, ...]           # strata the case is built to populate (each >= 5 % of the rows)
    ref64: Dict[str, torch.Tensor] = field(default_factory=dict)
    ref32: Dict[str, torch.Tensor] = field(default_factory=dict)
    floor: Dict[str, float] = field(default_factory=dict)          # over the rows whose inputs are ordinary
    floor_hot: Dict[str, float] = field(default_factory=dict)      # over all rows (sites f, g: inputs of 7e4 / 1e5 on every other row)
    hot: Optional[np.ndarray] = None                               # [POOL] rows with such inputs (None: no such rows)
    stratum_fwd: Optional[np.ndarray] = None                       # [POOL] SDF cases: the strata as a forward-mode kernel sees them
    split: Dict[str, torch.Tensor] = field(default_factory=dict)   # [POOL] per block; zeros where the case has no probe

    def rows(self, which: str) -> np.ndarray:
        return np.nonzero(self.stratum == which)[0]

    def clean_rows(self) -> np.ndarray:
        return np.nonzero((self.stratum == "quiet") | (self.stratum == "large") | (self.stratum == "other"))[0]

    def _floor_rows(self, block: str, idx) -> torch.Tensor:
        fl = torch.full((len(idx),), self.floor[block], dtype=torch.float64)
        if self.hot is not None:
            fl = torch.where(torch.from_numpy(self.hot[idx]), torch.full_like(fl, self.floor_hot[block]), fl)
        return fl

    def bound(self, block: str, idx, stratum=None) -> torch.Tensor:
        """[len(idx), 1] the yardstick of every row: 4 x floor + 1e-7, the floor of a row outside quiet / other being
        max(fp32 floor, its split floor)."""
        idx = np.asarray(idx)
        fl = self._floor_rows(block, idx)
        plain = torch.from_numpy(np.isin((self.stratum if stratum is None else stratum)[idx], ("quiet", "other")))
        sp = torch.where(plain, torch.zeros_like(fl), self.split[block][idx])
        return (4.0 * torch.maximum(fl, sp) + 1e-7).reshape(-1, 1)

    def exact_bound(self, block: str, idx) -> torch.Tensor:
        """R3: the exact-fp32 core is held to the plain yardstick on every row (rows with inputs of 7e4 / 1e5: the floor of those rows)."""
        idx = np.asarray(idx)
        return (4.0 * self._floor_rows(block, idx) + 1e-7).reshape(-1, 1)


def strata_of(z: np.ndarray) -> np.ndarray:
    s = np.full(z.shape, "other", dtype=object)
    s[z < -0.5] = "quiet"
    s[z >= 1.0] = "large"
    s[z >= F16_MAX] = "band"
    s[z >= F16_OVER] = "dirty"
    return s


def near_a_cut(z: np.ndarray) -> int:
    return int(sum((np.abs(z - c) < CUT_GUARD).sum() for c in (-0.5, 1.0, F16_MAX, F16_OVER)))


def _finish(case: Case, perturb: Optional[Callable] = None) -> Case:
    """Oracle runs: fp64, the reference's fp32, and the two perturbed fp64 runs of the split floor."""
    sd64, sd32 = _sd(case.net, torch.float64), _sd(case.net, torch.float32)
    case.ref64 = {k: v.double() for k, v in oracle_blocks(case.kind, sd64, case.spec, case.inputs, torch.float64).items()}
    case.ref32 = {k: v.double() for k, v in oracle_blocks(case.kind, sd32, case.spec, case.inputs, torch.float32).items()}
    for k in case.ref64:
        d = (case.ref32[k] - case.ref64[k]).abs()[:FLOOR_ROWS]
        case.floor_hot[k] = float(d[torch.isfinite(d)].max())
        case.floor[k] = case.floor_hot[k] if case.hot is None else float(d[~torch.from_numpy(case.hot[:FLOOR_ROWS])].max())
        case.split[k] = torch.zeros(POOL, dtype=torch.float64)
    if perturb is not None:
        for which in ("col", "act"):
            sdp = perturb(sd64, which)
            out = oracle_blocks(case.kind, sdp, case.spec, case.inputs, torch.float64)
            for k in case.ref64:
                case.split[k] += (out[k].double() - case.ref64[k]).abs().reshape(POOL, -1).max(dim=1).values
    return case


def _perturb_fn(kind, names_next, j_cols, names_probe, j_rows):
    """sd64 -> a copy with (col) the listed folded columns moved by 2^-22 |w| + 2^-35 away from zero, or (act) the listed rows'
    weight and bias scaled by 1 + 2^-22.  `names_*`: state-dict prefixes ("lin1", "pts_linears.1")."""
    def run(sd, which):
        sd = {k: v.clone() for k, v in sd.items()}
        if which == "col":
            for name, cols in zip(names_next, j_cols):
                if name + ".weight_v" in sd:
                    v, g = sd[name + ".weight_v"], sd[name + ".weight_g"].reshape(-1, 1)
                    W = g * v / v.norm(dim=1, keepdim=True)
                else:
                    W = sd[name + ".weight"].clone()
                c = W[:, cols]
                W[:, cols] = c + torch.sign(c) * (EPS22 * c.abs() + Q35)
                if name + ".weight_v" in sd:
                    sd[name + ".weight_v"] = W
                    sd[name + ".weight_g"] = W.norm(dim=1, keepdim=True).reshape(sd[name + ".weight_g"].shape)
                else:
                    sd[name + ".weight"] = W
        else:
            for name, rows in zip(names_probe, j_rows):
                key = name + (".weight_g" if name + ".weight_g" in sd else ".weight")
                w = sd[key]
                w[rows] = w[rows] * (1.0 + EPS22)
                sd[name + ".bias"][rows] = sd[name + ".bias"][rows] * (1.0 + EPS22)
        return sd
    return run


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _points(seed: int, lo=-0.9, hi=0.9) -> torch.Tensor:
    return torch.rand(POOL, 3, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


def _render_inputs(seed: int):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(POOL, 3, generator=g) * 1.8 - 0.9
    nrm = torch.nn.functional.normalize(torch.randn(POOL, 3, generator=g), dim=-1)
    view = torch.nn.functional.normalize(torch.randn(POOL, 3, generator=g), dim=-1)
    feat = torch.randn(POOL, 256, generator=g) * 0.3
    return pts, nrm, view, feat


# ---- builders: the SDF net (S1's) ------------------------------------------------------------------------------------------------------
def _s1_sdf():
    from iron_amd import scenes
    return scenes.build_networks("S1")["sdf_network"]


def _sdf_spec():
    from oracle import iron_ref as R
    return R.SDFSpec()


@torch.no_grad()
def probe_layer0(net, G: float, p: float, j: int = 5, seed: int = 11, zero_col: bool = False):
    """Neuron j of layer 0 := G (x_0 - p); the next layer's column j := ~1e-6 draws (or 0).  Works on the SDF and material nets
    (weight-normed; the first input column is the raw coordinate x_0)."""
    lin0, lin1 = net.lin0, net.lin1
    row = torch.zeros(lin0.in_features, dtype=torch.float64)
    row[0] = G
    _set_row(lin0, j, row, -G * p)
    _set_column(lin1, j, seed, zero_col)
    return net


@torch.no_grad()
def probe_hidden(net, kind, spec, inputs, layer: int, j: int = 3, seed: int = 12, quiet_q: float = 0.5, dirty_q: float = 0.90):
    """A probe in hidden layer `layer` >= 1 (not the skip layer): row j := c u, u the direction in which the layer's input spreads
    most over the draw (so the folded weights stay small for the spread they buy), shifted so that the rows below the draw's
    `quiet_q` quantile are quiet and those above its `dirty_q` quantile dirty; the next layer's column j := ~1e-6 draws.
    The material nets' hidden activations are ~0.05, which would need folded weights above 65 504 for that spread: their layer
    `layer` - 1 is scaled by 16 first and layer `layer` by 1/16 (relu is homogeneous: the same function, S3's transformation)."""
    if kind == "render":
        prev, cur = getattr(net, "lin%d" % (layer - 1)), getattr(net, "lin%d" % layer)
        _set_effective(prev, _effective(prev) * 16.0)
        prev.bias.mul_(16.0)
        _set_effective(cur, _effective(cur) / 16.0)
    sd = _sd(net, torch.float64)
    act = _nets_act(kind)
    h = act(hidden_preact(kind, sd, spec, inputs, layer - 1))
    lin, nxt = getattr(net, "lin%d" % layer), getattr(net, "lin%d" % (layer + 1))
    assert h.shape[1] == lin.in_features
    mean = h.mean(dim=0)
    u = torch.linalg.svd(h - mean, full_matrices=False).Vh[0]
    proj = (h - mean) @ u
    lo, hi = proj.quantile(quiet_q), proj.quantile(dirty_q)
    c = float(F16_OVER * 1.03 / (hi - lo))
    _set_row(lin, j, u * c, float(-c * (u @ mean + lo)))
    _set_column(nxt, j, seed, False)
    return j


def _nets_act(kind):
    from oracle import iron_ref as R
    return R.softplus100 if kind == "sdf" else torch.relu


def sdf_case(site: str) -> Case:
    """site: a probe (b: zero column, h: G < 0) | c the BLOW_UP net of tests/test_gpu_envelope.py | d probe in front of the skip layer
    | e probe in the last hidden layer | f input coordinates of 7e4 on every other row."""
    net, spec = _s1_sdf(), _sdf_spec()
    x = _points(21)
    loud, uses, perturb, z = False, ("quiet", "large", "dirty"), None, None
    if site in ("a", "b", "h"):
        G = -G_PROBE if site == "h" else G_PROBE
        j = 5
        probe_layer0(net, G, -0.3, j=j, zero_col=(site == "b"))
        z = (float(net.lin0.weight_g.detach().reshape(-1)[j]) * np.sign(G) * x[:, 0].double() + float(net.lin0.bias.detach()[j])).numpy()
        loud = site == "a"
        uses = ("quiet", "large") if site == "h" else uses
        perturb = _perturb_fn("sdf", ["lin1"], [[j]], ["lin0"], [[j]])
    elif site in ("d", "e"):
        layer = 3 if site == "d" else 7
        j = probe_hidden(net, "sdf", spec, (x,), layer)
        z = hidden_preact("sdf", _sd(net, torch.float64), spec, (x,), layer)[:, j].numpy()
        perturb = _perturb_fn("sdf", ["lin%d" % (layer + 1)], [[j]], ["lin%d" % layer], [[j]])
    elif site == "c":
        blow = 1.8e5
        with torch.no_grad():
            net.lin0.weight_g.mul_(blow)
            net.lin0.bias.mul_(blow)
            net.lin1.weight_g.mul_(1.0 / blow)
        z0 = hidden_preact("sdf", _sd(net, torch.float64), spec, (x,), 0)
        z = z0.max(dim=1).values.numpy()
        uses = ("large",)     # (a few per cent of a uniform draw are dirty: the rows whose largest layer-0 pre-activation is)
        allc = list(range(256))
        perturb = _perturb_fn("sdf", ["lin1"], [allc], ["lin0"], [allc])
    elif site == "f":
        with torch.no_grad():
            x[1::2, 0] = 7.0e4
        z = np.where(np.arange(POOL) % 2 == 1, 7.0e4, -1.0)   # the "probe" is the input's own split
        uses = ("quiet", "dirty")
    else:
        raise ValueError(site)
    case = Case("sdf/" + site, "sdf", net, spec, (x,), strata_of(z), z, loud, uses, hot=(np.arange(POOL) % 2 == 1) if site == "f" else None)
    if site != "f":
        layer, cols = {"a": (0, [5]), "b": (0, [5]), "h": (0, [5]), "c": (0, list(range(256)))}.get(site) or (3 if site == "d" else 7, [j])
        case.stratum_fwd = _forward_mode_strata(case, layer, cols)
    return _finish(case, perturb=perturb)


def _forward_mode_strata(case: Case, layer: int, cols) -> np.ndarray:
    """A forward-mode kernel (k_sdf_grad_h2: one value and three tangent waves) carries d/dx_k of every activation through the same
    fp16 split: the probe's tangent softplus'(z_j) dz_j/dx_k is an operand too.  Where it leaves fp16's range the row is dirty (band)
    for such an entry although its activations are in range -- the reverse-mode kernel carries adjoints instead, which are small."""
    sd = _sd(case.net, torch.float64)
    x = case.inputs[0].double()

    def f(xx):
        return hidden_preact("sdf", sd, case.spec, (xx,), layer)[:, cols]
    z = f(x)
    t = torch.zeros(POOL, dtype=torch.float64)
    for k in range(3):
        v = torch.zeros_like(x)
        v[:, k] = 1.0
        _, jv = torch.autograd.functional.jvp(f, x, v)
        t = torch.maximum(t, (torch.sigmoid(100.0 * z) * jv).abs().max(dim=1).values)
    s = case.stratum.copy()
    t = t.numpy()
    s[(t >= F16_MAX) & (s != "dirty")] = "band"
    s[t >= F16_OVER] = "dirty"
    return s


# ---- builders: the material nets (the four h2 instances launch_material can pick) ------------------------------------------------------
def render_case(family: str, site: str) -> Case:
    """family: a key of _nets.RENDER_FAMILIES; site: a | e (last hidden layer) | d (in front of the skip layer; skip net only) | g
    (features of 1e5 on every other row) | h (G < 0)."""
    from iron_amd.fields import RenderingNetwork
    kw = dict(_nets.RENDER_FAMILIES[family])
    net = _nets.build(RenderingNetwork, kw, family + "/prod")
    spec = _nets.render_spec(kw)
    pts, nrm, view, feat = _render_inputs(31)
    ins = (pts, nrm if kw["mode"] in ("idr", "no_view_dir") else None, view if kw["mode"] == "idr" else None, feat)
    loud, uses, perturb = False, ("quiet", "large", "dirty"), None
    if site in ("a", "h"):
        G = -G_PROBE if site == "h" else G_PROBE
        j = 7
        probe_layer0(net, G, -0.35, j=j)
        z = (float(net.lin0.weight_g.detach().reshape(-1)[j]) * np.sign(G) * pts[:, 0].double() + float(net.lin0.bias.detach()[j])).numpy()
        loud = site == "a"
        uses = ("quiet", "large") if site == "h" else uses
        perturb = _perturb_fn("render", ["lin1"], [[j]], ["lin0"], [[j]])
    elif site in ("d", "e"):
        layer = 3 if site == "d" else kw["n_layers"] - 1
        j = probe_hidden(net, "render", spec, ins, layer)
        z = hidden_preact("render", _sd(net, torch.float64), spec, ins, layer)[:, j].numpy()
        perturb = _perturb_fn("render", ["lin%d" % (layer + 1)], [[j]], ["lin%d" % layer], [[j]])
    elif site == "g":
        with torch.no_grad():
            feat[1::2] *= 1.0e5 / 0.3
        ins = (ins[0], ins[1], ins[2], feat)
        z = np.where(np.arange(POOL) % 2 == 1, 1.0e5, -1.0)
        uses = ("quiet", "dirty")
    else:
        raise ValueError(site)
    case = Case("%s/%s" % (family, site), "render", net, spec, ins, strata_of(z), z, loud, uses,
                hot=(np.arange(POOL) % 2 == 1) if site == "g" else None)
    return _finish(case, perturb=perturb)


# ---- builders: the NeRF net ---------------------------------------------------------------------------------------------------------------
def nerf_case(site: str) -> Case:
    """site: a (probe in pts_linears.0 on the raw coordinate x_0) | v (probe in views_linears.0 on the raw view component v_0: the
    rgb head reads that layer's fp32 accumulators, so finite and right is a legitimate outcome) | w (a view component of 7e4 on
    every other row: the views layer's input split overflows, so rgb is lost and alpha, which never sees the view, is not)."""
    from iron_amd.fields import NeRF
    kw = _nets.nerf_kw("prod")
    net = _nets.build(NeRF, kw, "prod")
    spec = _nets.nerf_spec(kw)
    g = torch.Generator().manual_seed(41)
    pts = torch.rand(POOL, 4, generator=g) * 1.8 - 0.9
    views = torch.nn.functional.normalize(torch.randn(POOL, 3, generator=g), dim=-1)
    j = 9
    if site == "w":
        with torch.no_grad():
            views[1::2, 0] = 7.0e4
        z = np.where(np.arange(POOL) % 2 == 1, 7.0e4, -1.0)
        return _finish(Case("nerf/w", "nerf", net, spec, (pts, views), strata_of(z), z, False, ("quiet", "dirty"), hot=np.arange(POOL) % 2 == 1))
    if site == "a":
        lin, nxt, col, coord, p = net.pts_linears[0], net.pts_linears[1], j, pts[:, 0], -0.35
        row = torch.zeros(lin.in_features, dtype=torch.float64)
        row[0] = G_PROBE
        names = (["pts_linears.1"], ["pts_linears.0"])
    elif site == "v":
        lin, nxt, col, coord, p = net.views_linears[0], net.rgb_linear, j, views[:, 0], -0.45
        row = torch.zeros(lin.in_features, dtype=torch.float64)
        row[256] = G_PROBE          # input = [feature (256) | PE(view)]: column 256 is the raw v_0
        names = (["rgb_linear"], ["views_linears.0"])
    else:
        raise ValueError(site)
    with torch.no_grad():
        _set_row(lin, j, row, -G_PROBE * p)
        _set_column(nxt, col, 13, False)
    z = (G_PROBE * coord.double() + float(lin.bias.detach()[j])).numpy()
    case = Case("nerf/" + site, "nerf", net, spec, (pts, views), strata_of(z), z, site == "a", ("quiet", "large", "dirty"))
    return _finish(case, perturb=_perturb_fn("nerf", names[0], [[col]], names[1], [[j]]))


# ---- row arrangements ------------------------------------------------------------------------------------------------------------------
def arrangements(case: Case) -> Dict[str, np.ndarray]:
    """Index sets into the case's draw.  A workgroup is 4 waves x 32 points: n = 1, 33, 129, 300 (the draw's first rows, strata
    mixed), one dirty row behind 299 clean ones, dirty rows only in the ragged tail tile of 300 (rows 288..299), one dirty row alone."""
    out = {"n%d" % n: np.arange(n) for n in (33, 129, 300)}
    clean, dirty = case.clean_rows(), case.rows("dirty")
    out["n1"] = clean[:1]
    if len(dirty):
        out["last_dirty"] = np.concatenate([clean[:299], dirty[:1]])
        out["tail_dirty"] = np.concatenate([clean[:288], dirty[:12]])
        out["n1_dirty"] = dirty[:1]
    return out


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def judge(case: Case, idx, got: Dict[str, torch.Tensor], exact: bool = False, forward_mode: bool = False):
    """R1 on the rows `idx` of the case for the blocks in `got` ([len(idx), k] tensors; exact: R3, the plain yardstick and every row
    finite): returns (problems, any_bad_row, worst, nonfinite_row) -- nonfinite_row: [len(idx)] rows with a non-finite value; problems: finite values outside the yardstick and non-finite values on clean rows, as text; any_bad_row: some returned value
    is non-finite or outside the yardstick (R2: then, and only then, the handle's flag must be pending); worst: {(block, stratum):
    largest |got - fp64| / yardstick over the finite values}.  forward_mode: the entry differentiates in forward mode, so the probe's
    tangent is an operand of the h2 core as well (Case.stratum_fwd)."""
    idx = np.asarray(idx)
    stratum = case.stratum_fwd if (forward_mode and case.stratum_fwd is not None) else case.stratum
    problems, worst = [], {}
    bad_row = np.zeros(len(idx), dtype=bool)
    nonfinite_row = np.zeros(len(idx), dtype=bool)
    for k, v in got.items():
        v = v.detach().cpu().double().reshape(len(idx), -1)
        ref = case.ref64[k][idx].reshape(len(idx), -1)
        bound = case.exact_bound(k, idx) if exact else case.bound(k, idx, stratum)
        fin = torch.isfinite(v)
        ratio = torch.where(fin, (v - ref).abs() / bound, torch.zeros_like(v))
        wrong = (ratio > 1.0)
        bad_row |= (wrong.any(dim=1) | (~fin).any(dim=1)).numpy()
        nonfinite_row |= (~fin).any(dim=1).numpy()
        for s in STRATA:
            m = torch.from_numpy(stratum[idx] == s)
            if bool(m.any()):
                worst[(k, s)] = max(worst.get((k, s), 0.0), float(ratio[m].max()))
        if bool(wrong.any()):
            r, c = np.nonzero(wrong.numpy())
            problems.append("%s %s: %d finite values outside the yardstick, worst ratio %.2f at row %d (%s, z %.1f)"
                            % (case.name, k, len(r), float(ratio.max()), int(idx[r[0]]), stratum[idx[r[0]]], case.z[idx[r[0]]]))
        must = np.isin(stratum[idx], ("quiet", "large", "other")) | exact
        lost = must & (~fin).any(dim=1).numpy()
        if lost.any():
            problems.append("%s %s: %d clean rows came back non-finite (first: row %d, %s)"
                            % (case.name, k, int(lost.sum()), int(idx[np.nonzero(lost)[0][0]]), stratum[idx[np.nonzero(lost)[0][0]]]))
    return problems, bool(bad_row.any()), worst, nonfinite_row


def table_line(tag: str, worst: dict) -> str:
    return "envelope %-28s " % tag + "  ".join("%s/%s %.2f" % (k, s, r) for (k, s), r in sorted(worst.items()))


# ---- the list ---------------------------------------------------------------------------------------------------------------------------
SDF_SITES = ("a", "b", "c", "d", "e", "f", "h")
RENDER_KEYS = tuple("%s/%s" % (fam, site) for fam in _nets.RENDER_FAMILIES for site in ("a", "e", "g", "h")) + ("idr_10_4_skip/d",)
NERF_SITES = ("a", "v", "w")
ALL_KEYS = tuple("sdf/" + s for s in SDF_SITES) + tuple("render/" + k for k in RENDER_KEYS) + tuple("nerf/" + s for s in NERF_SITES)
_cache: Dict[str, Case] = {}


def get_case(key: str) -> Case:
    """Built once per process and left unchanged (the GPU tests move a deep copy of case.net to the device)."""
    if key not in _cache:
        kind, rest = key.split("/", 1)
        _cache[key] = sdf_case(rest) if kind == "sdf" else nerf_case(rest) if kind == "nerf" else render_case(*rest.rsplit("/", 1))
    return _cache[key]
