"""High-precision side of the per-row tests of the co-located BRDF heads (tests/test_brdf_oracle.py on the CPU,
tests/test_gpu_brdf_kernels.py on the GPU): csrc/ggx_core.h as instantiated with float (pointwise.hip, shade.hip) and with
Dual<N> (k_ggx_back, k_composite_back, k_coloc_head_back of train.hip).

The truth is oracle/iron_ref.py, which is dtype-generic, run in fp64 from the fp32 inputs (`run_as` / `fp64` / `ulp32` come from
_neus_oracle.py), forward and -- by torch autograd -- backward.  Two things are added to a plain fp64 run:

* the clamp bounds are those of the fp32 program.  `torch.clamp(x, min=0.00001)` on an fp32 tensor compares with
  float32(0.00001), and the kernels hold 0.00001f; a row that sits exactly on that fp32 bound is live (torch's clamp passes the
  gradient on [min, max]) in fp32 but would be dead in an fp64 run that compares with the double 0.00001.  `clamp_bounds("fp32")`
  rounds the Python bounds to fp32 for the length of a run, so that liveness is the fp32 program's and the value is fp64's.

* a per-entry yardstick y, from the fp64 side alone: what an fp32 evaluation can deliver FOR THAT ROW,

      y_i = 2 ulp32(o_i) + 1/2 sum_x sum_+- |o_i(x +- dx) - o_i(x)| + [mixed-sign sums only] 4 ulp32(sum |partial terms|)

  x runs over the fp32 scalars the formula consumes: the clamped cosine (dx = 2^-23 sum_k |v_k n_k|, the forward error of a
  three-term fp32 dot), roughness, distance or env light, the three optical constants and each albedo channel (dx = 1 ulp32).  The
  sensitivities are evaluated on the formula behind its clamps (`scalar space`: n = (0,0,1), v = (0,0,c), every clamped input
  already clamped, the clamps of differentiable inputs open), so that a row ON a bound is not perturbed across it.  An input that
  the clamp replaced keeps its dx: the roundings inside the formula are amplified like a perturbation of what it consumes
  (dielectric_eta clamped to 1.000001: cos_i - eta cos_t loses 6 % to one rounding of 1 - sin^2 / eta^2).  The partial terms of a
  gradient entry are upstream x albedo x the terms that the derivative of the lobe adds up (class AD); d/dalpha of the GGX lobe at
  grazing incidence is the textbook case: d ln D/dalpha -> +2/alpha, 2 d ln G1/dalpha -> -2/alpha.

Flags, also from the fp64 side only, mark the discrete decisions no fp32 evaluation can be asked to reproduce: a warped table
coordinate within 1e-4 of an integer (the diffuse lobe of that row is excused), and a raw dot or a clamped input that lies
within 4 ulp32 of a bound -- for the dot, within twice its fp32 forward error dx if that is more -- without being equal to it.

Nothing here touches the GPU."""
from __future__ import annotations

import contextlib
import functools
import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from _neus_oracle import run_as, ulp32
from oracle import iron_ref as R

LIGHT = 31.0
N_ROWS = 130                      # two full waves plus two lanes: the backward kernels run 64 threads per block
SMALL_DISTANCE_ROWS = (3, 67, 129)
TABLE_DELTA = 1e-4
OPEN_SLACK = 0.025   # scalar space: a clamp lets a perturbed input through (dx / x <= 2^-23 / 1e-5 = 1.2 % for the cosine)


def f32(x: float) -> float:
    return float(np.float32(x))


COS_LO, COS_HI = f32(0.00001), f32(0.99999)
# clamped inputs: (low bound, high bound) per head family, as the fp32 program holds them
BOUNDS_GGX = {"rough": (f32(0.0001), None)}
BOUNDS_COMPOSITE = {"rough": (f32(0.00001), None), "m_eta": (f32(0.099999), f32(4.999999)), "m_k": (f32(0.099999), f32(9.999999)),
                    "d_eta": (f32(1.000001), f32(1.999999)), "kd": (f32(0.00001), None), "ks": (f32(0.00001), None),
                    "env_light": (f32(0.000001), f32(20.0))}

HEADS = ("ggx", "composite", "composite_env", "smooth_dielectric", "thin_dielectric", "smooth_conductor", "rough_conductor")
FIELDS = ("distance", "normal", "viewdir", "kd", "ks", "rough", "m_eta", "m_k", "d_eta", "env_light")


def is_composite(head: str) -> bool:
    return head.startswith("composite")


def bounds(head: str) -> Dict[str, tuple]:
    if is_composite(head):
        b = dict(BOUNDS_COMPOSITE)
        if head == "composite":
            del b["env_light"]
        return b
    return dict(BOUNDS_GGX) if head in ("ggx", "rough_conductor") else {}


def inputs_of(head: str) -> tuple:
    """The differentiable inputs of a head, in the names of the stratum dicts."""
    if head == "composite":
        return ("light", "distance", "normal", "viewdir", "kd", "ks", "rough", "m_eta", "m_k", "d_eta")
    if head == "composite_env":
        return ("normal", "viewdir", "kd", "ks", "rough", "m_eta", "m_k", "d_eta", "env_light")
    base = ("light", "distance", "normal", "viewdir", "kd", "ks")
    return base + ("rough",) if head in ("ggx", "rough_conductor") else base


def upstream_keys(head: str) -> tuple:
    if head == "composite":
        return ("rgb", "specular_rgb", "metallic_rgb", "dielectric_rgb")
    if head == "composite_env":
        return ("rgb", "specular_rgb", "metallic_rgb", "dielectric_rgb", "env_light")
    return ("diffuse_rgb", "specular_rgb", "rgb")


@functools.lru_cache(maxsize=None)
def tables():
    """(MTS_TRANS [5000], MTS_DIFF_TRANS [50]) as CPU fp32 tensors, read without importing the GPU package."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iron_amd", "data", "mts_rtrans_tables.npz")
    z = np.load(path, allow_pickle=False)
    return torch.from_numpy(z["ext_rtrans"].astype(np.float32)), torch.from_numpy(z["int_diff_rtrans"].astype(np.float32))


def oracle(head: str, v: Dict[str, torch.Tensor], mt: torch.Tensor, md: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The head's function of oracle/iron_ref.py on a stratum dict, in the dtype of its tensors.  The composite's "diffuse_rgb"
    is the same tensor as its "rgb" and is left out."""
    if head == "ggx":
        p = {"diffuse_albedo": v["kd"], "specular_albedo": v["ks"], "specular_roughness": v["rough"]}
        return R.ggx_colocated(v["light"], v["distance"], v["normal"], v["viewdir"], p, mt, md)
    if is_composite(head):
        p = {"diffuse_albedo": v["kd"], "specular_albedo": v["ks"], "specular_roughness": v["rough"], "metallic_eta": v["m_eta"],
             "metallic_k": v["m_k"], "dielectric_eta": v["d_eta"], "env_light": v["env_light"]}
        out = dict(R.composite_forward(v["light"], v["distance"], v["normal"], v["viewdir"], p, mt, md, use_env_light=head == "composite_env"))
        del out["diffuse_rgb"]
        return out
    return getattr(R, head)(v["light"], v["distance"], v["normal"], v["viewdir"], v["kd"], v["ks"], v["rough"] if head == "rough_conductor" else None)


@contextlib.contextmanager
def clamp_bounds(mode: Optional[str]):
    """torch.clamp for the length of an oracle run: "fp32" rounds Python bounds to fp32 (see the module docstring); "open" also
    passes the gradient of every tensor that requires grad and moves only values more than OPEN_SLACK outside the bounds (scalar
    space: the inputs arrive clamped and are perturbed by a few ulp; the composite's table lookup still needs its second, wider
    roughness clamp); None leaves torch alone."""
    calls = [0]
    if mode is None:
        yield calls
        return
    real = torch.clamp   # the module attribute is replaced: this reaches torch.clamp(x, ...) calls only, not x.clamp(...); `evaluate` asserts
                         # that the oracle came through here, so that an edit of iron_ref.py cannot silently lose the fp32 bounds

    def rnd(b):
        return b if (b is None or torch.is_tensor(b)) else f32(b)

    def clamp(x, min=None, max=None):
        calls[0] += 1
        if not x.is_floating_point():
            return real(x, min=min, max=max)
        if mode == "open" and x.requires_grad:   # straight through, and only a value well outside the bounds is moved at all
            lo, hi = (None if min is None else rnd(min) * (1.0 - OPEN_SLACK)), (None if max is None else rnd(max) * (1.0 + OPEN_SLACK))
            return x + (real(x, min=lo, max=hi) - x).detach()
        return real(x, min=rnd(min), max=rnd(max))

    torch.clamp = clamp
    try:
        yield calls
    finally:
        torch.clamp = real


def evaluate(head: str, inp: Dict[str, torch.Tensor], ups: Dict[str, Optional[torch.Tensor]], dtype, mode: Optional[str], wrt=None):
    """(outputs, gradients of sum_k <ups[k], out[k]> w.r.t. `wrt`) of the oracle in `dtype`; an unused input gets zeros."""
    wrt = inputs_of(head) if wrt is None else wrt
    mt, md = tables()

    def body(inp, ups, mt, md):
        leaves = {k: (x.clone().requires_grad_(True) if k in wrt else x) for k, x in inp.items()}
        with clamp_bounds(mode) as calls:
            out = oracle(head, leaves, mt, md)
            assert mode is None or calls[0] > 0, "oracle/iron_ref.py no longer clamps through torch.clamp(...)"
            loss = sum((out[k] * u).sum() for k, u in ups.items() if u is not None)
            g = torch.autograd.grad(loss, [leaves[k] for k in wrt], allow_unused=True)
        return ({k: o.detach() for k, o in out.items()},
                {k: (torch.zeros_like(leaves[k]) if x is None else x.detach()) for k, x in zip(wrt, g)})

    return run_as(dtype, body, inp, ups, mt, md)


# ---- input builders ------------------------------------------------------------------------------------------------------
def _uniform(gen, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, 1, generator=gen, dtype=torch.float64)


def _log_uniform(gen, n, lo, hi):
    return torch.exp(_uniform(gen, n, math.log(lo), math.log(hi)))


def _axis_aligned(c: float):
    """n = (0,0,1), v = (sqrt(1 - c^2), 0, c): the kernel's dot (v0 n0 + v1 n1) + v2 n2 is exactly c."""
    return torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), torch.tensor([math.sqrt(1.0 - c * c), 0.0, c], dtype=torch.float64)


def _directions(gen, cos: torch.Tensor):
    """A unit normal and a view direction with the wanted n.v, built in fp64 ([n, 3] each)."""
    n = cos.shape[0]
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=-1)
    t = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    t = torch.nn.functional.normalize(t - (t * nrm).sum(-1, keepdim=True) * nrm, dim=-1)
    return nrm, cos * nrm + torch.sqrt((1.0 - cos * cos).clamp(min=0.0)) * t


def _base(gen, n: int, cos: torch.Tensor, rough: torch.Tensor) -> Dict[str, torch.Tensor]:
    nrm, view = _directions(gen, cos)
    dist = _uniform(gen, n, 0.5, 2.5)
    for r in SMALL_DISTANCE_ROWS:
        if r < n:
            dist[r] = 1e-3
    s = {"distance": dist, "normal": nrm, "viewdir": view, "rough": rough,
         "kd": 0.05 + 0.95 * torch.rand(n, 3, generator=gen, dtype=torch.float64), "ks": 0.05 + 0.45 * torch.rand(n, 3, generator=gen, dtype=torch.float64),
         "m_eta": _uniform(gen, n, 0.2, 4.5), "m_k": _uniform(gen, n, 0.2, 9.5), "d_eta": _uniform(gen, n, 1.05, 1.95),
         "env_light": _log_uniform(gen, n, 0.01, 15.0)}
    return s


def _on_bound_dirs(s, rows, c: float):
    nrm, view = _axis_aligned(c)
    for r in rows:
        s["normal"][r], s["viewdir"][r] = nrm, view


def _finish(s) -> Dict[str, torch.Tensor]:
    return {k: v.float().contiguous() for k, v in s.items()}


# category pattern of the two-sided clamps: 20 below, 10 on the low bound, 70 inside, 10 on the high bound, 20 above (130 rows)
_PATTERN = ("below", "below", "low", "in", "in", "in", "in", "high", "above", "above", "in", "in", "in")


def _categories(n: int, mult: int) -> List[str]:
    return [_PATTERN[(i * mult) % 13] for i in range(n)]


def _two_sided(gen, n, mult, lo, hi, below, inside, above):
    x = torch.empty(n, 1, dtype=torch.float64)
    for i, cat in enumerate(_categories(n, mult)):
        u = float(torch.rand(1, generator=gen, dtype=torch.float64))
        x[i] = {"below": below[0] + u * (below[1] - below[0]), "low": lo, "in": inside[0] + u * (inside[1] - inside[0]), "high": hi,
                "above": above[0] + u * (above[1] - above[0])}[cat]
    return x


def stratum(name: str, n: int = N_ROWS, seed: int = 0) -> Dict[str, torch.Tensor]:
    """fp32 CPU inputs of one stratum (every field of FIELDS; a head reads the ones it uses)."""
    gen = torch.Generator().manual_seed(1000 * (sorted(STRATA).index(name) + 1) + seed)
    U, LU = functools.partial(_uniform, gen, n), functools.partial(_log_uniform, gen, n)
    interior_cos, interior_rough = (0.05, 0.95), (0.02, 0.7)
    if name == "interior":
        return _finish(_base(gen, n, U(*interior_cos), U(*interior_rough)))
    if name == "grazing":
        return _finish(_base(gen, n, LU(1.1e-5, 1e-2), U(*interior_rough)))
    if name == "near_normal":
        return _finish(_base(gen, n, 1.0 - LU(1.1e-5, 1e-3), U(*interior_rough)))
    if name == "glossy":
        return _finish(_base(gen, n, U(*interior_cos), LU(1.1e-4, 1e-2)))
    if name == "glossy_near_normal":
        return _finish(_base(gen, n, 1.0 - LU(1.1e-5, 1e-3), LU(1.1e-4, 1e-2)))
    if name == "very_rough":
        return _finish(_base(gen, n, U(*interior_cos), U(0.7, 1.5)))
    if name == "clamp_cos_low":    # 40 rows back-facing, 40 in (0, 1e-5), 6 on the bound, 44 live close above it
        cos = torch.cat([-_uniform(gen, 40, 0.01, 0.9), _log_uniform(gen, 40, 1e-8, 9e-6), torch.full((6, 1), COS_LO, dtype=torch.float64),
                         _log_uniform(gen, n - 86, 1.2e-5, 1e-3)])
        s = _base(gen, n, cos, U(*interior_rough))
        _on_bound_dirs(s, range(80, 86), COS_LO)
        return _finish(s)
    if name == "clamp_cos_high":   # 30 rows above the bound, 10 with v == n, 6 on the bound, 84 live close below it
        cos = torch.cat([1.0 - _log_uniform(gen, 40, 1e-8, 8e-6), torch.full((6, 1), COS_HI, dtype=torch.float64),
                         1.0 - _log_uniform(gen, n - 46, 1.2e-5, 1e-3)])
        s = _base(gen, n, cos, U(*interior_rough))
        s["viewdir"][30:40] = s["normal"][30:40]
        _on_bound_dirs(s, range(40, 46), COS_HI)
        return _finish(s)
    if name == "clamp_rough":      # 0, negative, below 1e-5, in [1e-5, 1e-4), on either bound, live
        rough = torch.cat([torch.zeros(15, 1, dtype=torch.float64), -_uniform(gen, 15, 1e-3, 0.5), _log_uniform(gen, 20, 1e-8, 9e-6),
                           _log_uniform(gen, 20, 1.1e-5, 9e-5), torch.full((5, 1), BOUNDS_GGX["rough"][0], dtype=torch.float64),
                           torch.full((5, 1), BOUNDS_COMPOSITE["rough"][0], dtype=torch.float64), _log_uniform(gen, n - 80, 1.1e-4, 0.5)])
        return _finish(_base(gen, n, U(*interior_cos), rough))
    s = _base(gen, n, U(*interior_cos), U(*interior_rough))
    B = BOUNDS_COMPOSITE
    if name == "clamp_optics":
        s["m_eta"] = _two_sided(gen, n, 1, *B["m_eta"], (0.01, 0.09), (0.2, 4.5), (5.1, 8.0))
        s["m_k"] = _two_sided(gen, n, 2, *B["m_k"], (0.01, 0.09), (0.2, 9.5), (10.1, 15.0))
        s["d_eta"] = _two_sided(gen, n, 3, *B["d_eta"], (0.5, 0.99), (1.05, 1.95), (2.001, 3.0))
    elif name == "eta_near_one":
        s["d_eta"] = 1.0 + LU(2e-6, 1e-2)
    elif name == "clamp_albedo":   # one channel of kd and one of ks per row: 0, negative, below 1e-5, on it, or left alone
        for key, mult in (("kd", 1), ("ks", 2)):
            for i, cat in enumerate(_categories(n, mult)):
                u = float(torch.rand(1, generator=gen, dtype=torch.float64))
                ch = (i + mult) % 3
                if cat == "below":
                    s[key][i, ch] = (0.0, -0.3 * u, 1e-8 * (900.0 ** u))[i % 3]
                elif cat in ("low", "high"):
                    s[key][i, ch] = B[key][0]
    elif name == "clamp_env":
        env = _two_sided(gen, n, 1, *B["env_light"], (1e-9, 9e-7), (1e-3, 19.0), (20.5, 50.0))
        env[0], env[13] = 0.0, -2.0
        s["env_light"] = env
    else:
        raise KeyError(name)
    return _finish(s)


STRATA = {"interior", "grazing", "near_normal", "glossy", "glossy_near_normal", "very_rough", "clamp_cos_low", "clamp_cos_high", "clamp_rough",
          "clamp_optics", "eta_near_one", "clamp_albedo", "clamp_env", "single"}
TABLE_STRATA = ("interior", "grazing", "near_normal", "glossy", "glossy_near_normal", "very_rough")
# per clamp stratum, the clamped quantity it is about: (input name, heads it applies to)
CLAMP_STRATA = {"clamp_cos_low": "cos", "clamp_cos_high": "cos", "clamp_rough": "rough", "clamp_optics": ("m_eta", "m_k", "d_eta"),
                "clamp_albedo": ("kd", "ks"), "clamp_env": "env_light"}


def strata_of(head: str) -> tuple:
    cos = ("clamp_cos_low", "clamp_cos_high")
    if head in ("smooth_dielectric", "thin_dielectric"):   # no cosine, no roughness in the formula: the clamp must still be dead
        return ("interior", "clamp_cos_low", "single")
    if head == "smooth_conductor":
        return ("interior", "grazing", "near_normal") + cos + ("single",)
    if head in ("ggx", "rough_conductor"):
        return TABLE_STRATA + cos + ("clamp_rough", "single")
    extra = ("clamp_rough", "clamp_optics", "eta_near_one", "clamp_albedo") + (("clamp_env",) if head == "composite_env" else ())
    return TABLE_STRATA + cos + extra + ("single",)


@functools.lru_cache(maxsize=None)
def stratum_inputs(name: str) -> Dict[str, torch.Tensor]:
    if name == "single":
        return {k: v[:1].clone() for k, v in stratum("interior").items()}
    return stratum(name)


def upstreams(head: str, n: int, seed: int = 77) -> Dict[str, Dict[str, Optional[torch.Tensor]]]:
    """Upstream gradients per configuration: each output alone with an all-positive upstream (None for the others: the kernels'
    null-pointer paths), and all outputs together, random-signed."""
    gen = torch.Generator().manual_seed(seed)
    keys = upstream_keys(head)
    width = lambda k: 1 if k == "env_light" else 3
    cfg = {}
    for k in keys:
        cfg["solo:" + k] = {j: (0.5 + torch.rand(n, width(j), generator=gen) if j == k else None) for j in keys}
    cfg["mixed"] = {j: torch.randn(n, width(j), generator=gen) for j in keys}
    return cfg


# ---- scalar space: the formula behind its clamps -----------------------------------------------------------------------------
def _clamped(x64: torch.Tensor, b) -> torch.Tensor:
    lo, hi = b
    return x64.clamp(min=lo, max=hi) if hi is not None else x64.clamp(min=lo)


def raw_dot(inp) -> torch.Tensor:
    return (inp["viewdir"].double() * inp["normal"].double()).sum(-1, keepdim=True)


def dot_delta(inp) -> torch.Tensor:
    """2^-23 sum_k |v_k n_k|: the forward error bound of the three-term fp32 dot."""
    return 2.0 ** -23 * (inp["viewdir"].double() * inp["normal"].double()).abs().sum(-1, keepdim=True)


def scalars(head: str, inp) -> Dict[str, Dict[str, torch.Tensor]]:
    """{"x": clamped fp64 scalars, "dx": their perturbations} for the variables the head's formula consumes: c, u (distance, or
    env light), rough, m_eta, m_k, d_eta [n, 1], kd, ks [n, 3]."""
    b = bounds(head)
    dot = raw_dot(inp)
    x = {"c": dot.clamp(COS_LO, COS_HI)}
    dx = {"c": dot_delta(inp)}
    names = {"u": "env_light" if head == "composite_env" else "distance", "kd": "kd", "ks": "ks"}
    if head in ("ggx", "rough_conductor") or is_composite(head):
        names["rough"] = "rough"
    if is_composite(head):
        names.update(m_eta="m_eta", m_k="m_k", d_eta="d_eta")
    for var, field in names.items():
        raw = inp[field].double()
        x[var] = _clamped(raw, b[field]) if field in b else raw
        dx[var] = ulp32(x[var])
    return {"x": x, "dx": dx}


def _scalar_inputs(head: str, x: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    m = x["c"].shape[0]
    zero, one = torch.zeros(m, 1, dtype=torch.float64), torch.ones(m, 1, dtype=torch.float64)
    inp = {"light": torch.tensor(LIGHT, dtype=torch.float64), "normal": torch.cat([zero, zero, one], -1), "viewdir": torch.cat([zero, zero, x["c"]], -1),
           "kd": x["kd"], "ks": x["ks"], "distance": one, "env_light": one}
    inp["env_light" if head == "composite_env" else "distance"] = x["u"]
    for k in ("rough", "m_eta", "m_k", "d_eta"):
        inp[k] = x.get(k, one)
    return inp


def _scalar_wrt(head: str):
    """(variable, oracle input) pairs of the scalar-space gradients."""
    pairs = [("c", "viewdir"), ("u", "env_light" if head == "composite_env" else "distance"), ("kd", "kd"), ("ks", "ks")]
    if head in ("ggx", "rough_conductor") or is_composite(head):
        pairs.append(("rough", "rough"))
    if is_composite(head):
        pairs += [("m_eta", "m_eta"), ("m_k", "m_k"), ("d_eta", "d_eta")]
    return pairs


def light_rows(head: str, out, ups) -> torch.Tensor:
    """[n, 1]: the per-row terms of d loss / d light (the outputs are linear in the light)."""
    t = 0.0
    for k, u in ups.items():
        if u is not None and k != "env_light":
            t = t + (out[k].double() * u.double()).sum(-1, keepdim=True)
    return t / LIGHT


def scalar_entries(head: str, x: Dict[str, torch.Tensor], ups) -> Dict[str, torch.Tensor]:
    """Every output entry as a function of the clamped scalars, in fp64: "out:<key>", "d:<variable>", "d:light"."""
    pairs = _scalar_wrt(head)
    out, g = evaluate(head, _scalar_inputs(head, x), ups, torch.float64, "open", wrt=tuple(f for _, f in pairs))
    e = {"out:" + k: v for k, v in out.items()}
    for var, field in pairs:
        e["d:" + var] = g[field][:, 2:3] if var == "c" else g[field]
    if head != "composite_env":
        e["d:light"] = light_rows(head, out, ups)
    return e


def sensitivity(head: str, sc, ups) -> Dict[str, torch.Tensor]:
    """1/2 sum_x sum_+- |e(x +- dx) - e(x)| per entry: all perturbed copies run as one stacked batch."""
    x, dx = sc["x"], sc["dx"]
    m = x["c"].shape[0]
    moves = []
    for var in x:
        for ch in range(x[var].shape[1]):
            for sign in (1.0, -1.0):
                moves.append((var, ch, sign))
    stacked = {}
    for var in x:
        copies = [x[var]]
        for mv, ch, sign in moves:
            if mv == var:
                y = x[var].clone()
                y[:, ch] += sign * dx[var][:, ch]
                copies.append(y)
            else:
                copies.append(x[var])
        stacked[var] = torch.cat(copies)
    reps = len(moves) + 1
    ups_s = {k: (None if u is None else u.double().repeat(reps, 1)) for k, u in ups.items()}
    e = scalar_entries(head, stacked, ups_s)
    sens = {}
    for k, v in e.items():
        v = v.reshape(reps, m, -1)
        sens[k] = 0.5 * (v[1:] - v[:1]).abs().sum(0)
    return sens


# ---- partial terms of the gradients ---------------------------------------------------------------------------------------------
def _abs(x):
    return x.abs() if torch.is_tensor(x) else abs(x)


U32 = 2.0 ** -24   # unit roundoff of fp32
_RUNNING = [False]  # AD: cancelling sums add to ev (inside the two Fresnel terms only, see AD)


def _lost(x, y, z):
    """What a cancelling sum z = x +- y adds to the error of its value, where that is being followed: the operands come with one
    rounding each, U32 (|x| + |y|) together; the part of it that a benign operation would have too, U32 |z|, is in the yardstick's
    ulp terms already, the excess is what the cancellation amplifies."""
    return U32 * (_abs(x) + _abs(y) - _abs(z)) if _RUNNING[0] else 0.0


class AD:
    """A value v with its derivatives d[x] in the scalar variables, and beside them three running sums:

      m[x]   the magnitudes of the terms that make up d[x]: every elementary operation adds |.| where the derivative adds signed
             terms.  This is the `sum |partial terms|` of the yardstick at the finest grain.  At the grain of whole factors
             (d ln D/dx against 2 d ln G1/dx) it already explains the GGX lobe, but the two Fresnel terms are no products: their own
             differences (term1 - term2, eta^2 - k^2 - sin^2, cos_i - eta cos_t) cancel inside one factor, and the honest fp32
             evaluation shows it: with whole factors it misses y by up to 120 x on d/dn of the composite (glossy near-normal rows)
             and 150 x on d/d metallic_k (grazing).
      ev     what the cancelling sums inside the two Fresnel terms cost the value: each such sum z = x +- y adds the excess
             U32 (|x| + |y| - |z|) of its operands' roundings over the rounding of a benign result (`_lost`); every other operation
             only passes on, to first order, what its operands carry.  No worst-case running bound: an operation's own rounding
             is what the yardstick's ulp terms are for, and ev is exactly 0 where nothing cancels.
      ed[x]  what ev costs d[x]: the coefficients of the chain rule (y in d(xy) = y dx + x dy, 1 / 2 sqrt(x), ...) are rounded
             intermediates themselves.  sqrt((a^2+b^2) + temp1) of the conductor's Fresnel term with temp1 < 0 loses three digits,
             and d/d eta runs through it: without this term the honest fp32 evaluation misses y by 63 x on d/d metallic_eta,
             9-10 x on d ks, 10.5 x on d env_light (all with both optical constants on their low clamps) and 8.2-8.5 x on d/dn at
             grazing incidence under a metallic-only upstream; with it, by at most 0.3 on those entries.

    ed enters the yardstick of the gradients (`cancellation`), ev that of the forward outputs.  Without ev the honest fp32
    evaluation misses the forward y of metallic_rgb, with both constants on their low clamps, by 7.1-8.0 on one CPU and by 9.5-12
    on another (torch's vectorised sqrt and division differ between them): the same lost digits.  Inputs are exact here: what
    their rounding costs is the sensitivity term.  `_RUNNING` is a module global switched by `_running` around the two Fresnel
    terms and restored in a finally block: AD is used from one thread, by partial_sums alone."""

    def __init__(self, v, d=None, m=None, ev=0.0, ed=None):
        self.v, self.d, self.m, self.ev, self.ed = v, d or {}, m or {}, ev, ed or {}

    @staticmethod
    def var(x, name):
        return AD(x, {name: torch.ones_like(x)}, {name: torch.ones_like(x)}, 0.0, {name: torch.zeros_like(x)})

    @staticmethod
    def lift(x):
        return x if isinstance(x, AD) else AD(x)

    def _lin(self, o, sa, sb, v, ev, e_sa=0.0, e_sb=0.0):   # v (error ev) with derivative sa * self' + sb * o'
        o = AD.lift(o)
        keys = set(self.d) | set(o.d)
        g = lambda t, k: t[k] if k in t else 0.0
        d = {k: sa * g(self.d, k) + sb * g(o.d, k) for k in keys}
        m = {k: _abs(sa) * g(self.m, k) + _abs(sb) * g(o.m, k) for k in keys}
        ed = {k: _abs(sa) * g(self.ed, k) + _abs(sb) * g(o.ed, k) + e_sa * g(self.m, k) + e_sb * g(o.m, k) for k in keys}
        return AD(v, d, m, ev, ed)

    def __add__(self, o):
        o = AD.lift(o)
        return self._lin(o, 1.0, 1.0, self.v + o.v, self.ev + o.ev + _lost(self.v, o.v, self.v + o.v))

    __radd__ = __add__

    def __sub__(self, o):
        o = AD.lift(o)
        return self._lin(o, 1.0, -1.0, self.v - o.v, self.ev + o.ev + _lost(self.v, o.v, self.v - o.v))

    def __rsub__(self, o):
        return AD.lift(o).__sub__(self)

    def __mul__(self, o):
        o = AD.lift(o)
        return self._lin(o, o.v, self.v, self.v * o.v, self.ev * _abs(o.v) + _abs(self.v) * o.ev, o.ev, self.ev)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = AD.lift(o)
        q = self.v / o.v
        eq = self.ev / _abs(o.v) + _abs(q) * o.ev / _abs(o.v)
        return self._lin(o, 1.0 / o.v, -q / o.v, q, eq, o.ev / (o.v * o.v), (eq + _abs(q) * o.ev / _abs(o.v)) / _abs(o.v))

    def __rtruediv__(self, o):
        return AD.lift(o).__truediv__(self)

    def sqrt(self):
        r = torch.sqrt(self.v)
        er = 0.5 * self.ev / r
        return self._lin(0.0, 0.5 / r, 0.0, r, er, 0.5 * er / (r * r))

    def hypot1(self):
        r = torch.hypot(self.v, torch.ones_like(self.v))
        er = _abs(self.v) / r * self.ev
        return self._lin(0.0, self.v / r, 0.0, r, er, self.ev / r + _abs(self.v) * er / (r * r))


def _running(fn):
    @functools.wraps(fn)
    def wrapped(*args):
        _RUNNING[0] = True
        try:
            return fn(*args)
        finally:
            _RUNNING[0] = False
    return wrapped


def _ad_smith_g1(c, a):
    tan = (1.0 - c * c).sqrt() / (c + 1e-10)
    return 2.0 / (1.0 + (a * tan).hypot1())


def _ad_ggx_ndf(c, a):
    c2 = c * c
    root = c2 + (1.0 - c2) / (a * a + 1e-10)
    return 1.0 / (np.pi * a * a * root * root + 1e-10)


def _ad_composite_ndf(c):
    eta = 1.48958738
    c2 = c * c
    root = c2 + (1.0 - c2) / (eta * eta + 1e-10)
    return 1.0 / (np.pi * eta * eta * root * root + 1e-10)


@_running
def _ad_fresnel_conductor(c, eta, k):
    eta, k = AD.lift(eta), AD.lift(k)
    c2 = c * c
    s2 = 1.0 - c2
    s4 = s2 * s2
    temp1 = eta * eta - k * k - s2
    a2pb2 = (temp1 * temp1 + 4.0 * k * k * eta * eta).sqrt()
    a = (0.5 * (a2pb2 + temp1)).sqrt()
    term1 = a2pb2 + c2
    term2 = 2.0 * a * c
    rs2 = (term1 - term2) / (term1 + term2)
    term3 = a2pb2 * c2 + s4
    term4 = term2 * s2
    rp2 = rs2 * (term3 - term4) / (term3 + term4)
    return 0.5 * (rp2 + rs2)


@_running
def _ad_fresnel_dielectric(c, eta):
    scale = 1.0 / eta
    cos_t = (1.0 - (1.0 - c * c) * (scale * scale)).sqrt()
    rs = (c - eta * cos_t) / (c + eta * cos_t)
    rp = (eta * c - cos_t) / (eta * c + cos_t)
    return 0.5 * (rs * rs + rp * rp)


def lobes(head: str, x: Dict[str, torch.Tensor]):
    """{lobe: (albedo variable, the lobe per unit albedo as an AD in the clamped scalars `x`, the outputs that contain the lobe)}:
    the formulas of oracle/iron_ref.py once more, in the one form that also yields m[x]; test_brdf_oracle.py holds their values
    and derivatives against the oracle's own."""
    v = {k: AD.var(t, k) for k, t in x.items() if k not in ("kd", "ks", "_diffuse_const")}
    c = v["c"]
    inten = v["u"] if head == "composite_env" else LIGHT / (v["u"] * v["u"] + 1e-10)
    t12 = x["_diffuse_const"]   # the table factors: piecewise constant
    if is_composite(head):
        g1 = _ad_smith_g1(c, v["rough"])
        return {"metallic": ("ks", _ad_fresnel_conductor(c, v["m_eta"], v["m_k"]) * inten, ("metallic_rgb", "specular_rgb", "rgb")),
                "dielectric": ("ks", _ad_fresnel_dielectric(c, v["d_eta"]) * _ad_composite_ndf(c) * (g1 * g1) / (4.0 * c) * inten,
                               ("dielectric_rgb", "specular_rgb", "rgb")),
                "diffuse": ("kd", inten * c * t12, ("rgb",))}
    spec = inten
    if head == "ggx":
        spec = spec * 0.03867
    if head == "smooth_dielectric":
        spec = spec * 0.04
    if head == "thin_dielectric":
        spec = spec * (0.04 + 0.96 * 0.96 * 0.04 / (1.0 - 0.04 * 0.04))
    if head in ("smooth_conductor", "rough_conductor"):
        spec = spec * _ad_fresnel_conductor(c, 2.58, 8.21)
    if head in ("ggx", "rough_conductor"):
        g1 = _ad_smith_g1(c, v["rough"])
        spec = spec * _ad_ggx_ndf(c, v["rough"]) * (g1 * g1) / (4.0 * c + 1e-10)
    return {"specular": ("ks", spec, ("specular_rgb", "rgb")), "diffuse": ("kd", inten * c * t12 if head == "ggx" else inten * 0.0001, ("diffuse_rgb", "rgb"))}


def lobe_values(head: str, out) -> Dict[str, torch.Tensor]:
    if is_composite(head):
        return {"metallic": out["metallic_rgb"], "dielectric": out["dielectric_rgb"], "diffuse": out["rgb"] - out["specular_rgb"]}
    return {"specular": out["specular_rgb"], "diffuse": out["diffuse_rgb"]}


def partial_sums(head: str, sc, ups, entries) -> Dict[str, Dict[str, torch.Tensor]]:
    """Per gradient entry "d:<variable>", the sum of its partial terms ("signed": it is the gradient again, which checks the
    restated formulas) and the sum of their magnitudes ("abs"), in fp64 at the clamped scalars; "lobe": the lobes' values."""
    x = dict(sc["x"])
    vals = lobe_values(head, {k[4:]: e for k, e in entries.items() if k.startswith("out:")})
    if head == "ggx" or is_composite(head):   # the table factor of the diffuse lobe, read off the oracle's own value
        inten = x["u"] if head == "composite_env" else LIGHT / (x["u"] * x["u"] + 1e-10)
        x["_diffuse_const"] = (vals["diffuse"] / x["kd"])[:, :1] / (inten * x["c"])
    else:
        x["_diffuse_const"] = None
    lb = lobes(head, x)
    names = [k for k in sc["x"]]
    signed = {"d:" + k: torch.zeros_like(sc["x"][k]) for k in names}
    mag = {"d:" + k: torch.zeros_like(sc["x"][k]) for k in names}
    carried = {"d:" + k: torch.zeros_like(sc["x"][k]) for k in names}
    if head != "composite_env":
        signed["d:light"], mag["d:light"] = torch.zeros_like(x["c"]), torch.zeros_like(x["c"])
    lobe_v, value_lost = {}, {}
    for name, (albedo, K, outs) in lb.items():
        lobe_v[name] = K.v * x[albedo]
        for o in outs:   # what the Fresnel terms' cancelling sums cost the lobe's value, per output that contains it (0 where none cancels)
            value_lost[o] = value_lost.get(o, 0.0) + K.ev * x[albedo].abs()
        for o in outs:
            u = ups.get(o)
            if u is None:
                continue
            ua = u.double() * x[albedo]   # [n, 3]: upstream x albedo per channel
            for k in K.d:
                signed["d:" + k] += (ua * K.d[k]).sum(-1, keepdim=True)
                mag["d:" + k] += (ua.abs() * K.m[k]).sum(-1, keepdim=True)
                carried["d:" + k] += (ua.abs() * K.ed[k]).sum(-1, keepdim=True)
            signed["d:" + albedo] += u.double() * K.v
            mag["d:" + albedo] += (u.double() * K.v).abs()
            carried["d:" + albedo] += u.double().abs() * K.ev
            if head != "composite_env":
                signed["d:light"] += (ua * K.v).sum(-1, keepdim=True) / LIGHT
                mag["d:light"] += (ua * K.v).abs().sum(-1, keepdim=True) / LIGHT
                carried["d:light"] = carried.get("d:light", 0.0) + (ua.abs() * K.ev).sum(-1, keepdim=True) / LIGHT
    if head == "composite_env" and ups.get("env_light") is not None:   # the "env_light" output is the clamp itself
        signed["d:u"] += ups["env_light"].double()
        mag["d:u"] += ups["env_light"].double().abs()
    return {"signed": signed, "abs": mag, "carried": carried, "value_lost": value_lost, "lobe": lobe_v, "lobe_oracle": vals}


def cancellation(parts) -> Dict[str, torch.Tensor]:
    """4 ulp32(sum |partial terms|) where the partial terms are of mixed sign, else 0; plus what the rounding of the chain rule's
    coefficients carries into the derivative where a Fresnel term cancels (AD.ed; 0 elsewhere)."""
    out = {}
    for k, s in parts["abs"].items():
        mixed = s > parts["signed"][k].abs() * (1.0 + 1e-9)
        out[k] = torch.where(mixed, 4.0 * ulp32(s), torch.zeros_like(s))
        if k in parts["carried"]:
            out[k] = out[k] + parts["carried"][k]
    return out


# ---- flags ----------------------------------------------------------------------------------------------------------------
def flags(head: str, inp) -> Dict[str, torch.Tensor]:
    """{"table": [n] rows whose diffuse lobe is excused, "bound": [n] rows excused altogether}."""
    n = inp["normal"].shape[0]
    dot = raw_dot(inp)
    table = torch.zeros(n, dtype=torch.bool)
    if head == "ggx" or is_composite(head):
        c = dot.clamp(COS_LO, COS_HI)
        a = inp["rough"].double().clamp(min=bounds(head)["rough"][0]).clamp(min=BOUNDS_GGX["rough"][0])
        for w in (c ** 0.25 * 100.0, (a / 4.0) ** 0.25 * 50.0):
            table |= ((w - torch.round(w)).abs() < TABLE_DELTA)[:, 0]
    bound = torch.zeros(n, dtype=torch.bool)
    reach = torch.maximum(4.0 * ulp32(dot), 2.0 * dot_delta(inp))
    uses_cos = head not in ("smooth_dielectric", "thin_dielectric")
    for b in (COS_LO, COS_HI):
        bound |= (((dot - b).abs() <= reach) & (dot != b) & uses_cos)[:, 0]
    for field, bb in bounds(head).items():
        x = inp[field].double()
        for b in bb:
            if b is not None:
                bound |= (((x - b).abs() <= 4.0 * ulp32(torch.tensor(b))) & (x != b)).any(-1)
    return {"table": table, "bound": bound}


def diffuse_touched(head: str, ups) -> bool:
    keys = ("rgb",) if is_composite(head) else ("diffuse_rgb", "rgb")
    return any(ups.get(k) is not None for k in keys)


def diffuse_outputs(head: str) -> tuple:
    return ("rgb",) if is_composite(head) else ("diffuse_rgb", "rgb")


# ---- the reference of a head: every stratum, every upstream configuration --------------------------------------------------------
def _grad_field_var(head: str):
    """oracle input -> scalar-space variable, for the gradients that are per-row scalars or albedo channels."""
    m = {"distance": "u", "env_light": "u", "kd": "kd", "ks": "ks", "rough": "rough", "m_eta": "m_eta", "m_k": "m_k", "d_eta": "d_eta"}
    return {f: m[f] for f in inputs_of(head) if f in m}


@functools.lru_cache(maxsize=None)
def reference(head: str):
    """reference_for on the concatenation of the head's strata (the rows are independent), with the strata's row slices."""
    names = strata_of(head)
    parts = [stratum_inputs(s) for s in names]
    inp = {k: torch.cat([p[k] for p in parts]) for k in FIELDS}
    slices, at = {}, 0
    for s, p in zip(names, parts):
        slices[s] = slice(at, at + p["normal"].shape[0])
        at += p["normal"].shape[0]
    return reference_for(head, inp, slices)


def reference_for(head: str, inp, slices=None, seed: int = 77):
    """Everything the two test files compare against, for the rows of `inp` (fp32, [n, .]): per upstream configuration the fp64
    and the fp32 CPU outputs and gradients and the yardstick y of every entry; the flags."""
    inp = dict(inp)
    inp["light"] = torch.tensor(LIGHT)
    at = inp["normal"].shape[0]
    slices = {"all": slice(0, at)} if slices is None else slices
    sc = scalars(head, inp)
    ref = {"inputs": inp, "slices": slices, "flags": flags(head, inp), "scalars": sc, "cfg": {}}
    absv, absn = inp["viewdir"].double().abs(), inp["normal"].double().abs()
    for cfg, ups in upstreams(head, at, seed).items():
        out64, g64 = evaluate(head, inp, ups, torch.float64, "fp32")
        out32, g32 = evaluate(head, inp, ups, torch.float32, None)
        base = scalar_entries(head, sc["x"], ups)
        sens = sensitivity(head, sc, ups)
        parts_ = partial_sums(head, sc, ups, base)
        canc = cancellation(parts_)
        y = {"out:" + k: 2.0 * ulp32(v) + sens["out:" + k] + parts_["value_lost"].get(k, 0.0) for k, v in out64.items()}
        for f, var in _grad_field_var(head).items():
            y["d:" + f] = 2.0 * ulp32(g64[f]) + sens["d:" + var] + canc["d:" + var]
        yc = sens["d:c"] + canc["d:c"]
        y["d:normal"] = 2.0 * ulp32(g64["normal"]) + absv * yc
        y["d:viewdir"] = 2.0 * ulp32(g64["viewdir"]) + absn * yc
        r = {"ups": ups, "out64": out64, "out32": out32, "g64": g64, "g32": g32, "y": y, "scalar": base, "partials": parts_}
        if head != "composite_env":
            r["t64"], r["t32"] = light_rows(head, out64, ups), light_rows(head, out32, ups)
            y["d:light"] = 2.0 * ulp32(r["t64"]) + sens["d:light"] + canc["d:light"]
        ref["cfg"][cfg] = r
    return ref


def dead(g32: torch.Tensor, g64: torch.Tensor) -> torch.Tensor:
    """Entries where the reference's gradient is exactly 0, in fp32 and in fp64: the kernel's must be exactly 0 too.  (An fp32
    gradient that only rounds to 0 -- a Fresnel term saturated at 1 -- is an ordinary entry, compared by ratio.)"""
    return (g32 == 0) & (g64 == 0)


def ratio(got: torch.Tensor, ref64: torch.Tensor, y: torch.Tensor, skip: torch.Tensor) -> float:
    """max_i |got_i - ref_i| / y_i over the entries not in `skip` ([n, w] bool, or [n] for whole rows); 0 when none is left."""
    err = (got.detach().cpu().double().reshape(ref64.shape) - ref64).abs() / y
    if skip.dim() == 1:
        skip = skip[:, None].expand_as(err)
    err = err[~skip]
    return float(err.max()) if err.numel() else 0.0


def light_tolerance(y_rows: torch.Tensor, t_rows: torch.Tensor, r_cpu: float) -> float:
    """sum_i 4 max(1, r_cpu) y_i + n 2^-24 sum_i |t_i|: the rows' own error plus that of an fp32 sum of n terms in any order."""
    n = t_rows.shape[0]
    return float(4.0 * max(1.0, r_cpu) * y_rows.sum() + n * 2.0 ** -24 * t_rows.abs().sum())


SMITH_STRATA = TABLE_STRATA + ("clamp_cos_low", "clamp_cos_high", "clamp_rough", "single")   # every stratum with a cosine or a roughness of its own


def smith_inputs(name: str):
    """(cos, alpha) [n] fp32 of the standalone smithG1 on a stratum: the clamped cosine and roughness as the GGX head forms them."""
    s = stratum_inputs(name)
    c = raw_dot(s).clamp(COS_LO, COS_HI).float()[:, 0]
    a = s["rough"].clamp(min=BOUNDS_GGX["rough"][0])[:, 0]
    return c.contiguous(), a.contiguous()


def smith_reference(name: str):
    """fp64 value, fp32 CPU value and yardstick (2 ulp32 + the effect of one ulp32 of either input) of smithG1 on a stratum."""
    c, a = smith_inputs(name)
    c64, a64 = c.double(), a.double()
    ref = R.smith_g1(c64, a64)
    y = 2.0 * ulp32(ref)
    for dc, da in ((ulp32(c64), 0.0), (-ulp32(c64), 0.0), (0.0, ulp32(a64)), (0.0, -ulp32(a64))):
        y = y + 0.5 * (R.smith_g1((c64 + dc).clamp(max=1.0), a64 + da) - ref).abs()
    return ref, R.smith_g1(c, a), y


def skip_mask(head: str, ref, cfg: str, key: str) -> torch.Tensor:
    """[n, w] bool over all rows of reference(head): the entries of "out:<key>" / "d:<input>" that are not compared by ratio --
    rows flagged on a bound, table-flagged rows where the entry contains the diffuse lobe, and dead gradient entries."""
    r, fl = ref["cfg"][cfg], ref["flags"]
    kind, name = key.split(":")
    shape = (r["out64"][name] if kind == "out" else (r["t64"] if name == "light" else r["g64"][name])).shape
    rows = fl["bound"].clone()
    if kind == "out":
        if name in diffuse_outputs(head):
            rows |= fl["table"]
    elif diffuse_touched(head, r["ups"]):
        rows |= fl["table"]
    skip = rows[:, None].expand(shape).clone()
    if kind == "d" and name != "light":
        skip |= dead(r["g32"][name], r["g64"][name])
    return skip


def entry_keys(head: str, ref, cfg: str) -> List[str]:
    r = ref["cfg"][cfg]
    return ["out:" + k for k in r["out64"]] + ["d:" + k for k in inputs_of(head) if k != "light"]


def r_cpu(head: str, ref, cfg: str, key: str, sl) -> float:
    """max |fp32 CPU oracle - fp64| / y over the compared entries of a stratum: how close an honest fp32 evaluation comes."""
    r = ref["cfg"][cfg]
    kind, name = key.split(":")
    if name == "light":
        return ratio(r["t32"][sl], r["t64"][sl], r["y"][key][sl], ref["flags"]["bound"][sl])
    lo, hi = (r["out32"][name], r["out64"][name]) if kind == "out" else (r["g32"][name], r["g64"][name])
    return ratio(lo[sl], hi[sl], r["y"][key][sl], skip_mask(head, ref, cfg, key)[sl])
