"""High-precision side of the per-operator NeuS kernel tests (tests/test_neus_oracle.py on the CPU,
tests/test_gpu_neus_kernels.py on the GPU).

oracle/neus_ref.py is dtype-generic: under torch.set_default_dtype(torch.float64) with fp64 inputs it evaluates the reference's
formulas in fp64.  `fp64` does that, `fp32_floor` measures how far an honest fp32 evaluation of the same formula on the same
inputs lies from it -- the yardstick of every tolerance in the GPU file -- and the flagging functions mark, from the fp64 side
only, the discrete decisions that no fp32 evaluation can be asked to reproduce.  The input builders live here so that both test
files see the same tensors.  Nothing here touches the GPU.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from oracle import neus_ref as N

DELTA_CDF = 1e-5     # inverse CDF: u this close to an interior CDF knot, or denom this close to the 1e-5 switch, is flagged
DELTA_RADIUS = 1e-6  # compositing: a mid point this close to |p| = 1 or |p| = 1.2 flags its ray
DENOM_SWITCH = 1e-5  # sample_pdf: denom < 1e-5 -> 1  (renderer.py:70)


# ---- running the oracle in a chosen precision ----------------------------------------------------------------------
def _cast(x, dtype):
    if torch.is_tensor(x) and x.is_floating_point():
        return x if x.dtype == dtype else x.detach().to(dtype)  # a tensor already in `dtype` keeps its autograd graph
    if isinstance(x, (list, tuple)):
        return type(x)(_cast(v, dtype) for v in x)
    if isinstance(x, dict):
        return {k: _cast(v, dtype) for k, v in x.items()}
    return x


def run_as(dtype, fn, *args, **kwargs):
    """fn(*args) with every floating tensor argument cast to `dtype` and `dtype` as torch's default (the oracle creates its
    constants with the default dtype); the default is restored whatever happens."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return fn(*_cast(args, dtype), **_cast(kwargs, dtype))
    finally:
        torch.set_default_dtype(prev)


def fp64(fn, *args, **kwargs):
    """An oracle function evaluated in fp64 from the given (fp32) inputs; returns fp64 tensors."""
    return run_as(torch.float64, fn, *args, **kwargs)


def _pairs(a, b, prefix=""):
    if torch.is_tensor(a):
        if a.is_floating_point():
            yield prefix, a, b
    elif isinstance(a, dict):
        for k in a:
            yield from _pairs(a[k], b[k], prefix + str(k))
    elif isinstance(a, (list, tuple)):
        for i, (x, y) in enumerate(zip(a, b)):
            yield from _pairs(x, y, "%s%d" % (prefix, i))


def fp32_deviation(fn, *args, **kwargs):
    """|fp32 evaluation - fp64 evaluation| of fn on the same inputs, entry by entry (fp64 tensors): a tensor for a tensor
    result, a dict for a dict result (floating outputs only)."""
    lo, hi = run_as(torch.float32, fn, *args, **kwargs), fp64(fn, *args, **kwargs)
    dev = {k: (x.double() - y.double()).abs() for k, x, y in _pairs(lo, hi)}
    return dev[""] if torch.is_tensor(hi) else dev


def fp32_floor(fn, *args, **kwargs):
    """Per output, the max abs deviation of the fp32 CPU evaluation of fn from its fp64 evaluation: the error of an honest fp32
    evaluation of the same formula on the same inputs (a float for a tensor result, a dict of floats for a dict result)."""
    dev = fp32_deviation(fn, *args, **kwargs)
    if torch.is_tensor(dev):
        return float(dev.max())
    return {k: float(v.max()) for k, v in dev.items()}


# ---- sample_pdf with a given u --------------------------------------------------------------------------------------
def pdf_cdf(weights: torch.Tensor) -> torch.Tensor:
    """renderer.py:47-50 in the dtype of `weights`: [n, m-1] section weights -> [n, m] CDF knots, cdf[:, 0] = 0."""
    w = weights + 1e-5
    cdf = torch.cumsum(w / torch.sum(w, -1, keepdim=True), -1)
    return torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)


def inverse_cdf(bins: torch.Tensor, weights: torch.Tensor, u: torch.Tensor) -> Dict[str, torch.Tensor]:
    """renderer.py:47-75 with u [n, k] given, in fp64: the samples and, per sample, the section the search chose (below, above),
    its raw CDF width `denom` (before the 1e-5 switch) and the CDF knots."""
    bins, weights, u = bins.double(), weights.double(), u.double().contiguous()
    cdf = pdf_cdf(weights)
    inds = torch.searchsorted(cdf, u, right=True)
    below = (inds - 1).clamp(min=0)
    above = inds.clamp(max=cdf.shape[-1] - 1)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = c1 - c0
    used = torch.where(denom < DENOM_SWITCH, torch.ones_like(denom), denom)
    t = (u - c0) / used
    return {"samples": b0 + t * (b1 - b0), "cdf": cdf, "below": below, "above": above, "denom": denom, "denom_used": used,
            "width": b1 - b0}


def sample_pdf_u(bins: torch.Tensor, weights: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """The stochastic branch of sample_pdf with its uniform numbers given: fp64 samples [n, k]."""
    return inverse_cdf(bins, weights, u)["samples"]


def det_u(n: int, k: int) -> torch.Tensor:
    """The u of sample_pdf(det=True) as the fp64 evaluation of the oracle forms it: linspace(0.5/k, 1 - 0.5/k, k) per row."""
    return torch.linspace(0.0 + 0.5 / k, 1.0 - 0.5 / k, steps=k, dtype=torch.float64).expand(n, k).contiguous()


def flag_inverse_cdf(bins: torch.Tensor, weights: torch.Tensor, u: torch.Tensor, delta: float = DELTA_CDF) -> torch.Tensor:
    """[n, k] bool, from the fp64 side only: the entries whose value fp32 cannot be asked to reproduce.  The inverse CDF is
    continuous in u, but its slope changes from one section to the next by orders of magnitude, and at denom = 1e-5 the
    reference switches the divisor to 1: an entry is flagged when u lies within `delta` of a knot BETWEEN two sections (an fp32
    CDF may put it into the neighbour) or its section's denom lies within `delta` of the switch.  The end knots are no such
    decision: cdf[0] is 0 in every precision, beyond the last knot there is no section, and a last section narrow enough to
    make u ~ 1 jump is flagged by its denom."""
    r = inverse_cdf(bins, weights, u)
    cdf, ud = r["cdf"], u.double()
    m = cdf.shape[-1]
    near_knot = torch.zeros_like(ud, dtype=torch.bool)
    if m > 2:
        inner = cdf[:, 1:m - 1].contiguous()
        pos = torch.searchsorted(inner, ud.contiguous(), right=True)
        lo = torch.gather(inner, 1, (pos - 1).clamp(min=0))
        hi = torch.gather(inner, 1, pos.clamp(max=m - 3))
        near_knot = ((ud - lo).abs() < delta) | ((ud - hi).abs() < delta)
    return near_knot | ((r["denom"] - DENOM_SWITCH).abs() < delta)


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 at the magnitude of x (fp64 tensor): 2^(floor(log2 |x|) - 23), the smallest normal's below that."""
    a = x.double().abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23.0)


def inverse_cdf_bound(bins: torch.Tensor, weights: torch.Tensor, u: torch.Tensor, weights32: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per entry, what an fp32 CDF costs an inverse-CDF sample, to first order: dcdf * (b_above - b_below) / denom + 2 ulp(b),
    with dcdf the measured max deviation of the row's fp32 CDF (torch, CPU) from its fp64 CDF.  `weights32` are the section
    weights as the fp32 evaluation has them when they are themselves computed (up_sample); else the fp32 inputs."""
    r = inverse_cdf(bins, weights, u)
    c32 = pdf_cdf((weights if weights32 is None else weights32).float())
    dcdf = (c32.double() - r["cdf"]).abs().max(dim=-1, keepdim=True)[0]
    return dcdf * r["width"] / r["denom_used"] + 2.0 * ulp32(r["samples"])


def up_sample_sections(rays_o, rays_d, z_vals, sdf, inv_s: float, dtype) -> torch.Tensor:
    """The section weights NeuSRenderer.up_sample hands to sample_pdf, as oracle.neus_ref.up_sample computes them in `dtype`
    (captured from the oracle's own call, not restated)."""
    seen = {}
    real = N.sample_pdf

    def spy(bins, weights, n_samples, det=True):
        seen["w"] = weights.detach().clone()
        return real(bins, weights, n_samples, det=det)

    N.sample_pdf = spy
    try:
        run_as(dtype, N.up_sample, rays_o, rays_d, z_vals, sdf, 1, inv_s)
    finally:
        N.sample_pdf = real
    return seen["w"]


# ---- compositing ------------------------------------------------------------------------------------------------------
def flag_composite_rays(pts: torch.Tensor, n: int, m: int, delta: float = DELTA_RADIUS) -> torch.Tensor:
    """[n] bool: rays with a mid point whose norm (fp64, from the fp32 point) lies within `delta` of the inside-sphere radius 1
    or of the eikonal statistic's radius 1.2 -- an fp32 norm may fall on the other side."""
    r = pts.double().reshape(n, m, 3).norm(dim=-1)
    return (((r - 1.0).abs() < delta) | ((r - 1.2).abs() < delta)).any(dim=-1)


def background_alpha(bg_density: torch.Tensor, bg_dists: torch.Tensor) -> torch.Tensor:
    """renderer.py:174: 1 - exp(-softplus(density) * dists), [n, mo], in the dtype of the arguments."""
    return 1.0 - torch.exp(-torch.nn.functional.softplus(bg_density.reshape(bg_dists.shape)) * bg_dists)


def composite_with_density(sdf, grad, color, inv_s, bg_density, bg_color, dists, pts, dirs, bg_dists, background_rgb, cos_anneal_ratio):
    """oracle.neus_ref.composite behind the argument list of iron_amd.autograd.NeusCompositeFn: the background enters as the NeRF
    density (alpha by `background_alpha`), weight_sum / weight_max are added as render() forms them."""
    n, m = dists.shape
    bga = bgc = None
    if bg_density is not None:
        bga = background_alpha(bg_density, bg_dists)
        bgc = bg_color.reshape(n, bg_dists.shape[1], 3)
    out = N.composite(sdf.reshape(-1, 1), grad.reshape(-1, 3), color.reshape(n, m, 3), dists, pts.reshape(-1, 3), dirs.reshape(-1, 3),
                      inv_s, bga, bgc, None if background_rgb is None else background_rgb.reshape(1, 3), cos_anneal_ratio)
    w = out["weights"]
    return {"color": out["color"], "weights": w, "weight_sum": w.sum(dim=-1, keepdim=True), "weight_max": w.max(dim=-1, keepdim=True)[0],
            "cdf": out["cdf"], "gradient_error": out["gradient_error"], "inside_sphere": out["inside_sphere"]}


COMPOSITE_ARGS = ("sdf", "grad", "color", "inv_s", "bg_density", "bg_color", "dists", "pts", "dirs", "bg_dists", "background_rgb")
TOGGLE_ROWS = (3, 64, 129)                         # rays whose inside_sphere flips many times
ZERO_NORMALS = ((2, 40), (70, 55), (129, 47))      # (ray, sample) with an exactly zero normal; ray 129 is in the last partial wave
BIG_DENSITY = ((0, 0, 20.5), (5, 2, 25.0), (129, 1, 40.0), (64, 4, 21.0), (17, 3, 88.0), (1, 0, 20.0))  # (ray, sample, density)


def composite_inputs(n: int, m: int, mo: int, seed: int = 41, zero_normals: bool = False) -> Dict[str, torch.Tensor]:
    """fp32 CPU inputs of the compositing kernels: rays from (0, 0, -2.3) through a noisy sphere SDF of radius 0.6, m section
    mid points per ray running from beyond |p| = 1.2 through the unit sphere and out beyond 1.2 again, mo - m further outside
    samples; rows TOGGLE_ROWS have every fifth mid point pushed across |p| = 1; the background density is 3 randn with
    BIG_DENSITY beyond the softplus threshold.  Normals are kept off the relu kinks of iter_cos (|tc| > 1e-3, |1 - tc| > 2e-3);
    with zero_normals, ZERO_NORMALS are exactly zero.  mo == m gives the same without the extra samples."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([[0.0, 0.0, -2.3]]).expand(n, 3).contiguous()
    d = (torch.randn(n, 3, generator=gen) * 0.1).clamp(-0.2, 0.2) * torch.tensor([1.0, 1.0, 0.0]) + torch.tensor([0.0, 0.0, 1.0])
    d = torch.nn.functional.normalize(d, dim=-1)
    zi = torch.sort(torch.rand(n, m, generator=gen) * 3.1 + 0.8, dim=-1)[0]
    z = torch.cat([zi, torch.sort(torch.rand(n, mo - m, generator=gen) * 4.0 + 3.95, dim=-1)[0]], dim=-1)
    tail = torch.full((n, 1), 2.0 / 64)
    dists = torch.cat([zi[:, 1:] - zi[:, :-1], tail], dim=-1)
    bg_dists = torch.cat([z[:, 1:] - z[:, :-1], tail], dim=-1)
    pts = o[:, None, :] + d[:, None, :] * (zi + dists * 0.5)[..., None]
    for r in TOGGLE_ROWS:
        if r < n:
            rad = pts[r, ::5].norm(dim=-1, keepdim=True)
            pts[r, ::5] = pts[r, ::5] / rad * torch.where(rad < 1.0, 1.05, 0.95)
    for _ in range(8):  # keep every mid point clear of the two radii (decided in fp64): no ray is flagged, by construction
        rad = pts.double().norm(dim=-1)
        close = ((rad - 1.0).abs() < 4 * DELTA_RADIUS) | ((rad - 1.2).abs() < 4 * DELTA_RADIUS)
        if not bool(close.any()):
            break
        pts[close] = pts[close] * 1.0001
    pts = pts.reshape(-1, 3).contiguous()
    dirs = d[:, None, :].expand(n, m, 3).reshape(-1, 3).contiguous()
    sdf = pts.norm(dim=-1, keepdim=True) - 0.6 + 0.01 * torch.randn(n * m, 1, generator=gen)
    grad = torch.nn.functional.normalize(pts, dim=-1) * (1 + 0.1 * torch.randn(n * m, 1, generator=gen)) + 0.05 * torch.randn(n * m, 3, generator=gen)
    for _ in range(16):  # resample the normals that sit on a relu kink of iter_cos
        tc = (dirs.double() * grad.double()).sum(-1)
        bad = (tc.abs() < 2e-3) | ((1.0 - tc).abs() < 4e-3)
        if not bool(bad.any()):
            break
        grad[bad] = grad[bad] + 0.05 * torch.randn(int(bad.sum()), 3, generator=gen)
    color = torch.rand(n * m, 3, generator=gen)
    bg_density = 3.0 * torch.randn(n * mo, 1, generator=gen)
    for r, j, v in BIG_DENSITY:
        if r < n and j < mo:
            bg_density[r * mo + j, 0] = v
    bg_color = 0.5 * torch.randn(n * mo, 3, generator=gen)
    if zero_normals:
        for r, j in ZERO_NORMALS:
            if r < n and j < m:
                grad[r * m + j] = 0.0
    return {"sdf": sdf, "grad": grad, "color": color, "inv_s": torch.tensor(37.0), "bg_density": bg_density, "bg_color": bg_color,
            "dists": dists, "pts": pts, "dirs": dirs, "bg_dists": bg_dists, "background_rgb": torch.tensor([0.2, 0.5, 0.9]),
            "z": z, "rays_o": o, "rays_d": d}


def composite_args(inp: Dict[str, torch.Tensor], inv_s: float, with_bg: bool, with_rgb: bool) -> list:
    """The positional arguments of composite_with_density / NeusCompositeFn.apply (without cos_anneal_ratio) from composite_inputs."""
    a = dict(inp)
    a["inv_s"] = torch.tensor(float(inv_s))
    if not with_bg:
        a["bg_density"] = a["bg_color"] = a["bg_dists"] = None
    if not with_rgb:
        a["background_rgb"] = None
    return [a[k] for k in COMPOSITE_ARGS]


COMPOSITE_SHAPES = ((130, 192, 192, False), (130, 160, 192, True))  # (n, m, mo, with_bg): the per-thread arrays' bound, with and without background


# ---- inverse-CDF inputs ------------------------------------------------------------------------------------------------
PDF_ROW_ZERO, PDF_ROW_HEAD_ZERO = 7, 128  # an all-zero row; a row whose first 100 sections are zero (in the last partial wave)


def pdf_inputs(n: int = 130, n_bins: int = 192, seed: int = 11):
    """bins [n, n_bins] ascending, weights [n, n_bins-1] = rand**6 (ragged: most of the mass in a few sections).  The first
    and the last section of a row carry a weight of 0.2 .. 1: a thinner one has denom < 2e-5 and would flag the entries with
    u = 0 and u = 1 - 2^-24 that the GPU test places there on purpose (the interior keeps its thin sections)."""
    gen = torch.Generator().manual_seed(seed)
    bins = torch.sort(torch.rand(n, n_bins, generator=gen) * 2.0 + 1.5, dim=-1)[0]
    w = torch.rand(n, n_bins - 1, generator=gen) ** 6
    ends = 0.2 + 0.8 * torch.rand(n, 2, generator=gen)
    w[:, 0], w[:, -1] = ends[:, 0], ends[:, 1]
    if n > PDF_ROW_ZERO:
        w[PDF_ROW_ZERO] = 0.0
    if n > PDF_ROW_HEAD_ZERO:
        w[PDF_ROW_HEAD_ZERO, :min(100, n_bins - 1)] = 0.0
    return bins, w


def pdf_given_u(n: int, k: int, seed: int = 12) -> torch.Tensor:
    """Uniform numbers [n, k] with, where k allows, columns of exactly 0, 1 - 2^-24 (the largest fp32 below 1) and 0.5."""
    gen = torch.Generator().manual_seed(seed + k)
    u = torch.rand(n, k, generator=gen)
    if k < 3:
        return u
    for col, v in zip(range(0, k, max(k // 3, 1)), (0.0, 1.0 - 2.0 ** -24, 0.5)):
        u[:, col] = v
    return u


PDF_K = (1, 16, 64)
PDF_CASES = tuple((130, nb, k) for nb in (192, 2) for k in PDF_K) + ((1, 192, 16),)  # (rows, bins, samples per row)
UP_SAMPLE_M = (2, 64, 192)
UP_SAMPLE_INV_S = (64.0, 512.0, 4096.0)


def up_sample_inputs(n: int, m: int, seed: int = 5):
    """rays through the unit sphere and m ascending depths with a noisy sphere SDF (radius 0.6) on them; no sample lies within
    DELTA_RADIUS of |p| = 1, where up_sample's `inside_sphere` decision could differ between precisions."""
    gen = torch.Generator().manual_seed(seed + m)
    o = torch.randn(n, 3, generator=gen) * 0.3
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    o = o - 2.5 * d
    z = torch.sort(torch.rand(n, m, generator=gen) * 2.4 + 1.3, dim=-1)[0]
    for _ in range(8):
        rad = (o.double()[:, None, :] + d.double()[:, None, :] * z.double()[..., None]).norm(dim=-1)
        close = (rad - 1.0).abs() < 4 * DELTA_RADIUS
        if not bool(close.any()):
            break
        z = torch.sort(torch.where(close, z + 1e-4, z), dim=-1)[0]
    sdf = (o[:, None, :] + d[:, None, :] * z[..., None]).norm(dim=-1) - 0.6 + 0.02 * torch.randn(n, m, generator=gen)
    return o, d, z, sdf


def up_sample_radius_clear(o, d, z) -> bool:
    rad = (o.double()[:, None, :] + d.double()[:, None, :] * z.double()[..., None]).norm(dim=-1)
    return not bool(((rad - 1.0).abs() < DELTA_RADIUS).any())


# ---- placement --------------------------------------------------------------------------------------------------------
def placement_inputs(n: int, m: int, seed: int = 3):
    """Rays whose origin and direction agree in sign per component and ascending positive depths: o + d t then adds terms of one
    sign, so the fp32 result is within 2 ulp OF ITS OWN magnitude (a cancelling sum is only within an ulp of its larger term).
    Origins lie inside the unit ball, so the first mid points have |p| < 1 -- the clip of the outside parametrisation is
    active -- and the later ones run far outside."""
    gen = torch.Generator().manual_seed(seed + m)
    sign = torch.where(torch.rand(n, 3, generator=gen) < 0.5, -1.0, 1.0)
    o = sign * (0.02 + 0.3 * torch.rand(n, 3, generator=gen))
    d = sign * torch.nn.functional.normalize(0.1 + torch.rand(n, 3, generator=gen), dim=-1)
    near = 0.05 + 0.5 * torch.rand(n, generator=gen)
    far = near + 1.0 + 2.0 * torch.rand(n, generator=gen)
    z = torch.sort(torch.rand(n, m, generator=gen) * 3.0 + 0.05, dim=-1)[0]
    return o.contiguous(), d.contiguous(), near, far, z
