"""The per-ray kernels of the stage-1 NeuS renderer (csrc/neus.hip, k_neus_composite_back of csrc/train.hip), one operator at a
time against oracle/neus_ref.py evaluated in fp64 (tests/_neus_oracle.py), on tiny tensors: n = 130 rays (two full waves plus
two lanes, three blocks) and n = 1, rows of 2, 64, 160 and 192 = the bound of the per-thread arrays.

Every tolerance is a multiple of the error of an honest fp32 evaluation of the same formula on the same inputs (torch on the
CPU against fp64), measured in the test, never a guessed figure.  The inputs and the flags of the decisions no fp32 evaluation
can be asked to reproduce come from _neus_oracle.py; tests/test_neus_oracle.py checks their caps and margins on the CPU.
Lines starting with "neus-k" carry the measured figures (DESIGN.md keeps a table of them)."""
import ctypes as C
import functools

import pytest
import torch

import _neus_oracle as O
from oracle import iron_ref as R
from oracle import neus_ref as N

from _util import cpu_sd, golden, rel_l2, t

pytestmark = pytest.mark.gpu

SAMPLE_DIST = 2.0 / 64
IRON_ERR_BAD_ARG = -1  # include/iron_hip.h


def _L():
    from iron_amd import _lib
    return _lib


def cu(x):
    return x.cuda().contiguous() if torch.is_tensor(x) else x


def _ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at the magnitude of the reference."""
    return (got.detach().cpu().double().reshape(ref64.shape) - ref64).abs() / O.ulp32(ref64)


# ---- (a) placement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [130, 1])
def test_placement_linspace_outside_z_points(n):
    """iron_neus_linspace / _outside_z / _points against the same expressions in fp64 from the same fp32 inputs, 2 ulp of the
    result per entry.  Every expression here adds terms of one sign (O.placement_inputs): a rounding of (far - near) reaches the
    result as at most 1 ulp of the product, which is below the result; the product and the sum round once each -- 2 ulp."""
    L, lib = _L(), _L().load()
    o, d, near, far, z = O.placement_inputs(n, 64)
    dev = torch.device("cuda", 0)
    st = L.stream_ptr(dev)
    lin = torch.linspace(0.0, 1.0, 64)
    rev = torch.flip(torch.linspace(1e-3, 1.0 - 1.0 / 33.0, 32), dims=[-1]).contiguous()
    g = {k: cu(v) for k, v in dict(o=o, d=d, near=near, far=far, z=z, lin=lin, rev=rev).items()}
    zl = torch.full((n, 64), -7.0, device=dev)
    L.check(lib.iron_neus_linspace(g["near"].data_ptr(), g["far"].data_ptr(), g["lin"].data_ptr(), n, 64, zl.data_ptr(), st))
    zo = torch.full((n, 32), -7.0, device=dev)
    L.check(lib.iron_neus_outside_z(g["far"].data_ptr(), g["rev"].data_ptr(), n, 32, 1.0 / 64, zo.data_ptr(), st))
    pts = torch.full((n * 64, 3), -7.0, device=dev)
    L.check(lib.iron_neus_points(g["o"].data_ptr(), g["d"].data_ptr(), g["z"].data_ptr(), n, 64, pts.data_ptr(), st))
    ref_l = near.double()[:, None] + (far.double() - near.double())[:, None] * lin.double()[None, :]
    ref_o = far.double()[:, None] / rev.double()[None, :] + 1.0 / 64
    ref_p = (o.double()[:, None, :] + d.double()[:, None, :] * z.double()[..., None]).reshape(-1, 3)
    worst = {"linspace": float(_ulps(zl, ref_l).max()), "outside_z": float(_ulps(zo, ref_o).max()), "points": float(_ulps(pts, ref_p).max())}
    print("neus-k (a) n=%d max ulp" % n, " ".join("%s=%.2f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 2.0, worst


@pytest.mark.parametrize("n,m", [(130, 33), (1, 2)])
def test_placement_mid_points_both_parametrisations(n, m):
    """iron_neus_mid_points: section lengths with the sample_dist tail, mid points, copied directions, and the outside
    parametrisation [p / r, 1 / r] with r = clip(|p|, 1, 1e10), 2 ulp of the result per entry.  Each stage is held against fp64
    from the fp32 values the stage before it wrote (the mid point from the kernel's dists, the parametrisation from the kernel's
    mid point, which the outside = 0 launch of the same kernel returns): the bound is one of a few roundings, not of a chain."""
    from iron_amd.renderer import NeuSRenderer
    o, d, _, _, z = O.placement_inputs(n, m)
    with torch.cuda.device(0):
        dists, pts3, dirs = NeuSRenderer._mid_points(cu(o), cu(d), cu(z), SAMPLE_DIST, False)
        dists1, pts4, dirs1 = NeuSRenderer._mid_points(cu(o), cu(d), cu(z), SAMPLE_DIST, True)
    assert dists.shape == (n, m) and pts3.shape == (n * m, 3) and pts4.shape == (n * m, 4)
    assert torch.equal(dists, dists1) and torch.equal(dirs, dirs1)
    assert torch.equal(dirs.cpu(), d[:, None, :].expand(n, m, 3).reshape(-1, 3))
    ref_d = torch.cat([z.double()[:, 1:] - z.double()[:, :-1], torch.full((n, 1), SAMPLE_DIST, dtype=torch.float64)], dim=-1)
    mid = z.double() + dists.cpu().double() * 0.5
    ref_p = (o.double()[:, None, :] + d.double()[:, None, :] * mid[..., None]).reshape(-1, 3)
    p = pts3.cpu().double()
    rad = p.norm(dim=-1, keepdim=True)
    r = rad.clip(1.0, 1e10)
    ref_4 = torch.cat([p / r, 1.0 / r], dim=-1)
    clipped = rad[:, 0] < 1.0 - 1e-6  # well inside the unit ball: r is exactly 1, the point comes through unchanged
    if n > 1:
        assert bool(clipped.any()) and bool((rad > 1.0 + 1e-6).any())  # the clip is active for some mid points and not for others
    assert bool((pts4.cpu()[clipped, 3] == 1.0).all()) and torch.equal(pts4.cpu()[clipped, :3], pts3.cpu()[clipped])
    worst = {"dists": float(_ulps(dists, ref_d).max()), "mid": float(_ulps(pts3, ref_p).max()), "outside": float(_ulps(pts4, ref_4).max())}
    print("neus-k (a) mid_points n=%d m=%d max ulp" % (n, m), " ".join("%s=%.2f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 2.0, worst


def _composite_fn(args, ca):
    from iron_amd.autograd import NeusCompositeFn
    out = NeusCompositeFn.apply(*[cu(a) for a in args], float(ca))
    return dict(zip(("color", "weights", "weight_sum", "gradient_error", "cdf", "inside_sphere", "weight_max"), out))


def test_need_background_is_the_complement_of_inside_sphere():
    """iron_neus_need_background == (|p| >= 1) in fp64 for the inside samples (no mid point of these inputs lies within 1e-6 of
    the sphere), 1 for every outside column, and 1 - inside_sphere as iron_neus_composite writes it for the same points."""
    L = _L()
    n, m, mo, _ = O.COMPOSITE_SHAPES[1]
    inp = O.composite_inputs(n, m, mo)
    assert int(O.flag_composite_rays(inp["pts"], n, m).sum()) == 0
    dev = torch.device("cuda", 0)
    pts = cu(inp["pts"])
    need = torch.full((n, mo), 9, dtype=torch.uint8, device=dev)
    L.check(L.load().iron_neus_need_background(pts.data_ptr(), n, m, mo, need.data_ptr(), L.stream_ptr(dev)))
    need = need.cpu()
    ref = (inp["pts"].double().reshape(n, m, 3).norm(dim=-1) >= 1.0).to(torch.uint8)
    assert torch.equal(need[:, :m], ref) and bool((need[:, m:] == 1).all())
    assert 0.2 < float(ref.double().mean()) < 0.8
    with torch.no_grad():
        out = _composite_fn(O.composite_args(inp, 64.0, True, False), 0.3)
    assert torch.equal(1.0 - out["inside_sphere"].cpu(), need[:, :m].float())


# ---- rows beyond the per-thread arrays ----------------------------------------------------------------------------------
def test_rows_of_193_are_refused_before_any_launch():
    """kMaxSamples = kNeusMax = 192: the extern "C" wrappers answer IRON_ERR_BAD_ARG from their argument checks, which precede
    the launch, so nothing is written."""
    from iron_amd.renderer import NeuSRenderer, sample_pdf
    L, lib = _L(), _L().load()
    dev = torch.device("cuda", 0)
    n, big = 3, 193
    o, d, z, sdf = O.up_sample_inputs(n, big)
    r = NeuSRenderer(None, None, None, None, 64, 64, 0, 4, 0.0)
    with pytest.raises(L.IronError):
        r.up_sample(cu(o), cu(d), cu(z), cu(sdf), 16, 64.0)
    bins, w = O.pdf_inputs(n, big)
    with pytest.raises(L.IronError):
        sample_pdf(cu(bins), cu(w), 16, det=True)
    out = torch.full((n, 16), -7.0, device=dev)
    gb, gw = cu(bins), cu(w)
    assert lib.iron_neus_sample_pdf(gb.data_ptr(), gw.data_ptr(), None, n, big, 16, out.data_ptr(), L.stream_ptr(dev)) == IRON_ERR_BAD_ARG
    nz = torch.full((n, 16), -7.0, device=dev)
    go, gd, gz, gs = cu(o), cu(d), cu(z), cu(sdf)
    assert lib.iron_neus_up_sample(go.data_ptr(), gd.data_ptr(), gz.data_ptr(), gs.data_ptr(), n, big, 16, 64.0, nz.data_ptr(),
                                   L.stream_ptr(dev)) == IRON_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((nz == -7.0).all())
    with torch.no_grad():
        with pytest.raises(L.IronError):  # the inside row
            _composite_fn(O.composite_args(O.composite_inputs(n, big, big), 64.0, False, False), 0.3)
        with pytest.raises(L.IronError):  # the row with the outside samples
            _composite_fn(O.composite_args(O.composite_inputs(n, 160, big), 64.0, True, False), 0.3)
        inp = O.composite_inputs(n, 160, big)
        with pytest.raises(L.IronError):
            _composite_direct(inp, 64.0, 0.3, False, bg_alpha=O.background_alpha(inp["bg_density"], inp["bg_dists"]))
    a, g = L.iron_neus_composite_args(), L.iron_neus_composite_grads()
    a.n, a.m, a.mo = n, big, big
    with pytest.raises(L.IronError):
        L.check_train(L.load_train().iron_neus_composite_backward(C.byref(a), C.byref(g), L.stream_ptr(dev)))
    # 192 itself is accepted
    o, d, z, sdf = O.up_sample_inputs(n, 192)
    assert r.up_sample(cu(o), cu(d), cu(z), cu(sdf), 4, 64.0).shape == (n, 4)


# ---- (b) sample_pdf, (c) up_sample ----------------------------------------------------------------------------------------
def _check_inverse_cdf(tag, got, bins, w64, u64, dev_entry, w32=None, monotone=True):
    """On unflagged entries |got - ref64| <= 4 x max(the entry's fp32-oracle deviation, dcdf (b_above - b_below) / denom +
    2 ulp): the second term is what the measured fp32-vs-fp64 CDF deviation of the row costs the entry to first order, and keeps
    the yardstick from vanishing where the fp32 oracle happens to hit the fp64 value.  The factor 4 covers the kernel's
    sequential sums against torch's pairwise ones (the CDF enters an entry through cdf_below and through denom).  On all
    entries: inside [bins[0], bins[-1]], and non-decreasing along k where u is."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), tag
    r = O.inverse_cdf(bins, w64, u64)
    flag = O.flag_inverse_cdf(bins, w64, u64)
    assert float(flag.double().mean()) <= 0.01, (tag, float(flag.double().mean()))
    assert bool((got >= bins[:, :1]).all()) and bool((got <= bins[:, -1:]).all()), tag
    if monotone:
        assert bool((got[:, 1:] >= got[:, :-1]).all()), tag
    yard = O.inverse_cdf_bound(bins, w64, u64, weights32=w32)
    if dev_entry is not None:
        yard = torch.maximum(yard, dev_entry)
    err = (got.double() - r["samples"]).abs()
    ratio = torch.where(flag, torch.zeros_like(err), err / yard)
    floor = float(dev_entry[~flag].max()) if dev_entry is not None else float("nan")
    print("neus-k %s: fp32 floor %.2e, kernel max err %.2e (unflagged), worst err/yardstick %.2f, flagged %d / %d"
          % (tag, floor, float(err[~flag].max()), float(ratio.max()), int(flag.sum()), flag.numel()))
    assert float(ratio.max()) <= 4.0, (tag, float(ratio.max()))


def _sample_pdf_kernel(bins, w, u, k):
    L = _L()
    dev = torch.device("cuda", 0)
    gb, gw, gu = cu(bins), cu(w), cu(u)
    out = torch.full((bins.shape[0], k), -7.0, device=dev)
    L.check(L.load().iron_neus_sample_pdf(gb.data_ptr(), gw.data_ptr(), L.ptr(gu), bins.shape[0], bins.shape[1], k, out.data_ptr(),
                                          L.stream_ptr(dev)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,n_bins,k", O.PDF_CASES)
def test_sample_pdf_vs_fp64(n, n_bins, k):
    """iron_neus_sample_pdf, det=True through iron_amd.renderer.sample_pdf and with a given u driven directly (columns of
    exactly 0, 1 - 2^-24 and 0.5 where k >= 3), on rand**6 weights with an all-zero row and a row whose first 100 sections are
    zero."""
    from iron_amd.renderer import sample_pdf
    bins, w = O.pdf_inputs(n, n_bins)
    tag = "(b) sample_pdf n=%d bins=%d k=%d" % (n, n_bins, k)
    got = sample_pdf(cu(bins), cu(w), k, det=True)
    assert got.shape == (n, k)
    _check_inverse_cdf(tag + " det", got, bins, w.double(), O.det_u(n, k), O.fp32_deviation(N.sample_pdf, bins, w, k, det=True))
    u = O.pdf_given_u(n, k)
    _check_inverse_cdf(tag + " given u", _sample_pdf_kernel(bins, w, u, k), bins, w.double(), u.double(), None, monotone=False)
    order = torch.sort(u, dim=-1)[0]  # an ascending u gives ascending samples
    assert bool((_sample_pdf_kernel(bins, w, order, k).diff(dim=-1) >= 0).all())


@pytest.mark.parametrize("inv_s", O.UP_SAMPLE_INV_S)
@pytest.mark.parametrize("m", O.UP_SAMPLE_M)
def test_up_sample_vs_fp64(m, inv_s):
    """iron_neus_up_sample (section weights from the sdf at sharpness inv_s, then the inverse CDF at the regular u) by the rule
    of test_sample_pdf_vs_fp64; the row's CDF deviation is measured between the oracle's own fp32 and fp64 section weights."""
    from iron_amd.renderer import NeuSRenderer
    n = 130
    o, d, z, sdf = O.up_sample_inputs(n, m)
    assert O.up_sample_radius_clear(o, d, z)
    r = NeuSRenderer(None, None, None, None, 64, 64, 0, 4, 0.0)
    w64 = O.up_sample_sections(o, d, z, sdf, inv_s, torch.float64)
    w32 = O.up_sample_sections(o, d, z, sdf, inv_s, torch.float32)
    for k in O.PDF_K:
        got = r.up_sample(cu(o), cu(d), cu(z), cu(sdf), k, inv_s)
        assert got.shape == (n, k)
        ref = O.fp64(N.up_sample, o, d, z, sdf, k, inv_s)
        assert torch.equal(ref, O.sample_pdf_u(z, w64, O.det_u(n, k)))
        _check_inverse_cdf("(c) up_sample m=%d inv_s=%g k=%d" % (m, inv_s, k), got, z, w64, O.det_u(n, k),
                           O.fp32_deviation(N.up_sample, o, d, z, sdf, k, inv_s), w32=w32)


# ---- (d) compositing forward ------------------------------------------------------------------------------------------------
VALUE_KEYS = ("color", "weights", "weight_sum", "weight_max", "cdf", "gradient_error")


def _check_composite(tag, got, args, ca, ref=None):
    """|got - ref64| <= 4 x fp32 floor + 1e-7 per output, inside_sphere exactly equal.  The floor is torch's fp32 evaluation of
    the same formula; the kernel differs from it in the order of its sums (a sequential transmittance scan against cumprod, a
    per-ray running sum and wave reduction against pairwise sums) and in expf against torch's exp / sigmoid (about 1 ulp each,
    entering through alpha like the floor's own roundings): a few times the floor, never an order of magnitude."""
    ref = O.fp64(O.composite_with_density, *args, ca) if ref is None else ref
    floor = O.fp32_floor(O.composite_with_density, *args, ca)
    fails, parts = [], []
    for k in VALUE_KEYS:
        g = got[k].detach().cpu().double().reshape(ref[k].shape)
        assert bool(torch.isfinite(g).all()), (tag, k)
        err = float((g - ref[k]).abs().max())
        tol = 4.0 * floor[k] + 1e-7
        parts.append("%s %.1e/%.1e" % (k, err, floor[k]))
        if err > tol:
            fails.append((k, err, tol))
    print("neus-k %s: kernel err / fp32 floor: %s" % (tag, ", ".join(parts)))
    assert torch.equal(got["inside_sphere"].detach().cpu().double(), ref["inside_sphere"].double()), tag
    return fails, {k: (float((got[k].detach().cpu().double().reshape(ref[k].shape) - ref[k]).abs().max()), floor[k]) for k in VALUE_KEYS}


@pytest.mark.parametrize("with_rgb", [False, True])
@pytest.mark.parametrize("n,m,mo,with_bg", O.COMPOSITE_SHAPES)
def test_composite_forward_vs_fp64(n, m, mo, with_bg, with_rgb):
    """iron_neus_composite through NeusCompositeFn (no grad) over cos_anneal_ratio x inv_s, without background at m = 192 and
    with the background density at m = 160, mo = 192, each with and without background_rgb; then one ray alone."""
    inp = O.composite_inputs(n, m, mo)
    assert int(O.flag_composite_rays(inp["pts"], n, m).sum()) == 0
    fails, worst = [], {}
    with torch.no_grad():
        for inv_s in (37.0, 512.0, 2048.0):
            for ca in (0.0, 0.3, 1.0):
                args = O.composite_args(inp, inv_s, with_bg, with_rgb)
                got = _composite_fn(args, ca)
                assert got["weights"].shape == (n, mo if with_bg else m) and got["cdf"].shape == (n, m)
                f, figures = _check_composite("(d) m=%d mo=%d bg=%d rgb=%d inv_s=%g ca=%g" % (m, mo, with_bg, with_rgb, inv_s, ca), got, args, ca)
                fails += [(inv_s, ca) + x for x in f]
                for k, (err, floor) in figures.items():
                    if err / floor > worst.get(k, (0.0, 0.0, 0.0))[2]:
                        worst[k] = (floor, err, err / floor)
        one = O.composite_inputs(1, m, mo)
        args = O.composite_args(one, 512.0, with_bg, with_rgb)
        f, _ = _check_composite("(d) one ray m=%d bg=%d rgb=%d" % (m, with_bg, with_rgb), _composite_fn(args, 0.3), args, 0.3)
        fails += f
    print("neus-k (d) summary m=%d bg=%d rgb=%d worst ratio per output (floor, err, ratio): %s"
          % (m, with_bg, with_rgb, ", ".join("%s %.1e %.1e %.2f" % ((k,) + v) for k, v in worst.items())))
    assert not fails, fails


# ---- (e) the two cores under their own names ---------------------------------------------------------------------------------
def _composite_direct(inp, inv_s, ca, with_rgb, bg_alpha=None, decoy_density=None):
    """iron_neus_composite, or iron_neus_composite_alpha when bg_alpha [n, mo] is given, called through the C ABI on the tensors
    of O.composite_inputs (the background as density otherwise)."""
    L = _L()
    dev = torch.device("cuda", 0)
    n, m = inp["dists"].shape
    mo = inp["bg_dists"].shape[1]
    g = {k: cu(inp[k]) for k in ("dists", "pts", "dirs", "sdf", "grad", "color", "bg_dists", "bg_density", "bg_color", "background_rgb")}
    if decoy_density is not None:
        g["bg_density"] = cu(decoy_density)
    a = L.iron_neus_composite_args()
    for k in ("dists", "pts", "dirs", "sdf", "grad", "color", "bg_dists", "bg_density", "bg_color"):
        setattr(a, k, g[k].data_ptr())
    a.background_rgb = g["background_rgb"].data_ptr() if with_rgb else None
    a.n, a.m, a.mo, a.inv_s, a.cos_anneal_ratio = n, m, mo, float(inv_s), float(ca)
    out = {"color": torch.empty((n, 3), device=dev), "weights": torch.empty((n, mo), device=dev), "cdf": torch.empty((n, m), device=dev),
           "inside_sphere": torch.empty((n, m), device=dev), "weight_sum": torch.empty((n, 1), device=dev),
           "weight_max": torch.empty((n, 1), device=dev)}
    acc = torch.zeros(2, device=dev)
    a.out_color, a.weights, a.cdf, a.inside_sphere = (out[k].data_ptr() for k in ("color", "weights", "cdf", "inside_sphere"))
    a.weight_sum, a.weight_max, a.gradient_error_acc = out["weight_sum"].data_ptr(), out["weight_max"].data_ptr(), acc.data_ptr()
    if bg_alpha is not None:
        ga = cu(bg_alpha.float())
        L.check(L.load().iron_neus_composite_alpha(C.byref(a), ga.data_ptr(), L.stream_ptr(dev)))
    else:
        L.check(L.load().iron_neus_composite(C.byref(a), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    out["gradient_error"] = acc[0] / (acc[1] + 1e-5)
    return out


@pytest.mark.parametrize("with_rgb", [False, True])
def test_composite_alpha_branch_equals_the_density_branch(with_rgb):
    """iron_neus_composite_alpha (render_core's own signature: the outside pass's alpha) on the synthetic inputs, with the alpha
    computed in fp64 from the density and rounded to fp32: its outputs equal iron_neus_composite's, which recomputes the alpha
    in fp32, and the fp64 composite, within 4 x fp32 floor + 1e-7.  args->bg_density is documented as ignored then: a decoy
    density is passed along."""
    n, m, mo, _ = O.COMPOSITE_SHAPES[1]
    inp = O.composite_inputs(n, m, mo)
    inv_s, ca = 512.0, 0.3
    args = O.composite_args(inp, inv_s, True, with_rgb)
    alpha = O.fp64(O.background_alpha, inp["bg_density"], inp["bg_dists"]).float()
    assert float(alpha.max()) > 0.3 and int((inp["bg_density"] > 20).sum()) >= 5
    by_alpha = _composite_direct(inp, inv_s, ca, with_rgb, bg_alpha=alpha, decoy_density=-inp["bg_density"] - 1.0)
    by_density = _composite_direct(inp, inv_s, ca, with_rgb)
    fails, _ = _check_composite("(e) composite_alpha rgb=%d vs fp64" % with_rgb, by_alpha, args, ca)
    f2, _ = _check_composite("(e) composite_alpha rgb=%d vs the density branch" % with_rgb, by_alpha, args, ca,
                             ref={k: v.detach().cpu().double() for k, v in by_density.items()})
    assert not fails + f2, fails + f2


@functools.lru_cache(maxsize=None)
def _cores():
    """32 of G13's rays, the stage-1 networks of test_gpu_neus.py, the oracle's own up-sampled depths and its two cores (fp32:
    the MLPs dominate the error).  Computed once for the tests below."""
    from test_gpu_neus import _renderer, _stage1
    g = golden("g13_neus.npz")
    nets = _stage1()
    sc = N.NeusScene(cpu_sd(nets["sdf_network"]), R.SDFSpec(), cpu_sd(nets["color_network"]), cpu_sd(nets["nerf"]),
                     nets["deviation_network"].variance.detach().clone())
    o, d, near, far = [t(g[k])[0:96:3].contiguous() for k in ("rays_o", "rays_d", "near", "far")]
    n = o.shape[0]
    with torch.no_grad():
        z = near + (far - near) * torch.linspace(0.0, 1.0, sc.n_samples)[None, :]
        sdf = sc.sdf((o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)).reshape(n, sc.n_samples)
        for i in range(sc.up_sample_steps):
            new_z = N.up_sample(o, d, z, sdf, sc.n_importance // sc.up_sample_steps, 64 * 2 ** i)
            z, sdf = N.cat_z_vals(sc, o, d, z, new_z, sdf, last=(i + 1 == sc.up_sample_steps))
        z_out = far / torch.flip(torch.linspace(1e-3, 1.0 - 1.0 / (sc.n_outside + 1.0), sc.n_outside), dims=[-1]) + 1.0 / sc.n_samples
        z_feed = torch.sort(torch.cat([z, z_out], dim=-1), dim=-1)[0]
        outside = {k: v.detach() for k, v in N.render_core_outside(sc, o, d, z_feed, SAMPLE_DIST).items()}
    detach = lambda out: {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}
    bgrgb = torch.tensor([[0.2, 0.4, 0.6]])
    core_bg = detach(N.render_core(sc, o, d, z, SAMPLE_DIST, outside["alpha"], outside["sampled_color"], None, 0.3))
    core_plain = detach(N.render_core(sc, o, d, z, SAMPLE_DIST, None, None, bgrgb, 0.3))
    return {"renderer": _renderer(nets), "nets": nets, "rays": (o, d), "z": z, "z_feed": z_feed, "outside": outside, "core_bg": core_bg,
            "core_plain": core_plain, "bgrgb": bgrgb}


def _rows_close(tag, got, ref):
    """test_gpu_neus._check's rule for per-sample rows: max <= 1e-2 with at most 2 % of the entries beyond 1e-4."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    dlt = (got - ref).abs()
    print("neus-k (e) %s: max|d| %.1e, %.2f %% beyond 1e-4" % (tag, float(dlt.max()), 100 * float((dlt > 1e-4).float().mean())))
    assert float(dlt.max()) <= 1e-2 and float((dlt > 1e-4).float().mean()) <= 0.02, tag


@pytest.mark.parametrize("with_rgb", [False, True])
def test_render_core_outside_vs_oracle(with_rgb):
    """NeuSRenderer.render_core_outside -> iron_neus_outside_composite, its alpha output included."""
    c = _cores()
    o, d = c["rays"]
    ref = c["outside"]
    bg = c["bgrgb"] if with_rgb else None
    with torch.no_grad():
        out = c["renderer"].render_core_outside(cu(o), cu(d), cu(c["z_feed"]), SAMPLE_DIST, c["nets"]["nerf"], background_rgb=cu(bg))
    assert sorted(out) == ["alpha", "color", "sampled_color", "weights"]
    ref_color = ref["color"] if bg is None else ref["color"] + bg * (1.0 - ref["weights"].sum(dim=-1, keepdim=True))
    dc = float((out["color"].cpu() - ref_color).abs().max())
    print("neus-k (e) render_core_outside rgb=%d: colour max|d| %.1e" % (with_rgb, dc))
    assert out["color"].shape == (32, 3) and dc <= 1e-4
    for k in ("alpha", "weights", "sampled_color"):
        _rows_close("render_core_outside rgb=%d %s" % (with_rgb, k), out[k], ref[k])
    assert float(out["alpha"].max()) > 0.01  # the background is not empty on these rays


@pytest.mark.parametrize("with_background", [True, False])
def test_render_core_vs_oracle(with_background):
    """NeuSRenderer.render_core: with background_alpha / background_sampled_color taken from the ORACLE's outside pass (so only
    the networks and the compositing -- iron_neus_composite_alpha -- differ), and with neither but a constant background colour
    (iron_neus_composite)."""
    c = _cores()
    o, d = c["rays"]
    nets = c["nets"]
    ref = c["core_bg"] if with_background else c["core_plain"]
    kw = ({"background_alpha": cu(c["outside"]["alpha"]), "background_sampled_color": cu(c["outside"]["sampled_color"])} if with_background
          else {"background_rgb": cu(c["bgrgb"])})
    with torch.no_grad():
        out = c["renderer"].render_core(cu(o), cu(d), cu(c["z"]), SAMPLE_DIST, nets["sdf_network"], nets["deviation_network"], nets["color_network"],
                                        cos_anneal_ratio=0.3, **kw)
    assert sorted(out) == sorted(["color", "sdf", "dists", "gradients", "s_val", "mid_z_vals", "weights", "cdf", "gradient_error", "inside_sphere"])
    assert out["weights"].shape == (32, 160 if with_background else 128)
    dc = float((out["color"].cpu() - ref["color"]).abs().max())
    dg = abs(float(out["gradient_error"]) - float(ref["gradient_error"]))
    print("neus-k (e) render_core background=%d: colour max|d| %.1e, gradient_error |d| %.1e" % (with_background, dc, dg))
    assert dc <= 1e-4 and dg <= 1e-5
    for k in ("weights", "cdf", "gradients"):
        _rows_close("render_core background=%d %s" % (with_background, k), out[k], ref[k].reshape(out[k].shape))
    assert torch.equal(out["inside_sphere"].cpu(), ref["inside_sphere"])
    assert float((out["s_val"].cpu() - ref["s_val"]).abs().max()) <= 1e-7
    assert float((out["dists"].cpu() - ref["dists"]).abs().max()) <= 1e-6 and float((out["mid_z_vals"].cpu() - ref["mid_z_vals"]).abs().max()) <= 1e-6


def test_the_cores_refuse_trainable_networks_under_grad_mode():
    L = _L()
    c = _cores()
    o, d = c["rays"]
    nets = c["nets"]
    assert torch.is_grad_enabled() and any(p.requires_grad for p in nets["nerf"].parameters())
    with pytest.raises(L.IronError):
        c["renderer"].render_core_outside(cu(o), cu(d), cu(c["z_feed"]), SAMPLE_DIST, nets["nerf"])
    with pytest.raises(L.IronError):
        c["renderer"].render_core(cu(o), cu(d), cu(c["z"]), SAMPLE_DIST, nets["sdf_network"], nets["deviation_network"], nets["color_network"])


# ---- (f) compositing backward -------------------------------------------------------------------------------------------------
LEAVES = ("sdf", "grad", "color", "inv_s", "bg_density", "bg_color")


def _upstreams(n, mo):
    gen = torch.Generator().manual_seed(43)
    return torch.randn(n, 3, generator=gen), torch.randn(n, 1, generator=gen), torch.randn(n, mo, generator=gen), 0.7


def _loss(out, ups, dtype, dev):
    up_c, up_s, up_w, up_g = ups
    mv = lambda x: x.to(device=dev, dtype=dtype)
    return (out["color"] * mv(up_c)).sum() + (out["weight_sum"] * mv(up_s)).sum() + (out["weights"] * mv(up_w)).sum() + up_g * out["gradient_error"]


def _autograd_reference(inp, inv_s, ca, ups, dtype):
    """Gradients of the loss w.r.t. LEAVES by torch.autograd over the oracle's composite, evaluated on the CPU in `dtype`."""
    args = [a.to(dtype) if torch.is_tensor(a) else a for a in O.composite_args(inp, inv_s, True, True)]
    for i in range(len(LEAVES)):
        args[i] = args[i].clone().requires_grad_(True)
    _loss(O.run_as(dtype, O.composite_with_density, *args, ca), ups, dtype, "cpu").backward()
    return {k: args[i].grad.double() for i, k in enumerate(LEAVES)}


def _kernel_gradients(inp, inv_s, ca, ups):
    args = [cu(a) for a in O.composite_args(inp, inv_s, True, True)]
    for i in range(len(LEAVES)):
        args[i] = args[i].clone().requires_grad_(True)
    from iron_amd.autograd import NeusCompositeFn
    out = dict(zip(("color", "weights", "weight_sum", "gradient_error"), NeusCompositeFn.apply(*args, float(ca))[:4]))
    _loss(out, ups, torch.float32, "cuda").backward()
    return {k: args[i].grad.detach().cpu().double() for i, k in enumerate(LEAVES)}


@pytest.mark.parametrize("inv_s", [37.0, 512.0])
@pytest.mark.parametrize("ca", [0.0, 1.0])
def test_composite_backward_vs_fp64_autograd(ca, inv_s):
    """k_neus_composite_back against fp64 autograd over the oracle's composite at n = 130, m = 160, mo = 192, with every upstream
    fed: colour, the kernel's weight_sum, the weights output itself ([n, mo] random upstream) and the eikonal statistic; with
    cos_anneal_ratio at 0 and 1, where one relu branch carries the whole derivative, and with densities beyond the softplus
    threshold.  rel-L2 <= 2e-4 per tensor; at inv_s = 512, where prev_cdf - next_cdf cancels in the formula itself, the bound is
    max(2e-4, 4 x the rel-L2 of fp32 CPU autograd against fp64 autograd on the same inputs)."""
    n, m, mo, _ = O.COMPOSITE_SHAPES[1]
    inp = O.composite_inputs(n, m, mo)
    ups = _upstreams(n, mo)
    ref = _autograd_reference(inp, inv_s, ca, ups, torch.float64)
    got = _kernel_gradients(inp, inv_s, ca, ups)
    lo = _autograd_reference(inp, inv_s, ca, ups, torch.float32) if inv_s > 37.0 else None
    fails = []
    for k in LEAVES:
        assert bool(torch.isfinite(got[k]).all()), k
        err = rel_l2(got[k].numpy().reshape(-1), ref[k].numpy().reshape(-1))
        floor = rel_l2(lo[k].numpy().reshape(-1), ref[k].numpy().reshape(-1)) if lo is not None else float("nan")
        bound = 2e-4 if lo is None else max(2e-4, 4.0 * floor)
        print("neus-k (f) ca=%g inv_s=%g d/d%s: rel-L2 %.2e, fp32 autograd floor %.2e, bound %.2e" % (ca, inv_s, k, err, floor, bound))
        if err > bound:
            fails.append((k, err, bound))
    assert float(ref["bg_density"].reshape(n, mo)[0, 0].abs()) > 0 and float(ref["inv_s"].abs()) > 0  # the threshold branch carries gradient
    assert not fails, fails


@pytest.mark.parametrize("ca", [0.0, 1.0])
def test_composite_backward_with_zero_normals(ca):
    """Three samples inside |p| < 1.2, one of them in the last partial wave, have an exactly zero normal, and the eikonal
    statistic has a non-zero upstream: 2 (|g| - 1) / |g| must not reach them as -inf * 0.  Every gradient is finite, the zero
    rows' d_grad is autograd's (which masks the zero norm; what is left is the alpha path's share, zero at cos_anneal_ratio = 1),
    and all tensors still agree to rel-L2 2e-4."""
    n, m, mo, _ = O.COMPOSITE_SHAPES[1]
    inp = O.composite_inputs(n, m, mo, zero_normals=True)
    ups = _upstreams(n, mo)
    ref = _autograd_reference(inp, 37.0, ca, ups, torch.float64)
    got = _kernel_gradients(inp, 37.0, ca, ups)
    for k in LEAVES:
        assert bool(torch.isfinite(got[k]).all()), "d/d%s is not finite" % k
    scale = float(ref["grad"].abs().max())
    for ray, j in O.ZERO_NORMALS:
        q = ray * m + j
        print("neus-k (f) zero normal (ray %d, sample %d) ca=%g: d_grad %s, autograd %s" % (ray, j, ca, got["grad"][q].tolist(), ref["grad"][q].tolist()))
        if ca == 1.0:
            assert float(ref["grad"][q].abs().max()) == 0.0 and float(got["grad"][q].abs().max()) == 0.0
        assert float((got["grad"][q] - ref["grad"][q]).abs().max()) <= 2e-4 * max(float(ref["grad"][q].abs().max()), 1e-3 * scale)
    for k in LEAVES:
        err = rel_l2(got[k].numpy().reshape(-1), ref[k].numpy().reshape(-1))
        print("neus-k (f) zero normals ca=%g d/d%s: rel-L2 %.2e" % (ca, k, err))
        assert err <= 2e-4, (k, err)
