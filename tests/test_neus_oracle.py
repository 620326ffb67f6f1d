"""The high-precision side of tests/test_gpu_neus_kernels.py, checked on the CPU: oracle/neus_ref.py run in fp64 against the real
reference's recorded output, sample_pdf with a given u against the oracle's det=True branch, and the conditions the GPU tests
lean on -- the flag caps for every input set they use, the margins of the input builders, and what torch.autograd makes of a
zero normal."""
import pytest
import torch

import _neus_oracle as O
from oracle import neus_ref as N

from _util import golden, t


def test_fp64_runs_the_oracle_in_fp64_and_restores_the_default():
    g = golden("g13_neus.npz")
    bins, w = t(g["pdf_bins"]), t(g["pdf_weights"])
    assert torch.get_default_dtype() == torch.float32
    s = O.fp64(N.sample_pdf, bins, w, 16, det=True)
    assert s.dtype == torch.float64 and torch.get_default_dtype() == torch.float32
    # G13's pdf_samples are the real reference's fp32 output: fp64 reproduces them to fp32 rounding of the depths (~2.5)
    assert float((s - t(g["pdf_samples"]).double()).abs().max()) <= 4 * 2.0 ** -22
    with pytest.raises(ZeroDivisionError):
        O.fp64(lambda x: 1 // 0, bins)
    assert torch.get_default_dtype() == torch.float32
    floor = O.fp32_floor(N.sample_pdf, bins, w, 16, det=True)
    assert 0.0 < floor <= 4 * 2.0 ** -22


@pytest.mark.parametrize("k", O.PDF_K)
def test_sample_pdf_u_with_the_linspace_is_the_det_branch(k):
    bins, w = O.pdf_inputs()
    ref = O.fp64(N.sample_pdf, bins, w, k, det=True)
    u = torch.linspace(0.0 + 0.5 / k, 1.0 - 0.5 / k, steps=k, dtype=torch.float64).expand(bins.shape[0], k)
    assert torch.equal(O.sample_pdf_u(bins, w, u), ref)
    g = golden("g13_neus.npz")
    u16 = torch.linspace(0.5 / 16, 1.0 - 0.5 / 16, steps=16, dtype=torch.float64).expand(16, 16)
    assert torch.equal(O.sample_pdf_u(t(g["pdf_bins"]), t(g["pdf_weights"]), u16), O.fp64(N.sample_pdf, t(g["pdf_bins"]), t(g["pdf_weights"]), 16))


def _cap(flag, what):
    share = float(flag.double().mean())
    print("%s: %d / %d entries flagged (%.2f %%)" % (what, int(flag.sum()), flag.numel(), 100 * share))
    assert share <= 0.01, (what, share)


def test_inverse_cdf_flag_caps_for_every_gpu_input_set():
    """At most 1 % of the entries of any case of the GPU file are left out of its value comparisons."""
    total = flagged = 0
    for n, n_bins, k in O.PDF_CASES:
        bins, w = O.pdf_inputs(n, n_bins)
        for u, tag in ((O.det_u(n, k), "det"), (O.pdf_given_u(n, k).double(), "given u")):
            f = O.flag_inverse_cdf(bins, w, u)
            _cap(f, "sample_pdf n=%d bins=%d k=%d %s" % (n, n_bins, k, tag))
            total, flagged = total + f.numel(), flagged + int(f.sum())
    for m in O.UP_SAMPLE_M:
        o, d, z, sdf = O.up_sample_inputs(130, m)
        assert O.up_sample_radius_clear(o, d, z)
        for inv_s in O.UP_SAMPLE_INV_S:
            w64 = O.up_sample_sections(o, d, z, sdf, inv_s, torch.float64)
            for k in O.PDF_K:
                f = O.flag_inverse_cdf(z, w64, O.det_u(130, k))
                _cap(f, "up_sample m=%d inv_s=%g k=%d" % (m, inv_s, k))
                total, flagged = total + f.numel(), flagged + int(f.sum())
    print("all inverse-CDF cases: %.3f %% flagged" % (100.0 * flagged / total))


def test_flagging_marks_what_it_should():
    bins = torch.tensor([[0.0, 1.0, 2.0, 3.0]])
    w = torch.tensor([[1.0, 2.0, 1.0]])
    cdf = O.pdf_cdf(w.double())[0]
    u = torch.stack([cdf[1] + 5e-6, cdf[1] + 5e-5, cdf[2] - 9e-6, torch.tensor(0.0, dtype=torch.float64), cdf[3] - 6e-8])[None]
    assert O.flag_inverse_cdf(bins, w, u).tolist() == [[True, False, True, False, False]]
    thin = torch.tensor([[1.0, 0.0, 1.0]])  # middle section: denom ~ 5e-6, below the switch
    assert bool(O.flag_inverse_cdf(bins, thin, torch.tensor([[0.5]]))[0, 0])
    pts = torch.tensor([[0.0, 0.0, 1.0 + 5e-7], [0.0, 0.5, 0.0], [0.0, 0.0, 0.3], [1.2 - 3e-7, 0.0, 0.0], [0.0, 0.3, 0.0], [2.0, 0.0, 0.0]])
    assert O.flag_composite_rays(pts, 3, 2).tolist() == [True, True, False]


def test_composite_inputs_keep_their_margins_and_flag_no_ray():
    for n, m, mo, with_bg in O.COMPOSITE_SHAPES:
        assert int(O.flag_composite_rays(O.composite_inputs(1, m, mo)["pts"], 1, m).sum()) == 0  # the single-ray case of the GPU file
        for zero in (False, True):
            inp = O.composite_inputs(n, m, mo, zero_normals=zero)
            assert int(O.flag_composite_rays(inp["pts"], n, m).sum()) == 0
            r = inp["pts"].double().reshape(n, m, 3).norm(dim=-1)
            assert bool(((r < 1).any(-1) & ((r > 1) & (r < 1.2)).any(-1) & (r > 1.2).any(-1)).all())  # both sides of both radii, every ray
            ins = r < 1
            flips = (ins[:, 1:] != ins[:, :-1]).sum(dim=-1)
            assert all(int(flips[i]) > 10 for i in O.TOGGLE_ROWS) and int(flips[0]) == 2
            tc = (inp["dirs"].double() * inp["grad"].double()).sum(-1)
            live = inp["grad"].abs().sum(-1) > 0
            assert int((~live).sum()) == (len(O.ZERO_NORMALS) if zero else 0)
            assert float(tc[live].abs().min()) > 1e-3 and float((-tc[live] * 0.5 + 0.5).abs().min()) > 1e-3
            if zero:
                for ray, j in O.ZERO_NORMALS:
                    assert float(r[ray, j]) < 1.2 and ray * m + j < n * m
                assert max(ray for ray, _ in O.ZERO_NORMALS) >= 128  # one in the last partial wave of n = 130
            dens = inp["bg_density"].reshape(n, mo)
            assert int((dens > 20).sum()) >= 5 and all(float(r[ray, j]) > 1.0 for ray, j, _ in O.BIG_DENSITY)  # and read by the blend
            # the fp64 and the fp32 evaluation agree on every discrete output
            for ca in (0.0, 1.0):
                args = O.composite_args(inp, 512.0, with_bg, True)
                dev = O.fp32_deviation(O.composite_with_density, *args, ca)
                assert float(dev["inside_sphere"].max()) == 0.0


def test_autograd_over_the_fp64_composite_gives_zero_for_a_zero_normal():
    """linalg.norm's backward masks the zero norm: the eikonal statistic sends nothing into an exactly zero normal, and with
    cos_anneal_ratio = 1 the alpha path (relu(-true_cos) at 0) sends nothing either -- the row's gradient is finite and zero."""
    n, m, mo, _ = O.COMPOSITE_SHAPES[1]
    inp = O.composite_inputs(n, m, mo, zero_normals=True)
    args = [a.double() if torch.is_tensor(a) else a for a in O.composite_args(inp, 37.0, True, True)]
    grad = args[1].requires_grad_(True)
    out = O.fp64(O.composite_with_density, *args, 1.0)
    ((out["color"] * 0.3).sum() + out["weight_sum"].sum() + 0.7 * out["gradient_error"]).backward()
    assert grad.grad.dtype == torch.float64 and bool(torch.isfinite(grad.grad).all())
    for ray, j in O.ZERO_NORMALS:
        assert grad.grad[ray * m + j].abs().max() == 0.0
    assert float(grad.grad.abs().max()) > 0.0
