"""CPU, from the oracle alone: the fields of tests/_hard_fields.py do exercise the tracer's rarely taken paths (so that
tests/test_gpu_trace_hard_fields.py cannot be vacuous), and the caps that test applies to what it leaves out hold without any
kernel: the share of rays within tau of a sign decision, and the reference's own fp32-vs-fp64 agreement on identical inputs.

Measured at 56 x 56 (3136 rays meet the unit sphere), fp64 oracle; "marginal" = share of sampler rays whose smallest |f| over the
samples up to and including the first negative one is <= tau:

  field               unfinished overshoot roots first<0  >=3 changes  marginal 1e-5 / 5e-5   max |f32 - f64|
  S1 (for scale)          491        1      242     0        59           0    / 1.6 %           1.0e-6
  bumpy02_s1              867      157      586     0       180         0.12 % / 0.81 %          1.1e-6
  bumpy03_s1             1144      396      905     0       317         0.09 % / 0.35 %          1.1e-6
  bumpy03_s2_yaw135       842      216      702     0       243         0.48 % / 1.31 %          1.1e-6
  bumpy04_s1             1336      488     1135     0       452         0.07 % / 0.30 %          1.2e-6
  gen0                   1796      862     1602   178       866         0.06 % / 0.45 %          5.7e-6
  gen1                   1885      943     1775   104       582         0.37 % / 1.17 %          2.5e-6

The floors asserted below sit well under these counts."""
import pytest
import torch

import _hard_fields as HF

FLOORS = {"overshoot": 100, "roots": 500, "multi": 150}
GEN_FLOORS = {"first_neg": 50, "reversed": 1}
EXCLUDED_CAP = 0.02


@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_coverage_and_exclusion_share(name):
    sg = HF.stage(name)
    c = HF.counts(sg)
    print("\n%-18s unfinished %d overshoot %d roots %d first<0 %d >=3 changes %d reversed %d (rooted %d) | marginal 1e-5 %.2f %% 5e-5 %.2f %% | "
          "max|f32-f64| %.1e tau %.1e marginal at tau %.2f %%" % (name, c["unfinished"], c["overshoot"], c["roots"], c["first_neg"], c["multi"],
                                                                 c["reversed"], c["reversed_rooted"], 100 * c["marginal_1e-5"], 100 * c["marginal_5e-5"],
                                                                 c["oracle_noise"], c["tau"], 100 * c["marginal_tau"]))
    for k, floor in FLOORS.items():
        assert c[k] >= floor, (name, k, c[k])
    if name in HF.GEN:
        for k, floor in GEN_FLOORS.items():
            assert c[k] >= floor, (name, k, c[k])
        assert c["reversed_rooted"] >= HF.REVERSED_ROOTED_FLOOR[name], (name, c["reversed_rooted"])   # gen0 only: see the table's comment
    assert c["tau"] >= 1e-5 and c["tau"] == max(1e-5, 4 * c["oracle_noise"])
    assert c["marginal_tau"] <= EXCLUDED_CAP, (name, c["marginal_tau"])
    # the subsets the GPU test wants >= 50 decided rays of
    for k in ("overshoot", "multi") + (("first_neg",) if name in HF.GEN else ()):
        assert int((getattr(sg.sets, k) & sg.decided).sum()) >= 50, (name, k)


@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_reference_sampler_agrees_with_itself(name):
    """Identical inputs, the oracle in fp32 against the oracle in fp64: no root-mask flip among decided rays, and every fp32 root
    of a decided ray inside the fp64 run's bracket (either orientation: a reversed range has z_hi < z_lo).  Undecided rays are left
    out of the bracket check, as in the GPU test: with a deciding value within tau of zero the fp32 run may rightly take another
    bracket.  Their number among the rays rooted in both runs is printed and held to the same 2 % cap."""
    sg = HF.stage(name)
    a, b = sg.sa32, sg.sa
    flips = (a.root != b.root)
    both = a.root & b.root
    dt = (a.t.double() - b.t)[both].abs()
    print("\n%-18s sampler fp32 vs fp64: flips %d (decided: %d), rooted in both %d, max |d root| %.1e" % (
        name, int(flips.sum()), int((flips & sg.decided).sum()), int(both.sum()), float(dt.max())))
    assert int((flips & sg.decided).sum()) == 0
    lo, hi = torch.minimum(b.z_lo, b.z_hi), torch.maximum(b.z_lo, b.z_hi)
    t = a.t.double()
    inside = (t >= lo - 1e-6) & (t <= hi + 1e-6)
    assert bool(inside[both & sg.decided].all()), (name, int((~inside & both & sg.decided).sum()))
    left_out = both & ~sg.decided
    print("   roots left out of the bracket check (undecided): %d of %d, of which outside the fp64 bracket: %d" % (
        int(left_out.sum()), int(both.sum()), int((~inside & left_out).sum())))
    assert int(left_out.sum()) <= EXCLUDED_CAP * int(both.sum())
    assert float(dt[sg.decided[both]].max()) <= 2e-4
    # the oracle's own roots lie in its brackets, and its rootless rays are zeros
    assert bool(((b.t >= lo) & (b.t <= hi))[b.root].all())
    assert float(b.t[~b.root].abs().max()) == 0.0
    # the reading of "reversed range" the GPU test relies on
    rev = sg.sets.reversed & b.root
    assert bool((b.z_hi < b.z_lo)[rev].all())


@pytest.mark.parametrize("name", list(HF.BUMPY))
def test_reference_tracer_agrees_with_itself_on_bumpy_fields(name):
    """The whole tracer (several bisection chunks), fp32 oracle against fp64 oracle: these fields are tame enough for the tight
    tolerances of tests/test_gpu_trace.py.  (The gen fields are not: sphere tracing on a field of slope ~20 is chaotic in the
    reference itself -- 32 mask flips of 1600 rays at 40 x 40 -- which is why they are compared stage by stage.)"""
    r64, e64, _ = HF.oracle_trace(name, "fp64")
    r32, e32, _ = HF.oracle_trace(name, "fp32")
    c64, c32 = r64["convergent_mask"], r32["convergent_mask"]
    flips = int((c64 != c32).sum())
    both = c64 & c32
    dd = float((r32["distance"].double() - r64["distance"])[both].abs().max())
    s64, s32 = float(r64["sdf"][c64].abs().max()), float(r32["sdf"][c32].abs().max())
    print("\n%-18s tracer fp32 vs fp64: hits %d, flips %d, max |d distance| %.1e, evals %d / %d, max |sdf| at a hit %.2e / %.2e" % (
        name, int(c64.sum()), flips, dd, e32, e64, s32, s64))
    assert int(both.sum()) > 1000
    assert flips <= 2
    assert dd <= 2e-4
    # the reference's own |sdf| at its hits exceeds the 1e-4 of S0 / S1 (slope ~1) on these steeper fields, so the GPU test bounds
    # |sdf_gpu - sdf_fp64| ray by ray instead (slope along the ray x |d distance| + tau): the reference's fp32 run must meet that too
    assert s64 <= 2e-4 and s32 <= 2e-4
    excess, slope = HF.sdf_excess(name, r64, r32["sdf"], r32["distance"], both)
    print("   slope along the ray at the hits <= %.2f; max |d sdf| - bound %.2e" % (float(slope.max()), float(excess.max())))
    assert float(excess.max()) <= 0.0


@pytest.mark.parametrize("name", list(HF.FIELDS))
def test_bisection_restatement_is_the_oracles(name):
    """_hard_fields.bisect64 (which also reports the smallest |f_mid| a ray branched on) gives R.rootfind's result on the sampler's
    brackets, reversed ones and two non-brackets included; every d_mid stays inside its bracket.  Printed: the share of rays that
    branched on some |f_mid| <= tau -- a third to a half, which is why the GPU's rootfind test leaves no ray out."""
    from oracle import iron_ref as R
    sg = HF.stage(name)
    sa, r = sg.sa, sg.sa.root
    f_lo, f_hi, d_lo, d_hi = (x[r].float().double() for x in (sa.f_lo, sa.f_hi, sa.z_lo, sa.z_hi))
    oo, dd = sg.ro[sg.m][r].double(), sg.rd[sg.m][r].double()
    f_lo[:2] = -1.0
    p, d, f, n_iter, met = HF.bisect64(sg.f64, f_lo, f_hi, d_lo, d_hi, oo, dd, sg.prm)
    rp, rd_, rf, rn = R.rootfind(sg.f64, f_lo.clone(), f_hi.clone(), d_lo.clone(), d_hi.clone(), oo, dd, sg.prm)
    assert n_iter == rn and torch.equal(d, rd_) and torch.equal(p, rp) and torch.equal(f, rf)
    assert bool(((d >= torch.minimum(d_lo, d_hi)) & (d <= torch.maximum(d_lo, d_hi))).all())
    print("\n%-18s rootfind: %d brackets (%d reversed), %d iterations, branched on |f_mid| <= tau: %.1f %%" % (
        name, int(r.sum()), int((d_hi < d_lo).sum()), n_iter, 100 * float((met <= sg.tau).float().mean())))
