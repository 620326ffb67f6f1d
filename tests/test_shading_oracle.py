"""CPU checks of tests/_shading_oracle.py: that the base rows exercise what tests/test_gpu_hit_shading.py is about, and that the
bounds it applies can be met by an honest fp32 evaluation -- from the oracle alone, no GPU."""
import pytest
import torch

import _brdf_oracle as E
import _shading_oracle as S

GPU_MARGIN = 4.0    # tests/test_gpu_hit_shading.py: MARGIN
CASES = [("ggx", False), ("ggx", True), ("mat2_6", False), ("comp", False)]


@pytest.mark.parametrize("netset", S.NETSETS)
def test_strata_lie_on_the_intended_side(netset):
    """130 rows per stratum; n.v on the upper clamp at 0 degrees, on the lower one at 120 (back-facing), strictly inside otherwise."""
    ref = S.reference(netset)
    rows, st = ref["rows"], ref["rows"]["stratum"]
    assert rows["points"].shape == (S.N_BASE, 3) and rows["points"].dtype == torch.float32
    dot = S.raw_dot(rows, ref["chain64"]["normal"])[:, 0]
    for s, deg in enumerate(S.ANGLES_DEG):
        d = dot[st == s]
        assert d.numel() == S.ROWS_PER_STRATUM
        if deg == 0.0:
            assert bool((d >= E.COS_HI).all()), (deg, float(d.min()))
        elif deg > 90.0:
            assert bool((d <= E.COS_LO).all()), (deg, float(d.max()))
        else:
            assert bool(((d > E.COS_LO) & (d < E.COS_HI)).all()), (deg, float(d.min()), float(d.max()))
    dist = (rows["points"].double() - rows["ray_o"].double()).norm(dim=-1)
    assert 0.99 <= float(dist.min()) and float(dist.max()) <= 3.01


@pytest.mark.parametrize("netset,is_metal", CASES)
def test_table_step_share_and_lobe(netset, is_metal):
    ref = S.reference(netset, is_metal)
    st = ref["rows"]["stratum"]
    share = float(ref["step"].double().mean())
    print("%s is_metal=%s: table-step share %.2e" % (netset, is_metal, share))
    assert share <= S.STEP_SHARE
    spec = ref["rad64"]["specular_color"]
    assert float(spec[st == 0].max()) > 1.0      # the specular lobe is exercised at its peak ...
    if S.kind_of(netset) == "ggx":               # (the composite's conductor term has no cosine factor)
        assert float(spec[st == 6].max()) < 1e-3     # ... and clamped away on the back-facing stratum
        ks = ref["chain64"]["specular_albedo"]
        same = bool((ks[:, 0] == ks[:, 1]).all() and (ks[:, 1] == ks[:, 2]).all())
        assert same != is_metal                  # is_metal decides between the channel mean and per-channel albedos
        if is_metal:
            assert float((ks.max(dim=-1).values - ks.min(dim=-1).values).median()) > 1e-3


def test_composite_parameters_are_general():
    """get_materials_comp in fp64 runs on the generalised S2 heads, and every parameter varies from row to row.  Roughness and the
    diffuse albedo lie inside their clamps, the specular albedo on all but a stray entry (its head has bias 0, so |raw| comes down
    to ~1e-5 now and then); metallic_eta lies around its lower bound 0.1; metallic_k and dielectric_eta (heads biased to 0.1, bounds 0.1 and 1.000001) lie
    below it on every row, so the two Fresnel terms see those constants at the bound, as with the untrained heads of S2."""
    c = S.reference("comp")["chain64"]
    B = E.BOUNDS_COMPOSITE
    for k in S.STAGE1["comp"][1:]:
        v = c[k]
        assert v.dtype == torch.float64 and bool(torch.isfinite(v).all())
        spread = float(v.max() - v.min()) / float(v.abs().mean())
        print("%-20s %.4f .. %.4f" % (k, float(v.min()), float(v.max())))
        assert spread >= 0.1, (k, spread)
    assert float(c["specular_roughness"].min()) > 10 * E.BOUNDS_GGX["rough"][0]
    assert float(c["diffuse_albedo"].min()) > 0.1
    assert float((c["specular_albedo"] <= B["ks"][0]).double().mean()) <= 0.01
    assert float(c["metallic_eta"].max()) < B["m_eta"][1]
    assert float(c["metallic_k"].max()) < B["m_k"][0] and float(c["dielectric_eta"].max()) < B["d_eta"][0]


@pytest.mark.parametrize("netset,is_metal", CASES)
def test_fp32_evaluation_meets_the_bounds(netset, is_metal):
    """judge() with margin 1 on the evaluation the floors were measured on (the fp64 chain's normal and materials rounded once,
    the fp32 BRDF of those): it passes at 1 and fails just below, so F, B, the strata and the step rows are wired as documented.
    The whole fp32 chain (its own fp32 normal and materials into the fp32 BRDF) is a different sample of the same roundings -- its
    worst entry is not bounded by the sample maximum B of its neighbour -- and is held to the margin the GPU file applies."""
    ref = S.reference(netset, is_metal)
    kind = S.kind_of(netset)
    once = {k: ref["chain64"][k].float() for k in S.STAGE1[kind]}
    once.update(S.brdf(netset, ref["rows"], once, torch.float32))
    rep = S.judge(netset, is_metal, once, 1.0, "floor sample")
    assert max(rep[k]["worst"] for k in S.RADIANCE[kind]) == 1.0
    with pytest.raises(AssertionError):
        S.judge(netset, is_metal, once, 0.99, "floor sample")
    rep = S.judge(netset, is_metal, ref["chain32"], GPU_MARGIN, "fp32 chain")
    print("%s is_metal=%s fp32 chain: %s" % (netset, is_metal, S.describe(rep)))
    for k in S.STAGE1[kind]:       # by construction: F is this very difference
        assert rep[k]["ratio"] <= 1.0


@pytest.mark.parametrize("netset", S.NETSETS)
def test_judge_sees_one_wrong_row(netset):
    """One row of one output off by 1e-3 (what a frame's rel-L2 of 1e-4 cannot see) fails, and the message names it."""
    ref = S.reference(netset)
    for key, row in (("normal", 131), ("color", 5), ("specular_roughness", 909)):
        got = {k: v.clone() for k, v in ref["chain32"].items()}
        got[key][row, 0] += 1e-3
        with pytest.raises(AssertionError, match="row %d" % row):
            S.judge(netset, False, got, 4.0, "one wrong row")
