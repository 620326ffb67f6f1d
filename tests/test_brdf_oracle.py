"""CPU checks of the high-precision side of the co-located BRDF tests (tests/_brdf_oracle.py): the yardstick y really is what an
honest fp32 evaluation delivers (r_cpu = max |fp32 CPU oracle - fp64| / y <= 8 for every head, stratum, upstream configuration and
output), the factorisation behind its cancellation term reproduces the gradient, the flags stay within their cap, and every clamp
stratum holds the dead, live and on-bound rows it is there for.  No GPU."""
import pytest
import torch

import _brdf_oracle as B

R_CPU_MAX = 8.0
FLAG_CAP = 0.01


@pytest.mark.parametrize("head", B.HEADS)
def test_honest_fp32_stays_within_the_yardstick(head):
    ref = B.reference(head)
    worst = {}
    for s, sl in ref["slices"].items():
        for cfg, r in ref["cfg"].items():
            for key in B.entry_keys(head, ref, cfg):
                v = B.r_cpu(head, ref, cfg, key, sl)
                assert v == v, (head, s, cfg, key)  # no NaN
                worst[(s, key)] = max(worst.get((s, key), 0.0), v)
            if head != "composite_env":   # the rows of d/dlight, and their fp32 sum against the sum's own tolerance
                worst[(s, "d:light")] = max(worst.get((s, "d:light"), 0.0), B.r_cpu(head, ref, cfg, "d:light", sl))
                tol = B.light_tolerance(r["y"]["d:light"][sl], r["t64"][sl], worst[(s, "d:light")])
                assert abs(float(r["t32"][sl].float().sum()) - float(r["t64"][sl].sum())) <= tol, (head, s, cfg)
        print("brdf-o %s %s r_cpu" % (head, s), " ".join("%s=%.2f" % (k, v) for (s2, k), v in worst.items() if s2 == s))
    bad = {k: v for k, v in worst.items() if v > R_CPU_MAX}
    assert not bad, bad


@pytest.mark.parametrize("head", B.HEADS)
def test_partial_terms_sum_to_the_gradient(head):
    """The lobes and factors of the cancellation term are the formula: their signed sum is the scalar-space gradient."""
    ref = B.reference(head)
    for cfg, r in ref["cfg"].items():
        for k, s in r["partials"]["signed"].items():
            g = r["scalar"][k]
            err = float(((s - g).abs() / (r["partials"]["abs"][k] + 1e-300)).max())
            assert err <= 1e-9, (head, cfg, k, err)
        for name, v in r["partials"]["lobe"].items():
            o = r["partials"]["lobe_oracle"][name]
            assert float(((v - o).abs() / (o.abs() + 1e-300)).max()) <= 1e-9, (head, cfg, name)


@pytest.mark.parametrize("head", B.HEADS)
def test_scalar_space_is_the_formula(head):
    """The scalar-space evaluation (n = (0,0,1), v = (0,0,c), clamped inputs, open clamps) returns the oracle's fp64 outputs."""
    ref = B.reference(head)
    r = ref["cfg"]["mixed"]
    for k, o in r["out64"].items():
        err = float(((r["scalar"]["out:" + k] - o).abs() / (o.abs() + 1e-300)).max())
        assert err <= 1e-12, (head, k, err)


@pytest.mark.parametrize("head", B.HEADS)
def test_flag_caps_and_liveness(head):
    ref = B.reference(head)
    fl = ref["flags"]
    for s, sl in ref["slices"].items():
        n = sl.stop - sl.start
        flagged = int((fl["table"] | fl["bound"])[sl].sum())
        assert flagged <= FLAG_CAP * n, (head, s, flagged)
    # off the flagged rows the fp32 and the fp64 run agree on which gradient entries are dead, but for ONE row of the composite
    # (near-normal, metallic-only upstream) where the fp32 derivative of the saturated Fresnel term rounds to 0
    rows = set()
    for cfg, r in ref["cfg"].items():
        for k in r["g64"]:
            if k != "light":
                differ = ((r["g32"][k] == 0) != (r["g64"][k] == 0)) & ~fl["bound"][:, None]
                rows |= set(differ.nonzero()[:, 0].tolist())
    print("brdf-o %s rows with a gradient that is zero in one precision only: %s" % (head, sorted(rows)))
    assert len(rows) <= (1 if B.is_composite(head) else 0), (head, sorted(rows))


def _quantity_rows(head, ref, sl, q):
    """(dead, live, on-bound) row masks of a clamped quantity within a stratum (any channel for an albedo)."""
    inp = ref["inputs"]
    if q == "cos":
        raw, bb = B.raw_dot(inp)[sl], (B.COS_LO, B.COS_HI)
    else:
        raw, bb = inp[q].double()[sl], B.bounds(head)[q]
    lo, hi = bb
    on = (raw == lo) | ((raw == hi) if hi is not None else torch.zeros_like(raw, dtype=torch.bool))
    dead = (raw < lo) | ((raw > hi) if hi is not None else torch.zeros_like(raw, dtype=torch.bool))
    return dead.any(-1), (~dead & ~on).all(-1), on.any(-1), dead, on


@pytest.mark.parametrize("head", B.HEADS)
def test_clamp_strata_hold_dead_live_and_on_bound_rows(head):
    ref = B.reference(head)
    r = ref["cfg"]["mixed"]
    grad_of = {"cos": "viewdir"}
    for s, what in B.CLAMP_STRATA.items():
        if s not in ref["slices"]:
            continue
        sl = ref["slices"][s]
        for q in ((what,) if isinstance(what, str) else what):
            if q != "cos" and q not in B.bounds(head):
                continue
            dead_rows, live_rows, on_rows, dead, on = _quantity_rows(head, ref, sl, q)
            assert int(dead_rows.sum()) >= 10 and int(live_rows.sum()) >= 10 and int(on_rows.sum()) >= 4, (head, s, q)
            if q == "cos" and head in ("smooth_dielectric", "thin_dielectric"):
                continue  # no cosine in the formula: the gradient is zero everywhere
            g = r["g32"][grad_of.get(q, q)][sl]
            if q == "cos":
                assert bool((g[dead_rows] == 0).all()) and bool((g[on_rows].abs().sum(-1) > 0).all()) and bool((g[live_rows].abs().sum(-1) > 0).all())
            else:
                assert bool((g[dead] == 0).all()) and bool((g[on] != 0).all()) and bool((g[~dead & ~on] != 0).all()), (head, s, q)


def test_interior_rows_are_better_conditioned():
    """Relative y (median over the stratum) of the GGX specular lobe and of d/droughness: smaller in the interior than at grazing
    incidence and for glossy near-normal rows -- the yardstick follows the conditioning of the row, not the stratum's worst."""
    ref = B.reference("ggx")
    r = ref["cfg"]["mixed"]

    def rel(key, s):
        kind, name = key.split(":")
        o = (r["out64"] if kind == "out" else r["g64"])[name][ref["slices"][s]]
        return float((r["y"][key][ref["slices"][s]] / o.abs()).median())

    for key in ("out:specular_rgb", "d:rough"):
        inner = rel(key, "interior")
        for s in ("grazing", "glossy_near_normal"):
            print("brdf-o conditioning %s interior %.2e %s %.2e" % (key, inner, s, rel(key, s)))
            assert inner < rel(key, s), (key, s)


@pytest.mark.parametrize("s", B.SMITH_STRATA)
def test_smith_g1_fp32_within_yardstick(s):
    ref, lo, y = B.smith_reference(s)
    v = float(((lo.double() - ref).abs() / y).max())
    print("brdf-o smith_g1 %s r_cpu=%.2f" % (s, v))
    assert v <= R_CPU_MAX
