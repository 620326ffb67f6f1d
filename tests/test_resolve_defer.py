"""CPU: the resolve's two rounds (csrc/trace.hip k_resolve_list) select enough.

A pending ray's outcome is made of `first` -- the smaller of the march's first certainly-negative sample and the first listed sample
whose exact value is negative -- and of the exact values of the listed samples `first` and `first - 1`.  The rule under test: a
listed sample is deferred when an earlier listed sample of its ray has a screened value f1 < 0 (strictly: NaN and zeros are not
negative; the first such sample is itself not deferred); round 1 evaluates the samples that are not deferred, round 2 the deferred
ones in front of round 1's `first`.  In plain torch, on random per-ray sequences of (f1, f_ex) and on hand-made ones, that selection
gives the `first`, f_ex[first] and f_ex[first - 1] of evaluating everything, and never reads a value it did not evaluate.

On S0 at 200 x 200 (the oracle's exact values standing in for the screened ones, delta = 0.0068, the stride-1 march of
tools/sampler_stride_margin.py) more than 40 % of the listed samples are deferred: the rule cannot pass on an empty deferral.
Measured with the oracle alone: 52 % (30 784 of 58 657 samples, 6 237 pending rays)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

NONE = 1 << 20   # "no such sample"


def deferred_mask(listed, f1):
    """[R, N] bool: listed samples behind their ray's first listed sample with f1 < 0."""
    neg1 = listed & (f1 < 0)
    earlier = (torch.cumsum(neg1.long(), 1) - neg1.long()) > 0
    return listed & earlier


def first_over(evaluated, fex, first_c):
    """min(first_c, first evaluated sample with f_ex < 0) per ray."""
    s = torch.arange(fex.shape[1]).expand_as(fex)
    cand = torch.where(evaluated & (fex < 0), s, torch.full_like(s, NONE))
    return torch.minimum(first_c, cand.min(1).values)


def outcome(evaluated, fex, first):
    """What k_screen_fin_entries takes: (f_ex[first], f_ex[first - 1]) as bit patterns, -1 where that sample has no exact value."""
    R, N = fex.shape
    bits = fex.view(torch.int32).long()
    r = torch.arange(R)
    hi_ok = (first < N) & evaluated[r, first.clamp(max=N - 1)]
    lo_ok = (first >= 1) & (first - 1 < N) & evaluated[r, (first - 1).clamp(0, N - 1)]
    hi = torch.where(hi_ok, bits[r, first.clamp(max=N - 1)], torch.full_like(first, -1 << 40))
    lo = torch.where(lo_ok, bits[r, (first - 1).clamp(0, N - 1)], torch.full_like(first, -1 << 40))
    return hi, lo


def two_rounds(listed, f1, fex, first_c):
    d = deferred_mask(listed, f1)
    r1 = listed & ~d
    first1 = first_over(r1, fex, first_c)
    s = torch.arange(fex.shape[1]).expand_as(fex)
    r2 = d & (s < first1[:, None])
    ev = r1 | r2
    first2 = first_over(ev, fex, first_c)
    return first2, ev, d, r2


def check(listed, f1, fex, first_c):
    want_first = first_over(listed, fex, first_c)
    want_hi, want_lo = outcome(listed, fex, want_first)
    first, ev, d, r2 = two_rounds(listed, f1, fex, first_c)
    assert torch.equal(first, want_first)
    hi, lo = outcome(ev, fex, first)
    assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo)
    return d, r2, ev


def _random_rays(R, N, seed):
    g = torch.Generator().manual_seed(seed)
    delta = 0.0068
    f1 = (torch.rand(R, N, generator=g) * 2 - 1) * delta
    # the exact value: near the screened one, or (one sample in six) of the other sign
    fex = f1 + (torch.rand(R, N, generator=g) * 2 - 1) * 0.05 * delta
    flip = torch.rand(R, N, generator=g) < 1.0 / 6.0
    fex = torch.where(flip, -fex, fex)
    special = torch.tensor([float("nan"), 0.0, -0.0])
    for t in (f1, fex):
        pick = torch.rand(R, N, generator=g) < 0.06
        t[pick] = special[torch.randint(0, 3, (int(pick.sum()),), generator=g)]
    # a third of the rays are positive throughout on the screen, a sixth in both
    kind = torch.randint(0, 6, (R,), generator=g)
    f1[kind < 2] = f1[kind < 2].abs()
    fex[kind == 0] = fex[kind == 0].abs()
    listed = torch.rand(R, N, generator=g) < 0.6
    # the march's own end: behind every listed sample, or none
    last = torch.where(listed, torch.arange(N).expand(R, N), torch.full((R, N), -1)).max(1).values
    first_c = torch.where(torch.rand(R, generator=g) < 0.5, last + 1 + torch.randint(0, 3, (R,), generator=g), torch.full((R,), N + 7))
    listed = listed & (torch.arange(N).expand(R, N) < first_c[:, None])
    return listed, f1.contiguous(), fex.contiguous(), first_c


def test_selection_matches_evaluating_everything_on_random_rays():
    seen_r2 = seen_moot = seen_none = seen_s0 = 0
    for seed in range(4):
        listed, f1, fex, first_c = _random_rays(4096, 12, seed)
        d, r2, ev = check(listed, f1, fex, first_c)
        seen_r2 += int(r2.sum())
        seen_moot += int((d & ~ev).sum())
        seen_none += int((~(listed & (fex < 0)).any(1) & ~(listed & (f1 < 0)).any(1) & listed.any(1)).sum())
        seen_s0 += int((listed[:, 0] & (f1[:, 0] < 0) & (fex[:, 0] < 0)).sum())
    # the cases the rule has to survive all occur: round 2 is not empty, deferred samples stay unevaluated, rays without a negative,
    # a negative at s = 0
    assert seen_r2 > 0 and seen_moot > 0 and seen_none > 0 and seen_s0 > 0, (seen_r2, seen_moot, seen_none, seen_s0)


def test_hand_made_rays():
    nan, N = float("nan"), 6
    rows = [
        # f1, f_ex, first_c
        ([1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], N + 7),             # no negative at all: nothing deferred
        ([-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], N + 7),  # negative at s = 0: everything behind it deferred and moot
        ([1, -1, 1, -1, 1, 1], [1, 1, 1, 1, -1, 1], N + 7),          # the screen's negatives are all wrong: round 2 finds s = 4
        ([1, -1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], 6),                # ... and none is right: the march's own end stands
        ([1, 1, 1, 1, 1, 1], [1, 1, -1, 1, 1, 1], N + 7),            # the screen misses a negative: no deferral, found by round 1
        ([nan, -0.0, 0.0, -1, 1, 1], [1, 1, 1, 1, 1, -1], N + 7),    # NaN and zeros on the screen are not negative
        ([-1, 1, 1, 1, 1, 1], [nan, -0.0, 0.0, 1, -1, 1], N + 7),    # ... nor as exact values: round 2 walks on to s = 4
        ([1, 1, -1, 1, 1, 1], [1, 1, 1, -1, 1, 1], N + 7),           # first = 3 deferred, first - 1 = 2 is the ray's first screened negative
        ([1, 1, -1, -1, 1, 1], [1, 1, 1, 1, -1, 1], 5),              # the sample before the march's end is deferred and needed
    ]
    f1 = torch.tensor([r[0] for r in rows], dtype=torch.float32) * 1e-3
    fex = torch.tensor([r[1] for r in rows], dtype=torch.float32) * 1e-3
    first_c = torch.tensor([r[2] for r in rows])
    listed = torch.arange(N).expand(len(rows), N) < first_c[:, None]
    d, r2, ev = check(listed, f1, fex, first_c)
    assert d.sum(1).tolist() == [0, 5, 4, 4, 0, 2, 5, 3, 2]
    assert r2.sum(1).tolist() == [0, 0, 4, 4, 0, 2, 5, 3, 2]   # (all of a ray's deferred samples, or none)
    first, _, _, _ = two_rounds(listed, f1, fex, first_c)
    assert first.tolist() == [N + 7, 0, 4, 6, 2, 5, 4, 3, 4]


def test_s0_defers_more_than_two_fifths_of_the_listed_samples():
    import sampler_stride_margin as ST
    from test_sampler_stride_margin import _net   # the S0 samples at 200 x 200, evaluated once per session
    _, _, (fe, _, dz, width) = _net("S0")
    m = ST.march_rays(fe, fe, dz, width, 0.0068, 0.0)   # stride 1 throughout; the exact value stands in for the screened one
    rows = [(r, listed) for r, (listed, _) in enumerate(m["classified"]) if listed]
    N = fe.shape[1]
    listed = torch.zeros(len(rows), N, dtype=torch.bool)
    for i, (_, ls) in enumerate(rows):
        listed[i, list(ls)] = True
    f = fe[[r for r, _ in rows]].float().contiguous()
    first_c = torch.tensor([m["classified"][r][1] for r, _ in rows])
    d, r2, ev = check(listed, f, f, first_c)
    n_listed, n_def = int(listed.sum()), int(d.sum())
    print("S0 200 x 200: pending rays %d, listed %d, deferred %d (%.3f), round 2 %d, without a negative %d"
          % (len(rows), n_listed, n_def, n_def / n_listed, int(r2.sum()), int((~(listed & (f < 0)).any(1)).sum())))
    assert len(rows) > 5000 and n_listed > 50000, (len(rows), n_listed)
    assert n_def > 0.40 * n_listed, (n_def, n_listed)
    assert int(r2.sum()) == 0   # with the screen's sign exact, nothing comes back
