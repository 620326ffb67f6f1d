"""The identity the bisection kernels rely on (csrc/trace.hip, k_bisect_a / k_bisect_b): "own iterations + 1, keep f, then
`remaining` more" visits the reference's mid-points in the reference's order, so d_mid, f_mid and p_mid are EQUAL to
oracle.iron_ref.rootfind run chunk by chunk.  Plain torch on an analytic fp32 SDF; no GPU."""
import torch

from oracle import iron_ref as R

from _bisect_emul import chunk_totals, finish_phase, own_phase


def _sphere_sdf(x):
    return torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]) - 0.5


def _brackets():
    """Rays towards a sphere of radius 0.5 from outside; brackets of widths 2^-3 .. 2^-13 placed unevenly around the root, and
    two that are no brackets (f_lo < 0).  Chunks of unequal sizes, so that the chunks' counts differ."""
    g = torch.Generator().manual_seed(5)
    widths = [2.0 ** -j for j in range(3, 14)]
    n = 4 * len(widths) + 2
    o = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 2.0
    aim = torch.randn(n, 3, generator=g) * 0.15
    d = torch.nn.functional.normalize(aim - o, dim=-1)
    # the root along the ray: |o + t d| = 0.5
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - 0.25
    root = -b - torch.sqrt(b * b - c)
    w = torch.tensor([widths[i % len(widths)] for i in range(n)])
    frac = 0.2 + 0.6 * torch.rand(n, generator=g)
    d_lo = root - frac * w
    d_hi = d_lo + w
    f_lo = _sphere_sdf(o + d * d_lo.unsqueeze(-1))
    f_hi = _sphere_sdf(o + d * d_hi.unsqueeze(-1))
    f_lo[7] = -1.0
    f_lo[n - 1] = -1.0
    sizes = [5, 1, 9, 3, 11, n - 29]   # (the second chunk is one wide bracket, the last holds a non-bracket)
    chunk_of = torch.cat([torch.full((s,), i, dtype=torch.int64) for i, s in enumerate(sizes)])
    assert chunk_of.numel() == n
    return o, d, f_lo, f_hi, d_lo, d_hi, chunk_of, len(sizes)


def test_own_iterations_plus_one_then_the_remainder_is_the_reference_sequence():
    prm = R.TracerParams()
    o, d, f_lo, f_hi, d_lo, d_hi, chunk_of, n_chunks = _brackets()
    assert bool(((f_lo > 0) & (f_hi < 0)).sum() >= f_lo.numel() - 2)

    st = own_phase(_sphere_sdf, f_lo, f_hi, d_lo, d_hi, o, d, prm.sdf_threshold)
    totals = chunk_totals(st, chunk_of, n_chunks)
    got_p, got_d, got_f = finish_phase(_sphere_sdf, st, o, d, totals[chunk_of])

    own = st["k"]
    assert int(own.min()) == 0 and int(own.max()) >= 10            # widths 2^-3 .. 2^-13 at threshold 5e-5: 0 .. 11 own iterations
    assert len(set(totals.tolist())) >= 3                          # chunks of unequal counts
    assert bool((totals[chunk_of] > own).any()) and bool((totals[chunk_of] == own).any())   # both kinds of ray

    for c in range(n_chunks):
        m = chunk_of == c
        want_p, want_d, want_f, n_iter = R.rootfind(_sphere_sdf, f_lo[m].clone(), f_hi[m].clone(), d_lo[m].clone(), d_hi[m].clone(),
                                                    o[m], d[m], prm)
        assert n_iter == int(totals[c])
        assert torch.equal(got_d[m], want_d), c
        assert torch.equal(got_f[m], want_f), c
        assert torch.equal(got_p[m], want_p), c
    # evaluations per ray: k_own + 1, then T - k_own: the reference's T + 1
    assert int((own + 1).sum() + (totals[chunk_of] - own).sum()) == int((totals[chunk_of] + 1).sum())
