"""CPU: the population the neural relight's occlusion query is checked on (tests/_neuralenv_oracle.py), under the oracle tracer in
fp64 and in fp32.  What the GPU test relies on is established here from the reference alone: S0, a near-sphere seen from outside,
shadows nothing at the default shadow_eps; bumpy04_s1 has occluded and free shadow rays side by side, and the reference's own two
precisions agree on (nearly) all of them."""
import torch

import _neuralenv_oracle as NO


def test_s0_shadows_nothing():
    s = NO.shadow_rays("S0")
    assert s.n_hits > 100 and s.o.shape[0] == NO.K * s.n_hits
    assert bool(s.work.any())
    for precision in ("fp64", "fp32"):
        occ = NO.oracle_occluded("S0", precision)
        print("S0 %s: %d hits, %d shadow rays, %d inside the unit sphere, %d occluded"
              % (precision, s.n_hits, occ.numel(), int(s.work.sum()), int(occ.sum())))
        assert int(occ.sum()) == 0


def test_bumpy_has_occluded_and_free_rays_side_by_side():
    s = NO.shadow_rays("bumpy04_s1")
    o64, o32 = NO.oracle_occluded("bumpy04_s1", "fp64"), NO.oracle_occluded("bumpy04_s1", "fp32")
    gap = NO.precision_gap("bumpy04_s1")
    print("bumpy04_s1: %d hits, %d shadow rays, occluded %d (fp64) / %d (fp32), the two precisions differ on %d (share %.3e)"
          % (s.n_hits, o64.numel(), int(o64.sum()), int(o32.sum()), int((o64 != o32).sum()), gap))
    assert 0 < int(o64.sum()) < o64.numel()
    assert 0 < int(o32.sum()) < o32.numel()
    assert not bool(o64[~s.work].any())   # a ray that misses the unit sphere is never occluded
    assert gap <= 1e-3                    # a stable population: the reference's own precisions differ on no more than the mesh path's VIS_SHARE


def test_directions_lie_in_the_normals_hemisphere():
    import _hard_fields as H
    s = NO.shadow_rays("S0")
    f64, _ = H.oracle_fns(NO.build("S0"))
    # the origins lie outside, EPS above the surface, and a step h along w does not lower the distance: f(o + h w) - f(o) =
    # h n.w + O(h^2 |f''|), n.w >= 0, with |f''| ~ 1e2 (tests/_hard_fields.py, sdf_excess) and h = 1e-3 the second term is ~5e-5
    at, ahead = f64(s.o.double()), f64(s.o.double() + 1e-3 * s.w.double())
    assert float(at.min()) > 0.5 * NO.EPS and float(at.max()) < 2 * NO.EPS
    assert float((ahead - at).min()) > -1e-4
    assert float((s.w.norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert torch.equal(s.o.reshape(-1, NO.K, 3)[:, 0], s.o.reshape(-1, NO.K, 3)[:, NO.K - 1])
