"""CPU: what tests/test_gpu_backward_rows.py rests on -- the live sets and strata of tests/_backward_oracle.py, the fp32 oracle
inside its own floors, the share of ReLU-kink rows, and the expected values of the activation probe."""
import math

import numpy as np
import pytest
import torch

import _backward_oracle as B


def test_live_sets_reach_the_edges_of_blocks_and_chunks():
    assert B.live_set(1, 32) == [0]
    assert B.live_set(128, 32) == [0, 127, 31, 32]                      # no partial block
    assert B.live_set(129, 32) == [0, 128, 31, 32]                      # a last block of one point (its first row is its last)
    assert B.live_set(161, 32) == [0, 160, 31, 32]
    assert B.live_set(127, 32) == [0, 126, 31, 32, 96]                  # first and last row of the 31-point block
    assert B.live_set(257, 64) == [0, 256, 31, 32]
    assert B.live_set(321, 64) == [0, 320, 31, 32]
    assert B.live_set(255, 64) == [0, 254, 31, 32, 192]
    assert B.live_set(B.SDF_CHUNK + 129, 32, B.SDF_CHUNK) == [0, 65664, 31, 32, 65535, 65536]
    assert B.live_set(B.SDF_CHUNK + 128, 32, B.SDF_CHUNK) == [0, 65663, 31, 32, 65535, 65536]
    assert B.live_set(B.SDF_CHUNK + 1, 32, B.SDF_CHUNK) == [0, 65536, 31, 32, 65535]
    assert B.live_set(B.SDF_CHUNK, 32, B.SDF_CHUNK) == [0, 65535, 31, 32]
    assert B.live_set(B.RENDER_CHUNK + 257, 64, B.RENDER_CHUNK) == [0, 131328, 31, 32, 131071, 131072]
    for n in B.SDF_TANGENT_SIZES + B.SDF_PLAIN_SIZES:
        for blk in (32, 64):
            s = B.live_set(n, blk)
            assert 1 <= len(s) <= 8 and len(set(s)) == len(s) and 0 in s and n - 1 in s and all(0 <= r < n for r in s)
    # the sizes straddle the row kernel's gate (256 rows: 128 points with tangent rows, 256 without)
    assert 127 in B.SDF_TANGENT_SIZES and 128 in B.SDF_TANGENT_SIZES and 129 in B.SDF_TANGENT_SIZES
    assert all(k in B.SDF_PLAIN_SIZES for k in (255, 256, 257)) and all(k in B.NET_SIZES for k in (255, 256, 257))


def _all_live_rows():
    """Every live position of a material-net or NeRF case (64-row blocks)."""
    rows = set()
    for n in B.NET_SIZES:
        rows.update(B.live_set(n, 64))
    for extra in B.RENDER_CHUNK_EXTRA:
        rows.update(B.live_set(B.RENDER_CHUNK + extra, 64, B.RENDER_CHUNK))
    return sorted(rows)


@pytest.mark.parametrize("kind,name", [("render", n) for n in B.RENDER_NETS] + [("nerf", "prod")])
def test_kink_rows_stay_under_the_cap(kind, name):
    """The reference alone decides which rows are left out; with the seeds in use none of the live positions is one (2 % of a
    live set of <= 8 rows is no row), and the pool as a whole stays under the cap too."""
    net = B.net_of(kind, name)
    kp = B.kink_pool(net)
    share = float(kp.float().mean())
    print("%s %s: %.2f %% of the pool's rows pass a ReLU kink" % (kind, name, 100 * share))
    assert share <= B.KINK_CAP
    live = _all_live_rows()
    keep, dropped = B.drop_kinks(net, live)
    assert dropped <= B.KINK_CAP * len(live), (dropped, [r for r in live if r not in keep])
    for n in B.NET_SIZES:
        s = B.live_set(n, 64)
        assert B.drop_kinks(net, s)[1] <= B.KINK_CAP * len(s)


CASES = [("sdf", "prod", 129, "sfg"), ("sdf", "n4_skip2", 128, "e"), ("sdf", "n8_dout1", 127, "g"), ("sdf", "n8_nown", 256, "sf"),
         ("sdf", "alt", 161, "sfg"), ("render", "idr_0_4/prod", 257, "o"), ("render", "idr_10_4_skip/prod", 255, "o"),
         ("render", "alt", 321, "o"), ("nerf", "prod", 257, "ar")]


@pytest.mark.parametrize("kind,name,n,parts", CASES)
def test_fp32_oracle_stays_inside_its_floors(kind, name, n, parts):
    """The per-point contributions add up to the live set's gradient (the embedding's premise), in fp64 to rounding; and the fp32
    oracle summed point by point -- another order of the same arithmetic than the evaluation F came from -- stays inside the bound
    the device is held to.  F itself is printed against the TOL_PARAM fallback."""
    net = B.net_of(kind, name)
    live, dropped = B.drop_kinks(net, B.live_set(n, 32 if (kind == "sdf" and ("g" in parts or "e" in parts)) else 64))
    assert dropped == 0
    bi, up = B.embed(net, n, live, parts)
    for k, v in up.items():
        if v is not None:
            dead = torch.ones(n, dtype=torch.bool)
            dead[live] = False
            assert float(v[dead].abs().max()) == 0.0 and float(v[live].abs().min(dim=1).values.min()) >= 0.0
    ex = B.expect(net, bi, up, live)
    pts64 = B.oracle_per_point(net, bi, up, live, torch.float64)
    pts32 = B.oracle_per_point(net, bi, up, live, torch.float32)
    worst = 0.0
    for name_ in net.param_names():
        ref = ex.ref[name_]
        if ref is None:
            assert all(p[0][name_] is None for p in pts64)
            continue
        s64 = sum(p[0][name_] for p in pts64)
        assert float((s64 - ref).norm()) <= 1e-12 * max(float(ref.norm()), 1e-300) + 1e-300, name_
        s32 = sum(p[0][name_].double() for p in pts32)
        err = float((s32 - ref).norm())
        assert err <= ex.bound(name_), (name_, err, ex.bound(name_))
        worst = max(worst, B.MARGIN * ex.floor[name_] / max(B.TOL_PARAM * float(ref.norm()), 1e-300))
    for j, r in enumerate(ex.in_ref):
        if r is None:
            continue
        rows32 = torch.cat([p[1][j] for p in pts32]).double()
        bound = torch.maximum(B.MARGIN * ex.in_floor[j], B.TOL_PARAM * r.norm(dim=1))
        assert bool(((rows32 - r).norm(dim=1) <= bound).all()), j
    print("%s %s n=%d %s: |S| = %d, 4 F is at most %.2f of the TOL_PARAM fallback" % (kind, name, n, parts, len(live), worst))
    if kind == "sdf" and parts in ("g", "e"):
        last = net.layers[-1][0] + ".bias"
        assert ex.ref[last] is None                     # a gradient-only loss has no path to the last bias


def test_softplus_strata():
    z = B.softplus_strata()
    assert z.dtype == np.float32 and len(z) == 22
    t = 100.0 * z.astype(np.float64)
    for c in (20.0, 25.0, 60.0):
        lo, hi = t[t < c].max(), t[t > c].min()
        assert c - lo < 1e-5 and hi - c < 1e-5 and lo < c < hi       # the two fp32 neighbours
    assert (t <= -87).sum() >= 6 and t.min() <= -104 + 1e-3
    # exp(100 z) goes subnormal and then to zero inside that stratum
    assert float(np.float32(math.exp(-87.0))) > 2.0 ** -126 > float(np.float32(math.exp(-88.8))) > 0.0 == np.float32(math.exp(-104.0))
    # every stratum in every 32-column tile and in the ragged last tile, over the 22 rotations
    for width in B.PROBE_FUSED_WIDTHS + B.PROBE_UNFUSED_WIDTHS:
        seen = {}
        for rot in range(len(z)):
            zz = B.probe_layers(width, rot, relu=False)[4].numpy()
            for j in range(width):
                seen.setdefault(j, set()).add(float(zz[j]))
        assert all(len(v) == len(set(z.tolist())) for v in seen.values()), width


@pytest.mark.parametrize("width", B.PROBE_FUSED_WIDTHS + B.PROBE_UNFUSED_WIDTHS)
def test_activation_probe_expected_values(width):
    """With one live point, d_bias of layer 0 IS zbar_j = s1 abar + s2 zdot adotbar per column, and d_weight row j is
    zbar_j x + s1 adotbar v: the reference's autograd agrees with the closed form, in fp32 within the bound the device gets."""
    for rot in (0, 7):
        W0, b0, W1, b1, z, asserted = B.probe_layers(width, rot, relu=False)
        assert float((W0.double() @ torch.tensor(B.PROBE_X, dtype=torch.float64)).abs().max()) == 0.0   # z = bias, exactly
        r64 = B.probe_reference(W0, b0, W1, b1, False, True, torch.float64)
        r32 = B.probe_reference(W0, b0, W1, b1, False, True, torch.float32)
        zd = z.double()
        s1 = torch.sigmoid(100 * zd)
        s2 = 100 * s1 * (1 - s1)
        thr = 100 * zd > 20
        s1, s2 = torch.where(thr, torch.ones_like(s1), s1), torch.where(thr, torch.zeros_like(s2), s2)
        zdot = W0.double() @ torch.tensor(B.PROBE_V, dtype=torch.float64)
        zbar = s1 * B.PROBE_D_SDF * W1[0].double() + s2 * zdot * W1[0].double()
        assert torch.allclose(r64["b0"], zbar, rtol=1e-12, atol=1e-300)
        w = zbar[:, None] * torch.tensor([B.PROBE_X], dtype=torch.float64) + (s1 * W1[0].double())[:, None] * torch.tensor([B.PROBE_V], dtype=torch.float64)
        assert torch.allclose(r64["w0"], w, rtol=1e-12, atol=1e-300)
        bb, bw = B.probe_bounds(W0, W1, r64, r32, True)
        assert bool(((r32["b0"].double() - r64["b0"]).abs() <= bb).all()) and bool((bb > 0).all())
        assert bool(((r32["w0"].double() - r64["w0"]).abs().max(dim=1).values <= bw).all())
        # the closed form the fused epilogue uses above the threshold, s2 = 100 u / (1 + u)^2, is not 0 there but stays inside the bound
        u = torch.exp(-100 * zd[thr])
        assert bool((100 * u * zdot[thr].abs() * W1[0].double().abs()[thr] <= bb[thr] / B.MARGIN).all())
    # relu: asserted columns and the kink share
    W0, b0, W1, b1, z, asserted = B.probe_layers(width, 1, relu=True)
    assert 0 < int((~asserted).sum()) <= B.KINK_CAP * width
    assert set(np.abs(z[asserted].numpy()).tolist()) == {float(np.float32(1e-3)), 1.0}
    assert set(np.abs(z[~asserted].numpy()).tolist()) == {2.0 ** -126}
    r = B.probe_reference(W0, b0, W1, b1, True, False, torch.float64)
    assert torch.equal(r["b0"], torch.where(z.double() > 0, B.PROBE_D_SDF * W1[0].double(), torch.zeros(width, dtype=torch.float64)))


def test_operand_scale_bound_follows_the_split():
    assert B.gemm_scale(1.0e3) == 16.0 and B.gemm_scale(1.0) == 2.0 ** 13 and B.gemm_scale(3e-7) == 2.0 ** 35
    h = torch.tensor([0.5, 1e-3], dtype=torch.float64)
    for k in B.SCALE_KS:
        d = B.SCALE_A * 2.0 ** -k
        b = B.scale_bound(h, h.float(), d, B.SCALE_A)
        # relative to the product it is 2^-20-ish while both pieces are normal, and grows once s d sinks into fp16's subnormals
        rel = float(b[0] / (d * 0.5))
        assert rel >= 2.0 ** -22
        if 16.0 * d >= 2.0 ** -14:
            assert rel <= 2e-5 + 4 * 2.0 ** -22
