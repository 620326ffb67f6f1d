"""The high-precision side of tests/test_gpu_silhouette_kernels.py, checked on the CPU from the reference alone: every formula that
tests/_silhouette_oracle.py restates equals the oracle's own function in fp64 on the same inputs; the caps hold (flagged pixel
candidates, undecided walk candidates, no sphere flag outside the grazing block); every walk input offers each of the three classes;
and the oracle's fp32 evaluation meets every comparison the GPU file makes, so a failing kernel cannot be blamed on the inputs."""
from types import SimpleNamespace

import pytest
import torch

import _silhouette_oracle as S
from oracle import iron_ref as R


# ---- the restatements are the oracle's formulas ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r", S.SPHERE_RADII)
def test_intersect_sphere_parts_is_the_oracle(r):
    o, d, blocks = S.sphere_rays(r, 255)
    for dtype in (torch.float64, torch.float32):
        mine = S.run_as(dtype, S.intersect_sphere_parts, o, d, S.r32(r))
        mask, near, far = S.run_as(dtype, R.intersect_sphere, o, d, S.r32(r))
        assert torch.equal(mine["mask"], mask) and torch.equal(mine["near"], near) and torch.equal(mine["far"], far)
        assert mine["near"].dtype == dtype
    hi = S.run_as(torch.float64, S.intersect_sphere_parts, o, d, S.r32(r))
    c, i, b = (S.SPHERE_NAMED[k] for k in ("through_centre", "inside_origin", "behind"))
    assert abs(float(hi["tmp"][c]) - S.r32(r) ** 2) < 1e-6                      # through the centre: p = 0
    assert float(hi["near"][i]) == 0.0 and bool(hi["mask"][i]) and float(hi["far"][i]) > 0
    assert float(hi["far"][b]) < 0 and bool(hi["mask"][b])                       # the sphere behind the origin: far < 0, mask true
    lengths = d.double().norm(dim=-1)
    assert all(bool(((lengths - v).abs() < 1e-5).any()) for v in (0.5, 1.0, 3.0))
    graze = blocks["grazing"]
    assert 0.3 < float(hi["mask"][graze].double().mean()) < 0.7                  # both sides of the sphere's rim
    assert 0.2 < float(hi["mask"][~graze].double().mean()) < 0.9
    assert bool((o[~graze].double().norm(dim=-1) < S.r32(r)).any())              # origins inside the sphere


@pytest.mark.parametrize("shape", S.FILL_SHAPES)
@pytest.mark.parametrize("case", S.FILL_CASES)
def test_fill_rule_is_the_oracle(shape, case):
    res, closed, special = S.fill_inputs(shape, case)
    real = R.raytrace_camera, R.morph_closing3x3
    for dtype in (torch.float64, torch.float32):
        cast = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in res.items()}
        mine = S.fill_rule(cast, closed.to(dtype))
        R.raytrace_camera = lambda scene, cam, max_num_rays=0, prm=None: {k: v.clone() for k, v in cast.items()}
        R.morph_closing3x3 = lambda depth: closed.to(dtype)
        try:
            ref = R.raytrace_camera_full(None, None, fill_holes=True)
        finally:
            R.raytrace_camera, R.morph_closing3x3 = real
        for k in ("depth", "convergent_mask", "distance", "points"):
            assert torch.equal(mine[k], ref[k]), k
    upd = (closed > S.HIT_DEPTH) & ~res["convergent_mask"]
    single_c = case == "c" and shape == (1, 1)
    assert mine["flag"] == int(case != "a" and not single_c) == int(bool(upd.any()))
    if case == "a":
        assert bool((res["convergent_mask"] & (closed <= S.HIT_DEPTH)).any()) or shape == (1, 1)   # hits that WOULD lose their mask
    if case == "c" and not single_c:
        flat = mine["convergent_mask"].view(-1)
        assert not bool(flat[special["loses_mask"]]) and not bool(flat[special["exact_hit"]]) and not bool(flat[special["exact_hole"]])
        assert bool(res["convergent_mask"].view(-1)[special["loses_mask"]])
        assert float(closed.view(-1)[special["exact_hit"]]) == float(torch.tensor(1e-2, dtype=torch.float32))


@pytest.mark.parametrize("n", [1, 130])
def test_edge_sides_and_blend_are_the_oracle(n):
    cam, uv, g, kind, rows = S.edge_sides_inputs(n)
    b = S.edge_blend_inputs(n, 200)
    pos_c, neg_c = b["side_color"][:n], b["side_color"][n:]
    for dtype in (torch.float64, torch.float32):
        mine = S.run_as(dtype, S.edge_sides, uv, g, cam.W2C)
        ref = S.oracle_edge_geometry(cam, uv, g, pos_c, neg_c, dtype)
        assert torch.equal(mine["pos_uv"], ref["pos_uv"]) and torch.equal(mine["neg_uv"], ref["neg_uv"])
        assert torch.equal(S.blend(pos_c.to(dtype), neg_c.to(dtype), mine["weight"]), ref["color"])
        ones = S.oracle_edge_geometry(cam, uv, g, torch.ones(n, 3), torch.zeros(n, 3), dtype)      # colour = the weight itself
        assert torch.equal(ones["color"][:, 0], mine["weight"])
        assert torch.equal(ref["normal"], g.to(dtype)) and torch.equal(ref["uv"], uv.to(dtype))
    if n > 1:
        hi = S.run_as(torch.float64, S.edge_sides, uv, g, cam.W2C)
        w = hi["weight"]
        assert all(abs(float(w[i]) - 0.5) < 1e-12 for i in rows["on_centre"] + rows["against_normal"] + rows["zero"])
        assert all(float(w[i]) == 1.0 for i in rows["ratio_ge_1"])
        assert all(1.0 - 1e-4 < float(w[i]) < 1.0 for i in rows["just_below_1"])
        assert all(0.5 < float(w[i]) < 0.5 + 1e-4 for i in rows["just_above_0"])
        assert all(float((uv[i].double() - (torch.floor(uv[i].double()) + 0.5)).abs().max()) < 0.5 for i in range(n))
        plen = hi["plen"][rows["ill"]].reshape(len(S.ILL_LENGTHS), S.ILL_ANGLES)
        assert torch.allclose(plen[:3], torch.tensor(S.ILL_LENGTHS[:3], dtype=torch.float64)[:, None].expand(3, S.ILL_ANGLES), rtol=1e-3)
        assert float(plen[5:].max()) < 1e-5 and float(hi["plen"][rows["zero"][0]]) == 0.0
        assert int((plen >= S.ILL_COMPARED).sum()) >= 2 * S.ILL_ANGLES
        assert float(hi["plen"][kind != 2].min()) > 1e-2                          # nothing ill-conditioned outside its block
        assert bool((uv < 0).any())


@pytest.mark.parametrize("field", S.WALK_FIELDS)
def test_walk_is_the_oracle(field):
    sd, spec = S._field(field)
    start, cam_o = S.walk_starts(field, S.WALK_POOL)[200:].contiguous(), S.walk_camera_origin()   # 68 on-surface, 32 displaced
    for dtype, max_step in ((torch.float64, 16), (torch.float64, 1), (torch.float64, 0), (torch.float32, 16)):
        pts, found, moves, margin = S.walk(sd, spec, start, cam_o, max_step, dtype)
        ref = S.oracle_walk(sd, spec, start, cam_o, max_step, dtype)
        assert pts.dtype == dtype and torch.equal(pts[found], ref), (dtype, max_step)
        assert int(moves.max()) <= max_step and bool((moves[~found] == max_step).all())
    assert torch.get_default_dtype() == torch.float32


# ---- caps and coverage ---------------------------------------------------------------------------------------------------------
def test_camera_inputs_and_fp32_oracle():
    cams = S.ray_cameras()
    assert (cams["resized"].W, cams["resized"].H) == (76, 46)
    for name, cam in cams.items():
        for n in (1, 255, 257):
            uv, blocks = S.ray_uv(cam, n)
            hi, lo = S.get_rays(cam, uv, torch.float64), S.get_rays(cam, uv, torch.float32)
            dev = S.deviation(lo, hi)
            for k in ("ray_d", "ray_d_norm", "ray_o"):
                pop = S.rays_pop(cam)
                assert S.check_blocks("cpu rays %s n=%d %s" % (name, n, k), lo[k], hi[k], dev[k], blocks, (pop[0][k], pop[1])) <= 1.0
            assert float((hi["ray_d"].norm(dim=-1) - 1).abs().max()) < 1e-15
            if n > 1:
                assert bool((uv < 0).any()) and bool((uv[:, 0] > cam.W).any()) and bool((uv[:, 1] > cam.H).any())
                frac = uv - torch.floor(uv)
                assert bool((frac[blocks["centre"]] == 0.5).all()) and not bool((frac[blocks["off-centre"]] == 0.5).all())


@pytest.mark.parametrize("r,n", S.SPHERE_CASES)
def test_sphere_flags_stay_in_the_grazing_block(r, n):
    o, d, blocks = S.sphere_rays(r, n)
    flag = S.sphere_flags(o, d, r, blocks)
    assert not bool((flag & ~blocks["grazing"]).any())
    hi = S.run_as(torch.float64, S.intersect_sphere_parts, o, d, S.r32(r))
    lo = S.run_as(torch.float32, S.intersect_sphere_parts, o, d, S.r32(r))
    assert torch.equal(lo["mask"][~flag], hi["mask"][~flag])
    print("sphere r=%g n=%d: %d flagged, all in the grazing block of %d" % (r, n, int(flag.sum()), int(blocks["grazing"].sum())))
    if n > 1:
        assert int((~flag & blocks["grazing"]).sum()) >= int(blocks["grazing"].sum()) // 2      # the grazing block is not excused wholesale
    dev = S.deviation(lo, hi)
    for k in ("near", "far"):
        pop = S.sphere_pop(r)
        assert S.check_blocks("cpu sphere r=%g n=%d %s" % (r, n, k), lo[k], hi[k], dev[k], blocks, (pop[0][k], pop[1])) <= 1.0


@pytest.mark.parametrize("res", S.EDGE_PIXEL_IMAGES)
@pytest.mark.parametrize("n", S.EDGE_PIXEL_N)
def test_edge_pixel_flag_cap_and_fp32_oracle(res, n):
    cam, pts, found, blocks = S.edge_pixel_inputs(res, n)
    tr = S.edge_pixel_truth(cam, pts, found, blocks)
    assert bool(torch.isfinite(tr.uv64).all())
    share, expect = float(tr.flagged.double().mean()), 4.0 * float(tr.delta.max())
    print("edge pixels %dx%d n=%d: delta %.2e, flagged %.4f %% (4 delta = %.4f %%), excused pixels %d / %d"
          % (res, res, n, float(tr.delta.max()), 100 * share, 100 * expect, int(tr.excused.sum()), res * res))
    assert share <= S.CAP_PIXEL_FLAGS and share <= 2.0 * expect + 4.0 / n
    assert S.check_blocks("cpu edge uv %d n=%d" % (res, n), tr.uv32, tr.uv64, tr.dev, blocks) <= 1.0
    win32 = S.first_winner(S.pixel_of(tr.uv32.double(), cam), found, res * res)
    assert torch.equal(win32[~tr.excused], tr.winner[~tr.excused])
    assert int(tr.excused.sum()) <= max(1, res * res // 20)
    if n >= 2:  # the wrap-around rows: u < 0 with 1 <= v < H and u >= W with v < H - 1 are accepted, as in the reference
        for row in S.WRAP_ROWS.values():
            u, v = (float(x) for x in tr.uv64[row])
            assert (u < 0 and 1 <= v < res) or (u >= res and v < res - 1)
            pix = int(S.pixel_of(tr.uv64[row:row + 1], cam)[0])
            assert pix >= 0 and int(tr.winner[pix]) == row and not bool(tr.flagged[row])
        uv = tr.uv64
        assert all(bool(m.any()) for m in (uv[:, 0] < 0, uv[:, 0] >= res, uv[:, 1] < 0, uv[:, 1] >= res))
    if n >= 63:
        assert bool(blocks["behind"].any()) and bool(found.any()) and bool((~found).any())
        frac = tr.uv64 - torch.floor(tr.uv64)
        assert 0.4 < float(frac.mean()) < 0.6
    if n == 70000 and res == 8:
        assert bool((tr.winner < n).all())                    # every pixel of the small image is contended for


def test_edge_pixel_reference_quirk_and_collisions():
    """R.locate_edge_points' own tail on a handful of hand-made uv: only the flat index is range-checked, and the first candidate
    in order wins its pixel."""
    cam = S.fixture_camera(8, 8)
    uv = torch.tensor([[-2.3, 3.6], [9.4, 2.2], [3.5, 3.5], [3.2, 3.9], [-1.0, 0.5], [2.0, 8.5], [9.0, 7.5]], dtype=torch.float64)
    pix = S.pixel_of(uv, cam)
    assert pix.tolist() == [3 * 8 - 3, 2 * 8 + 9, 27, 27, -1, -1, -1]
    win = S.first_winner(pix, torch.ones(7, dtype=torch.bool), 64)
    assert int(win[27]) == 2 and int(win[21]) == 0 and int(win[25]) == 1
    upd, uidx = R.unique_first(pix[pix >= 0])
    assert upd.tolist() == [21, 25, 27] and uidx.tolist() == [0, 1, 2]


def _walk_inputs():
    for field in S.WALK_FIELDS:
        yield field, S.WALK_POOL
    yield "bumpy03_s1", S.walk_big_n(S.NOMINAL_CUS)


@pytest.mark.parametrize("field,n", list(_walk_inputs()))
def test_walk_caps_classes_and_fp32_oracle(field, n):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    tr = S.walk_truth(field, n)
    start = tr.start
    assert start.shape == (n, 3) and torch.equal(start[:31], S.walk_starts(field, 31))        # a shorter list is a prefix
    undecided = float((~tr.decided).double().mean())
    shares = [float((tr.cls == c).double().mean()) for c in range(3)]
    floor = S.walk_floor(tr)
    print("walk %s n=%d: undecided %.2f %%, classes %.1f / %.1f / %.1f %%, point floor max %.2e median %.2e, moves 0..%d"
          % (field, n, 100 * undecided, *(100 * s for s in shares), floor, float(tr.dev[tr.decided].median()), int(tr.moves.max())))
    assert undecided <= S.CAP_UNDECIDED
    for sub in (31, 33, n):
        cls = tr.cls[:sub]
        assert all(float((cls == c).double().mean()) >= 0.10 for c in range(3)), (sub, [int((cls == c).sum()) for c in range(3)])
    d = tr.decided
    assert torch.equal(tr.found32[d], tr.found[d]) and torch.equal(tr.moves32[d], tr.moves[d])
    assert float(tr.dev[d].max()) <= S.FACTOR * floor + S.ABS
    # the displaced block lies off the surface by 2e-3 and the rest on it
    sd, spec = S._field(field)
    s, _ = S._get_all(sd, spec, start[:S.WALK_POOL].double())
    lo, hi = S.WALK_POOL - S.WALK_DISPLACED, S.WALK_POOL
    assert float(s[:lo].abs().max()) <= 1e-4 and float(s[lo:hi].abs().min()) > 3e-4     # 2e-3 x |gradient|, which is not 1 on these fields
    # max_step = 0 and 1: prefixes of the same candidates
    for ms in (0, 1):
        t = S.walk_truth(field, S.WALK_POOL, ms)
        assert int(t.moves.max()) == ms and float((~t.decided).double().mean()) <= S.CAP_UNDECIDED
        dd = t.decided
        assert torch.equal(t.found32[dd], t.found[dd])
    # the tile-sorted order: whole tiles found at step 0, whole tiles never found, and the second-trip tiles opposite to the first
    perm = S.tile_sorted_order(tr.cls, S.NOMINAL_CUS)
    tiles = [tr.cls[perm][i:i + 32] for i in range(0, n, 32)]
    kinds = [int(t[0]) if bool((t == t[0]).all()) else -1 for t in tiles]
    assert kinds[0] == 0 and kinds[1] == 2 and kinds.count(0) >= 2 and kinds.count(2) >= 2
    if len(tiles) > S.NOMINAL_CUS:
        assert kinds[S.NOMINAL_CUS] == 2 and kinds[S.NOMINAL_CUS + 1] == 0


@pytest.mark.parametrize("res,n", [(8, 300), (56, 300), (8, 70000)])
def test_pixel_of_and_first_winner_are_the_oracles_tail(res, n):
    """R.locate_edge_points itself in fp64 with the walk made inert (max_step = 0, a threshold every |n.v| passes, a stand-in for the
    network): its pixels, points and uv are those of pixel_of / first_winner on the found candidates."""
    cam, pts, found, blocks = S.edge_pixel_inputs(res, n)
    tr = S.edge_pixel_truth(cam, pts, found, blocks)
    real = R.sdf_get_all
    R.sdf_get_all = lambda sd, spec, x: (torch.zeros_like(x[:, :1]), None, torch.ones_like(x))
    try:
        out = S.run_as(torch.float64, R.locate_edge_points, SimpleNamespace(sdf_sd=None, sdf_spec=None), S.cam_as(cam, torch.float64), pts, found,
                       max_step=0, dot_threshold=2.0)
    finally:
        R.sdf_get_all = real
    taken = (tr.winner < n).nonzero().reshape(-1)
    assert torch.equal(out["edge_pixel_idx"], taken) and torch.equal(out["edge_mask"].reshape(-1).nonzero().reshape(-1), taken)
    win = tr.winner[taken]
    assert torch.equal(out["edge_points"], pts.double()[win]) and torch.equal(out["edge_uv"], tr.uv64[win])
