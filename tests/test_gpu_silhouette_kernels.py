"""The kernels of the silhouette and hole-filling path (fill_holes=True, handle_edges=True), one operator at a time against
oracle/iron_ref.py evaluated in fp64 from the same fp32 inputs (tests/_silhouette_oracle.py): iron_camera_rays,
iron_intersect_sphere, iron_fill_holes, iron_edge_pixels, iron_edge_sides, iron_edge_blend (csrc/pointwise.hip), the fused surface
walk iron_edge_walk / k_edge_walk_h2 (csrc/shade.hip) and the per-step fallback walk of locate_edge_points.

The rule is |kernel - fp64| <= 4 x floor + 1e-7, the floor being the deviation of torch's fp32 CPU evaluation of the same formula
from its fp64 one on the block of rows at hand, computed here from the reference alone.  Discrete decisions no fp32 evaluation can
reproduce -- the sign of a grazing ray's discriminant, a uv within delta of a pixel border, a walk step whose |n.v| came within 1e-4
of the threshold -- are flagged from the fp64 side and excused; tests/test_silhouette_oracle.py pins their caps on the CPU, and that
the oracle's own fp32 evaluation meets every comparison made here.  Bit-exact where the operation is a copy, a product or a choice.

A block of a handful of rows (the n = 1 cases) takes its floor from the same builder's larger draw (_silhouette_oracle.check_blocks).

Lines starting with "sil-k" carry the measured figures.  On an MI355X (256 CUs), worst case of each row
(columns: operator | block | fp32 floor | kernel error | ratio = error / (4 floor + 1e-7)):

  operator | block | fp32 floor | kernel error | ratio
  iron_camera_rays, 4 cameras, n = 1 / 255 / 257 / 524 545: ray_d | centre / off‑centre | 1.1e‑7 / 1.3e‑7 | 1.2e‑7 / 1.3e‑7 | 0.29
  ray_d_norm; ray_o; ‖ray_d‖ − 1 |  | 1.8e‑7; 0; — | 1.8e‑7; 0 (bit‑equal); 1.23 ulp (bound 2) | 0.22; 0; —
  iron_intersect_sphere, r = 0.5 / 1 / 1.2: near / far | regular | 4.5e‑7 … 1.6e‑6 | 5.0e‑7 … 1.7e‑6 | 0.36
   | grazing, b = r (1 ± 1e‑2 … 1e‑7) | 1.0e‑4 … 1.2e‑3 | the same | 0.25
  mask | 16–33 % of the grazing block flagged, none outside it |  | 0 differences unflagged (1 319 of 58 283 flagged rows differ at n = 524 545) | 
  iron_fill_holes, 1×1 / 3×5 / 17×67, cases a b c and the wrapper | depth, mask, distance, flag | bit‑equal | bit‑equal | 
   | points |  | 1.48 ulp of the larger addend (bound 2) | 
  iron_edge_pixels, 8² and 56², n = 1 / 63 / 300 / 70 000: uv | in front / behind | 3.8e‑6 (8²), 2.1e‑5 (56²) | 2.6e‑6, 1.5e‑5 | 0.25
  first | ≤ 51 candidates of 70 000 flagged, ≤ 12 of 3 136 pixels excused |  | equal on every compared pixel; wrap‑around rows accepted | 
  iron_edge_sides, n = 1 / 130: side uv | generic / edge rows / projected length ≥ 1e‑3 | 2.9e‑6 / 8.0e‑7 / 6.9e‑6 | 2.9e‑6 / 8.0e‑7 / 1.0e‑5 | 0.25 / 0.24 / 0.37
  weight | the same | 8.0e‑8 / 3.7e‑8 / 5.3e‑6 | 1.0e‑7 / 3.7e‑8 / 7.6e‑6 | 0.25 / 0.15 / 0.36
  iron_edge_blend, n = 1 / 130 | colour; normal, uv, points, untouched pixels |  | 0.95 ulp (bound 2); bit‑equal | 
  k_edge_walk_h2, n = 1 / 31 / 33 / 300, max_step 0 / 1 / 16, both fields | decided candidates (≥ 298 of 300) | 0 / 2.8e‑8 … 3.0e‑8 / 1.1e‑7 … 1.3e‑7 | 0 / 2.8e‑8 … 3.0e‑8 / 1.1e‑7 … 1.3e‑7 | 0 / 0.14 / 0.21
  random and tile‑sorted order; permutation and repeat |  |  | as above; bit‑equal | 0.21
  n = 32 × 256 + 33 = 8 225 on bumpy03_s1, also tile‑sorted | 8 174 decided | 1.7e‑7 | 3.8e‑7 | 0.48
  fallback walk (exact core) through locate_edge_points | matched points | as the fused walk | 7.7e‑8 | 0.14
"""
import functools

import pytest
import torch

import _hard_fields as HF
import _silhouette_oracle as S
from oracle import iron_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
NONE = 2 ** 31 - 1   # iron_edge_pixels: no candidate in this pixel


def _L():
    from iron_amd import _lib
    return _lib


def _dev():
    return torch.device("cuda", 0)


def cu(x):
    return x.to(_dev()).contiguous()


def product_camera(spec):
    """iron_amd's Camera on the oracle camera's K and W2C; its fp32 inverses are the oracle's, bit for bit."""
    from iron_amd.raytracer import Camera
    cam = Camera(spec.W, spec.H, cu(spec.K), cu(spec.W2C))
    assert torch.equal(cam.K_inv.cpu(), spec.K_inv) and torch.equal(cam.C2W.cpu(), spec.C2W)
    return cam


def _rule(tag, got, ref64, dev, blocks, pop=None):
    worst = S.check_blocks(tag, got, ref64, dev, blocks, pop)
    assert worst <= 1.0, (tag, worst)
    return worst


# ---- 1. Camera.get_rays / iron_camera_rays ------------------------------------------------------------------------------------------
def _check_rays(tag, spec, uv, blocks):
    n = uv.shape[0]
    o, d, dn = product_camera(spec).get_rays(cu(uv))
    torch.cuda.synchronize()
    assert o.shape == (n, 3) and d.shape == (n, 3) and dn.shape == (n,)
    hi, lo = S.get_rays(spec, uv, F64), S.get_rays(spec, uv, F32)
    dev = S.deviation(lo, hi)
    pop = S.rays_pop(spec) if n < S.POP_RAYS else None                           # few rows: floors from the 255-row draw (check_blocks)
    for k, got in (("ray_d", d), ("ray_d_norm", dn), ("ray_o", o)):
        _rule("rays %s %s" % (tag, k), got, hi[k], dev[k], blocks, pop and (pop[0][k], pop[1]))
    unit = float(((d.cpu().double().norm(dim=-1) - 1.0).abs() / 2.0 ** -23).max())
    print("sil-k rays %s |ray_d| - 1: %.2f ulp" % (tag, unit))
    assert unit <= 2.0
    assert torch.equal(o.cpu(), spec.C2W[:3, 3].view(1, 3).expand(n, 3))        # the same origin in every row, the matrix column itself


@pytest.mark.parametrize("name", ["yaw0", "yaw135", "crop", "resized"])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_camera_rays(name, n):
    spec = S.ray_cameras()[name]
    uv, blocks = S.ray_uv(spec, n)
    _check_rays("%s n=%d" % (name, n), spec, uv, blocks)


def test_camera_rays_second_grid_stride_trip():
    spec = S.ray_cameras()["resized"]
    uv, blocks = S.ray_uv(spec, S.BIG_N)
    _check_rays("resized n=%d" % S.BIG_N, spec, uv, blocks)


# ---- 2. intersect_sphere ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,n", S.SPHERE_CASES)
def test_intersect_sphere(r, n):
    from iron_amd.raytracer import intersect_sphere
    o, d, blocks = S.sphere_rays(r, n)
    mask, near, far = intersect_sphere(cu(o), cu(d), r)
    torch.cuda.synchronize()
    mask, near, far = mask.cpu(), near.cpu(), far.cpu()
    hi = S.run_as(F64, S.intersect_sphere_parts, o, d, S.r32(r))
    lo = S.run_as(F32, S.intersect_sphere_parts, o, d, S.r32(r))
    flag = S.sphere_flags(o, d, r, blocks)
    assert not bool((flag & ~blocks["grazing"]).any())
    assert mask.dtype == torch.bool and torch.equal(mask[~flag], hi["mask"][~flag])
    print("sil-k sphere r=%g n=%d mask: %d rows flagged, %d of them differ" % (r, n, int(flag.sum()), int((mask != hi["mask"]).sum())))
    dev = S.deviation(lo, hi)
    pop = S.sphere_pop(r) if n < S.POP_SPHERE else None
    _rule("sphere r=%g n=%d near" % (r, n), near, hi["near"], dev["near"], blocks, pop and (pop[0]["near"], pop[1]))
    _rule("sphere r=%g n=%d far" % (r, n), far, hi["far"], dev["far"], blocks, pop and (pop[0]["far"], pop[1]))
    inside = (o.double().norm(dim=-1) < 0.9 * S.r32(r)) & ~blocks["grazing"]
    assert bool((near[inside] == 0.0).all())                                     # an origin inside: near is exactly 0
    if n >= 3:
        b = S.SPHERE_NAMED["behind"]
        assert bool(mask[b]) and float(far[b]) < 0.0 and float(near[b]) == 0.0   # the reference's quirk: far < 0 with a true mask
        assert int(inside.sum()) > 0


# ---- 3. iron_fill_holes / fill_depth_holes ----------------------------------------------------------------------------------------------
def _fill_call(res, closed):
    L = _L()
    g = {k: cu(v.clone()) for k, v in res.items()}
    zc = cu(closed)
    flag = torch.full((1,), 7, dtype=torch.int32, device=_dev())
    n = closed.numel()
    with torch.cuda.device(_dev()):
        L.check(L.load().iron_fill_holes(zc.data_ptr(), g["ray_o"].data_ptr(), g["ray_d"].data_ptr(), g["ray_d_norm"].data_ptr(), n,
                                         g["depth"].data_ptr(), g["convergent_mask"].data_ptr(), g["distance"].data_ptr(),
                                         g["points"].data_ptr(), flag.data_ptr(), L.stream_ptr(_dev())))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in g.items()}, int(flag.item())


def _check_filled(tag, res, closed, got, flag):
    want = S.fill_rule(res, closed)                                               # fp32: copies, a comparison and one product
    assert flag == want["flag"], tag
    assert torch.equal(got["convergent_mask"], want["convergent_mask"])
    assert torch.equal(got["depth"], want["depth"]) and torch.equal(got["distance"], want["distance"])
    for k in ("ray_o", "ray_d", "ray_d_norm"):
        assert torch.equal(got[k], res[k])
    if not flag:
        assert torch.equal(got["points"], res["points"])                          # all four buffers as they were
        return
    assert torch.equal(got["convergent_mask"], closed > torch.tensor(1e-2, dtype=F32))
    new = (closed > S.HIT_DEPTH) & ~res["convergent_mask"]
    assert torch.equal(got["depth"][new], closed[new]) and torch.equal(got["depth"][~new], res["depth"][~new])
    assert torch.equal(got["distance"], got["depth"] * res["ray_d_norm"])        # at every pixel, old hits included
    assert not torch.equal(got["distance"], res["distance"])
    t = got["distance"].double().unsqueeze(-1)
    add = res["ray_d"].double() * t
    ref = res["ray_o"].double() + add
    ulps = ((got["points"].double() - ref).abs() / S.ulp32(torch.maximum(res["ray_o"].double().abs(), add.abs()))).max()
    print("sil-k fill %s points: %.2f ulp of the larger addend" % (tag, float(ulps)))
    assert float(ulps) <= 2.0


@pytest.mark.parametrize("shape", S.FILL_SHAPES)
@pytest.mark.parametrize("case", S.FILL_CASES)
def test_fill_holes(shape, case):
    res, closed, special = S.fill_inputs(shape, case)
    got, flag = _fill_call(res, closed)
    _check_filled("%dx%d %s" % (shape + (case,)), res, closed, got, flag)
    if case == "a" or (case == "c" and shape == (1, 1)):
        assert flag == 0
        for k in ("depth", "convergent_mask", "distance", "points"):
            assert torch.equal(got[k], res[k]), k
    else:
        assert flag == 1
    if case == "c" and shape != (1, 1):
        m = got["convergent_mask"].view(-1)
        assert not bool(m[special["loses_mask"]]) and not bool(m[special["exact_hit"]]) and not bool(m[special["exact_hole"]])


@pytest.mark.parametrize("shape", [(3, 5), (17, 67)])
def test_fill_depth_holes_wrapper(shape):
    """fill_depth_holes = the closing (pinned bit-exact elsewhere) + iron_fill_holes on a depth image with real holes."""
    from iron_amd.raytracer import fill_depth_holes
    res, _, _ = S.fill_inputs(shape, "b")
    gen = torch.Generator().manual_seed(shape[0])
    res["convergent_mask"] = torch.rand(shape, generator=gen) < 0.8
    res["depth"] = res["convergent_mask"].float() * (0.5 + torch.rand(shape, generator=gen))
    closed = R.morph_closing3x3(res["depth"])
    assert bool(((closed > S.HIT_DEPTH) & ~res["convergent_mask"]).any())
    g = {k: cu(v.clone()) for k, v in res.items()}
    fill_depth_holes(g)
    torch.cuda.synchronize()
    _check_filled("wrapper %dx%d" % shape, res, closed, {k: v.cpu() for k, v in g.items()}, 1)


# ---- 4. iron_edge_pixels and the tail of locate_edge_points -----------------------------------------------------------------------------
def _edge_pixels_call(cam, pts, found):
    L = _L()
    n = pts.shape[0]
    gp, gf = cu(pts), cu(found.to(torch.uint8))
    uv = torch.full((n, 2), -7.0, device=_dev())
    first = torch.full((cam.H * cam.W,), NONE, dtype=torch.int32, device=_dev())
    with torch.cuda.device(_dev()):
        L.check(L.load().iron_edge_pixels(gp.data_ptr(), gf.data_ptr(), n, cam._w2c_host16, cam._k_host16, cam.H, cam.W, uv.data_ptr(),
                                          first.data_ptr(), L.stream_ptr(_dev())))
    torch.cuda.synchronize()
    first = first.cpu().long()
    return uv.cpu(), torch.where(first == NONE, torch.full_like(first, n), first)


@pytest.mark.parametrize("res", S.EDGE_PIXEL_IMAGES)
@pytest.mark.parametrize("n", S.EDGE_PIXEL_N)
def test_edge_pixels(res, n):
    spec, pts, found, blocks = S.edge_pixel_inputs(res, n)
    tr = S.edge_pixel_truth(spec, pts, found, blocks)
    uv, first = _edge_pixels_call(product_camera(spec), pts, found)
    pop = S.edge_pixels_pop(res) if n < S.POP_EDGE_PIXELS else None
    _rule("edge uv %dx%d n=%d" % (res, res, n), uv, tr.uv64, tr.dev, blocks, pop)  # every candidate, found or not
    keep = ~tr.excused
    print("sil-k edge first %dx%d n=%d: %d of %d pixels compared, %d taken, %d candidates flagged"
          % (res, res, n, int(keep.sum()), res * res, int((tr.winner < n).sum()), int(tr.flagged.sum())))
    assert torch.equal(first[keep], tr.winner[keep])
    assert not bool(((first < n) & ~found[first.clamp(max=n - 1)]).any())          # a candidate that was not found never wins
    if n >= 2:
        for row in S.WRAP_ROWS.values():                                           # the flat-index quirk: accepted, as in the reference
            pix = int(S.pixel_of(tr.uv64[row:row + 1], spec)[0])
            assert pix >= 0 and int(first[pix]) == row


@pytest.mark.parametrize("n", [1, 300, 70000])
def test_locate_edge_points_tail(n):
    """locate_edge_points with the walk made inert (max_step = 0, a threshold every |n.v| passes): its pixels ascend and are the
    mask's, its points and uv are the winning candidate's rows, bit for bit."""
    from iron_amd.raytracer import locate_edge_points
    spec, pts, _, blocks = S.edge_pixel_inputs(56, n)
    cam = product_camera(spec)
    found = torch.ones(n, dtype=torch.bool)
    tr = S.edge_pixel_truth(spec, pts, found, blocks)
    uv, first = _edge_pixels_call(cam, pts, found)
    out = locate_edge_points(cam, cu(pts), _net("bumpy03_s1", False, "tail"), 0, S.WALK_STEP, 2.0)
    torch.cuda.synchronize()
    idx = out["edge_pixel_idx"].cpu()
    assert idx.dtype == torch.long and bool((idx[1:] > idx[:-1]).all())
    assert torch.equal(idx, out["edge_mask"].cpu().reshape(-1).nonzero().reshape(-1))
    assert torch.equal(idx, (first < n).nonzero().reshape(-1))
    win = first[idx]
    assert torch.equal(out["edge_points"].cpu(), pts[win]) and torch.equal(out["edge_uv"].cpu(), uv[win])
    keep = ~tr.excused[idx]
    assert torch.equal(win[keep], tr.winner[idx][keep]) and int(keep.sum()) >= int(0.9 * idx.numel())


# ---- 5. iron_edge_sides ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 130])
def test_edge_sides(n):
    L = _L()
    spec, uv, g, kind, rows = S.edge_sides_inputs(n)
    cam = product_camera(spec)
    guv, gg = cu(uv), cu(g)
    side = torch.full((2 * n, 2), -7.0, device=_dev())
    w = torch.full((n,), -7.0, device=_dev())
    with torch.cuda.device(_dev()):
        L.check(L.load().iron_edge_sides(guv.data_ptr(), gg.data_ptr(), cam._w2c_rot_host, n, side.data_ptr(), w.data_ptr(), L.stream_ptr(_dev())))
    torch.cuda.synchronize()
    side, w = side.cpu(), w.cpu()
    hi, lo = S.run_as(F64, S.edge_sides, uv, g, spec.W2C), S.run_as(F32, S.edge_sides, uv, g, spec.W2C)
    dev = S.deviation(lo, hi)
    well = hi["plen"] >= S.ILL_COMPARED
    blocks = {"generic": kind == 0, "edge rows": kind == 1, "ill-conditioned, length >= 1e-3": (kind == 2) & well}
    # the [2n, 2] layout: the n positive-side samples (centre - radius n2d) first, then the n negative-side ones
    pop = S.sides_pop() if n < S.POP_SIDES else None
    _rule("sides n=%d pos_uv" % n, side[:n], hi["pos_uv"], dev["pos_uv"], blocks, pop and (pop[0]["pos_uv"], pop[1]))
    _rule("sides n=%d neg_uv" % n, side[n:], hi["neg_uv"], dev["neg_uv"], blocks, pop and (pop[0]["neg_uv"], pop[1]))
    _rule("sides n=%d weight" % n, w, hi["weight"], dev["weight"], blocks, pop and (pop[0]["weight"], pop[1]))
    assert bool(torch.isfinite(side).all()) and bool(torch.isfinite(w).all())
    centre = torch.floor(uv) + 0.5
    reach = torch.maximum((side[:n] - centre).double().norm(dim=-1), (side[n:] - centre).double().norm(dim=-1))
    assert float(reach.max()) <= S.RADIUS + 1e-5
    assert float(w.min()) >= 0.5 - 1e-6 and float(w.max()) <= 1.0
    if n > 1:
        assert int(((kind == 2) & ~well).sum()) >= 6 * S.ILL_ANGLES and int(((kind == 2) & well).sum()) >= 2 * S.ILL_ANGLES
        z = rows["zero"][0]
        assert torch.equal(side[z], centre[z]) and torch.equal(side[n + z], centre[z]) and abs(float(w[z]) - 0.5) <= 1e-7
        assert all(float(w[i]) == 1.0 for i in rows["ratio_ge_1"])
        assert all(abs(float(w[i]) - 0.5) <= 1e-7 for i in rows["on_centre"] + rows["against_normal"])


# ---- 6. iron_edge_blend ---------------------------------------------------------------------------------------------------------------
def _blend_case(tag, b, n, n_pixels):
    L = _L()
    gen = torch.Generator().manual_seed(n + n_pixels)
    before = {"color": torch.randn(n_pixels, 3, generator=gen), "normal": torch.randn(n_pixels, 3, generator=gen),
              "uv": torch.randn(n_pixels, 2, generator=gen), "points": torch.randn(n_pixels, 3, generator=gen)}
    g = {k: cu(v.clone()) for k, v in before.items()}
    i = {k: cu(v) for k, v in b.items()}
    with torch.cuda.device(_dev()):
        L.check(L.load().iron_edge_blend(i["side_color"].data_ptr(), i["weight"].data_ptr(), i["grads"].data_ptr(), i["edge_uv"].data_ptr(),
                                         i["edge_points"].data_ptr(), i["pixel"].data_ptr(), n, n_pixels, g["color"].data_ptr(),
                                         g["normal"].data_ptr(), g["uv"].data_ptr(), g["points"].data_ptr(), L.stream_ptr(_dev())))
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in g.items()}
    pixel = b["pixel"]
    valid = (pixel >= 0) & (pixel < n_pixels)
    untouched = torch.ones(n_pixels, dtype=torch.bool)
    untouched[pixel[valid]] = False
    for k in before:
        assert torch.equal(got[k][untouched], before[k][untouched]), k            # skipped rows included: nothing is written for them
    p = pixel[valid]
    assert torch.equal(got["normal"][p], b["grads"][valid]) and torch.equal(got["uv"][p], b["edge_uv"][valid])
    assert torch.equal(got["points"][p], b["edge_points"][valid])
    if bool(valid.any()):
        ref = S.blend(b["side_color"][:n].double(), b["side_color"][n:].double(), b["weight"].double())[valid]
        ulps = float(((got["color"][p].double() - ref).abs() / S.ulp32(ref)).max())
        print("sil-k blend %s colour: %.2f ulp" % (tag, ulps))
        assert ulps <= 2.0
    return int(valid.sum())


def test_edge_blend():
    b = S.edge_blend_inputs(130, 200)
    assert int((b["pixel"] == -1).sum()) == 1 and int((b["pixel"] == 200).sum()) == 1
    assert _blend_case("n=130", b, 130, 200) == 128
    for tag, pix, n_valid in (("n=1", 2, 1), ("n=1 pixel=-1", -1, 0), ("n=1 pixel=n_pixels", 5, 0)):
        one = S.edge_blend_inputs(1, 5)
        one["pixel"][0] = pix
        assert _blend_case(tag, one, 1, 5) == n_valid


# ---- 7. iron_edge_walk / k_edge_walk_h2, and the fallback walk ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net(field, exact=False, tag=""):
    """One packed network per (field, core, user): a test that feeds far-away points keeps an instance of its own."""
    net = HF.build(field).to(_dev())
    if exact:
        net.force_exact(True)
    return net


def _n_cus():
    return int(_L().load().iron_set_cu_limit(0))   # lifts any limit and returns the device's CU count


def _walk_gpu(field, start, max_step):
    from iron_amd.raytracer import _edge_walk_fused
    out = _edge_walk_fused(_net(field), cu(start), S.walk_camera_origin(), max_step, S.WALK_STEP, S.WALK_THRESHOLD)
    assert out is not None, "the network is not on the h2 core"
    torch.cuda.synchronize()
    return out[0].cpu(), out[1].cpu()


def _check_walk(tag, tr, rows, pts, found):
    d = tr.decided[rows]
    assert found.dtype == torch.bool and torch.equal(found[d], tr.found[rows][d]), tag
    err = (pts.double() - tr.points[rows]).abs().max(dim=1)[0]
    floor = S.walk_floor(tr)
    e = float(err[d].max()) if bool(d.any()) else 0.0
    ratio = e / (S.FACTOR * floor + S.ABS)
    print("sil-k walk %s rows=%d decided=%d floor=%.3e err=%.3e ratio=%.3f" % (tag, rows.numel(), int(d.sum()), floor, e, ratio))
    assert ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize("field", S.WALK_FIELDS)
@pytest.mark.parametrize("max_step", [0, 1, 16])
@pytest.mark.parametrize("n", [1, 31, 33, 300])
def test_edge_walk(field, max_step, n):
    tr = S.walk_truth(field, S.WALK_POOL, max_step)
    rows = torch.arange(n)
    pts, found = _walk_gpu(field, tr.start[:n], max_step)
    _check_walk("%s n=%d max_step=%d" % (field, n, max_step), tr, rows, pts, found)
    if max_step == 0:
        assert torch.equal(pts, tr.start[:n])


@pytest.mark.parametrize("field", S.WALK_FIELDS)
def test_edge_walk_orders_and_structure(field):
    """Random order and the tile-sorted order against the truth; the walk of a permuted list is the permutation of the walk and two
    runs are identical, bit for bit (candidates are independent: a cross-lane mix-up in the LDS exchange would show)."""
    tr = S.walk_truth(field, S.WALK_POOL)
    base_p, base_f = _walk_gpu(field, tr.start, S.WALK_MAX_STEP)
    again_p, again_f = _walk_gpu(field, tr.start, S.WALK_MAX_STEP)
    assert torch.equal(base_p, again_p) and torch.equal(base_f, again_f)
    orders = {"random": torch.randperm(S.WALK_POOL, generator=torch.Generator().manual_seed(5)),
              "tile-sorted": S.tile_sorted_order(tr.cls, _n_cus())}
    for name, perm in orders.items():
        pts, found = _walk_gpu(field, tr.start[perm].contiguous(), S.WALK_MAX_STEP)
        _check_walk("%s n=%d %s order" % (field, S.WALK_POOL, name), tr, perm, pts, found)
        assert torch.equal(pts, base_p[perm]) and torch.equal(found, base_f[perm]), name


def test_edge_walk_second_tile_of_a_workgroup():
    """n = 32 x CUs + 33: the grid is one workgroup per CU, so workgroups 0 and 1 take a second tile and the last tile holds a single
    candidate; in the tile-sorted order those second tiles are of the class opposite to the first."""
    cus = _n_cus()
    n = S.walk_big_n(cus)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    tr = S.walk_truth("bumpy03_s1", n)
    base_p, base_f = _walk_gpu("bumpy03_s1", tr.start, S.WALK_MAX_STEP)
    _check_walk("bumpy03_s1 n=%d (CUs=%d)" % (n, cus), tr, torch.arange(n), base_p, base_f)
    perm = S.tile_sorted_order(tr.cls, cus)
    pts, found = _walk_gpu("bumpy03_s1", tr.start[perm].contiguous(), S.WALK_MAX_STEP)
    _check_walk("bumpy03_s1 n=%d tile-sorted order" % n, tr, perm, pts, found)
    assert torch.equal(pts, base_p[perm]) and torch.equal(found, base_f[perm])


FALLBACK_RES = 2048   # pixels of the camera the fallback cases project with: candidates 1e-2 apart land in pixels of their own


@pytest.mark.parametrize("field", S.WALK_FIELDS)
@pytest.mark.parametrize("max_step", [0, 1, 16])
def test_fallback_walk_through_locate_edge_points(field, max_step):
    """force_exact() takes the network off the h2 core: iron_edge_walk answers IRON_ERR_UNSUPPORTED (its h2_sdf_usable test) and
    locate_edge_points walks with one get_all launch per step.  It returns one point per pixel, so the candidates are projected with
    a 2048 x 2048 camera of the same pose and every returned point is matched to the nearest final point of the fp64 walk: it must lie
    within the rule of a candidate the truth found (or an undecided one), and every decided, found candidate alone in a pixel it is
    well inside of must be returned."""
    from iron_amd.raytracer import _edge_walk_fused, locate_edge_points
    net = _net(field, True)
    tr = S.walk_truth(field, S.WALK_POOL, max_step)
    spec = S.fixture_camera(FALLBACK_RES, FALLBACK_RES)
    cam = product_camera(spec)
    assert torch.equal(spec.C2W[:3, 3], tr.cam_o)
    assert _edge_walk_fused(net, cu(tr.start[:33]), tr.cam_o, max_step, S.WALK_STEP, S.WALK_THRESHOLD) is None
    tol = S.FACTOR * S.walk_floor(tr) + S.ABS
    for n in (1, 31, 33, 300):
        out = locate_edge_points(cam, cu(tr.start[:n]), net, max_step, S.WALK_STEP, S.WALK_THRESHOLD)
        torch.cuda.synchronize()
        got = out["edge_points"].cpu().double()
        truth, found, decided = tr.points[:n], tr.found[:n], tr.decided[:n]
        matched = torch.zeros(n, dtype=torch.bool)
        worst = 0.0
        if got.shape[0] > 0:
            dist, j = (got[:, None, :] - truth[None, :, :]).abs().max(dim=-1)[0].min(dim=1)
            matched[j] = True
            dec = decided[j]
            assert bool(found[j][dec].all()), "a candidate the truth never finds was returned"
            worst = float(dist[dec].max()) if bool(dec.any()) else 0.0
        uv = S.project(spec, truth.float(), F64)
        pix = S.pixel_of(uv, spec)
        clear = ((uv - torch.round(uv)).abs() > 0.02).all(dim=1) & (pix >= 0)
        alone = torch.tensor([int((pix[found | ~decided] == p).sum()) == 1 for p in pix.tolist()], dtype=torch.bool)
        due = found & decided & clear & alone
        print("sil-k fallback %s n=%d max_step=%d returned=%d due=%d of %d found err=%.3e ratio=%.3f"
              % (field, n, max_step, got.shape[0], int(due.sum()), int((found & decided).sum()), worst, worst / tol))
        assert worst <= tol
        assert bool(matched[due].all()), "a found candidate is missing"
        if n >= 31 and max_step > 0:
            assert 2 * int(due.sum()) >= int((found & decided).sum()) > 0      # the completeness check is not vacuous
