"""The fixed summation order of csrc/fixed_sum.h ("Fixed-order fp64 sums"), pinned bit for bit against a numpy emulation.

The order, as the kernels run it and as `fixed_order_sum` below restates it:
  1. every item's value is formed in fp32, one rounding per operation (np.float32 arithmetic here);
  2. a thread adds its items to an fp64 accumulator in the order it visits them (`rule`: "span" = workgroup b owns the items
     [b * block * per_thread, (b + 1) * block * per_thread), thread t takes t, t + block, ...; "stride" = a fixed grid of `nb`
     workgroups strides over the items by nb * block);
  3. the workgroup's `block` accumulators meet in the halving tree red[t] += red[t + s], s = block / 2 .. 1 -> slot b;
  4. one workgroup adds the slots: thread t takes slots t, t + block, ... in order, then the same tree;
  5. the final fp64 expression is rounded once to fp32 where the kernel stores an fp32 scalar.
The device results must equal the emulation in their raw bits (torch.equal on integer views).

So that the comparison cannot pass whatever the order is, every case with more than one item also asserts on the host that other
orders give other bits IN THE VALUE THE DEVICE RETURNS: a plain left-to-right sum, and the same scheme with another block size and
another number of items per thread.  iron_img_sqerr returns fp64, so its fp32 cases only need terms spread over many binades (fp32
values of one binade add exactly in fp64, in any order).  The other two entries return fp32 scalars; how their inputs are built so
that the last bit of the fp64 sum decides the fp32 result is described above OTHER_ORDERS.  Nothing can be asserted, and nothing about
the order is pinned, where no order can matter: a single item or a single thread's items (B = 1), and sums of integers below 2^53 (the
uint8 squared error, mask_sum, the counts), which are exact in every order.

iron_img_sqerr is reached through image_metrics.squared_error_device where the element count is a multiple of 3 (that wrapper takes
[H, W, 3] images only); counts 1 and 262 147 are not, and call the same C entry the way the wrapper does."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32


# ---- the emulation, written once ---------------------------------------------------------------------------------------------------
def tree(red, block):
    """red [..., block] fp64 -> the halving tree's red[0]."""
    red = np.array(red, dtype=np.float64)
    s = block // 2
    while s > 0:
        red[..., :s] += red[..., s:2 * s]
        s >>= 1
    return red[..., 0]


def slot_sum(part, block):
    """thread t adds part[t], part[t + block], ... in order; then the tree."""
    part = np.asarray(part, dtype=np.float64)
    rounds = -(-len(part) // block)
    padded = np.zeros(rounds * block)
    padded[:len(part)] = part
    acc = np.zeros(block)
    for r in range(rounds):
        acc = acc + padded[r * block:(r + 1) * block]
    return tree(acc, block)


def fixed_order_sum(items, block, per_thread, rule, nb=None):
    """items [n] or [n, c] (c values per item, added in column order) -> the fp64 total in the documented order."""
    items = np.asarray(items, dtype=np.float64)
    items = items.reshape(len(items), -1)
    n = len(items)
    if rule == "span":
        span = block * per_thread
        nb = -(-n // span)
        first = (np.arange(nb) * span)[:, None] + np.arange(block)[None, :]
        step = block
    else:
        first = (np.arange(nb) * block)[:, None] + np.arange(block)[None, :]
        step = nb * block
        per_thread = -(-n // step)
    acc = np.zeros((nb, block))
    for k in range(per_thread):
        i = first + k * step
        ok = i < n
        i = np.where(ok, i, 0)
        for c in range(items.shape[1]):
            acc = acc + np.where(ok, items[i, c], 0.0)   # + 0.0 is exact: a thread without an item keeps its accumulator
    return float(slot_sum(tree(acc, block), block))


def sequential_sum(items):
    return float(np.cumsum(np.asarray(items, dtype=np.float64).reshape(-1))[-1])   # cumsum adds from left to right, one at a time


def bits(x):
    x = np.asarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])


def assert_order_matters(items, total, what):
    items = np.asarray(items).reshape(-1)
    if items.size > 1:
        assert bits(np.float64(sequential_sum(items))) != bits(np.float64(total)), "%s: a left-to-right sum gives the same bits" % what


def assert_same_bits(dev, host, what):
    dev = dev.detach().cpu().reshape(-1)
    host = torch.from_numpy(np.atleast_1d(np.asarray(host))).reshape(-1)
    assert dev.dtype == host.dtype, what
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64}[dev.dtype]
    print("%s: device %r host %r" % (what, dev.tolist(), host.tolist()))
    assert torch.equal(dev.view(view), host.view(view)), what


def wide(rng, shape, lo, hi):
    """fp32 values over many binades, u * 2^e with e in [lo, hi): fp32 values of one binade add exactly in fp64 (24 + log2(n) < 53 bits),
    and then every order gives the same bits; an fp64 sum rounds only once its terms span more than 53 bits."""
    return (rng.rand(*shape) * 2.0 ** rng.randint(lo, hi, shape)).astype(F32)


# ---- iron_img_sqerr: 1024 workgroups of 256 stride over the elements -----------------------------------------------------------------
SQERR_BLOCK, SQERR_BLOCKS = 256, 1024


def sqerr_case(count, dtype, seed):
    rng = np.random.RandomState(seed)
    if dtype == "u8":
        a = rng.randint(0, 256, count).astype(np.uint8)
        b = rng.randint(0, 256, count).astype(np.uint8)
        d = a.astype(np.int64) - b.astype(np.int64)
        items = (d * d).astype(np.float64)
        scale = 1.0 / 65025.0
    else:
        # one squared difference of 1.0, all others a quarter to a half ulp of it in fp64 (see OTHER_ORDERS below)
        a = np.sqrt((1.0 + rng.rand(count)) * 2.0 ** -56).astype(F32)
        b = -a
        if count > 1:
            a[3], b[3] = 0.75, -0.25
        d = a - b                      # fp32
        items = d * d                  # fp32: the square is rounded before it is widened
        scale = 1.0
    total = fixed_order_sum(items, SQERR_BLOCK, None, "stride", nb=SQERR_BLOCKS)
    return a, b, items, np.array([total * scale, float(count)])


def sqerr_device(a, b):
    from iron_amd import _args, _lib, image_metrics
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    n = ta.numel()
    if n % 3 == 0:
        return image_metrics.squared_error_device(ta.reshape(-1, 1, 3), tb.reshape(-1, 1, 3))
    lib = _lib.load()   # squared_error_device's own calls, for a count that is no [H, W, 3] image
    with torch.cuda.device(DEV):
        ws = _args.sized_workspace(lib.iron_img_sqerr_workspace_bytes, n, device=DEV, tag="img_sqerr")
        out = torch.empty(2, dtype=torch.float64, device=DEV)
        _lib.check(lib.iron_img_sqerr(ta.data_ptr(), tb.data_ptr(), n, int(ta.dtype == torch.float32), ws.data_ptr(), out.data_ptr(),
                                      _lib.stream_ptr(DEV)))
    return out


SQERR_CASES = [(1, "f32", 1), (255, "f32", 3), (262147, "f32", 1), (262147, "u8", 1)]


@pytest.mark.parametrize("count,dtype,seed", SQERR_CASES, ids=["%s_%d" % (d, c) for c, d, _ in SQERR_CASES])
def test_sqerr_order(count, dtype, seed):
    a, b, items, want = sqerr_case(count, dtype, seed)
    if dtype == "u8":
        assert want[0] == float(items.sum()) / 65025.0   # integers below 2^53: exact in every order, nothing to tell orders apart
    else:
        assert_order_matters(items, want[0], "sqerr %d" % count)
        if count > 1:   # and 128-thread workgroups (the same 1024 of them) give other bits too
            assert bits(np.float64(fixed_order_sum(items, 128, None, "stride", nb=SQERR_BLOCKS))) != bits(np.float64(want[0]))
    assert_same_bits(sqerr_device(a, b), want, "sqerr %s %d" % (dtype, count))


# ---- the orders the fp32 outputs must tell apart ---------------------------------------------------------------------------------------
# volume_losses and surface_regularisers return fp32 scalars, which hide the last 29 bits of an fp64 sum, and orders that differ only in
# their block size mostly agree on a sum of random terms to the last bit.  So the sums of non-negative terms are built like this: one
# term H, every other term between a quarter and a half ulp of H in fp64 -- added to H one by one such terms vanish, added to each other
# first they survive, so how many survive is decided by the block size and the items per thread -- and two tuned terms (found by
# bisection, see tune() at the end of the file) that put the total right at a rounding tie of the fp32 result, where one ulp of the fp64
# sum decides which way it rounds.  Where the inputs may be signed (cdf, weight_max) the terms cancel in pairs instead, and the total is
# the rounding residue itself.  Every such output must differ, in its fp32 bits, between the documented order and each of these:
DOCUMENTED = (256, 8)                                        # (block, items per thread)
OTHER_ORDERS = {"left to right": None, "block 128 x 16": (128, 16), "block 256 x 4": (256, 4)}
# the frame's 1023 pixels start at item 4097: four rounds of one 256-thread workgroup whether it owns 8 rounds or 4, so 256 x 4 IS the
# documented order for the roughness sum; it is told apart from 512 x 4 instead
ROUGH_OTHER_ORDERS = {"left to right": None, "block 128 x 16": (128, 16), "block 512 x 4": (512, 4)}


def ordered_sum(items, order):
    return sequential_sum(items) if order is None else fixed_order_sum(items, order[0], order[1], "span")


def assert_order_decides(want_by_order, keys, what):
    doc = want_by_order["documented"]
    for name, other in want_by_order.items():
        for k in keys if name != "documented" else ():
            assert bits(doc[k]) != bits(other[k]), "%s: %s has the same fp32 bits in the order '%s'" % (what, k, name)


def f32_from_bits(b):
    return np.array(b, dtype=np.uint32).view(F32)


def f32_bits(x):
    return int(F32(x).view(np.uint32))


def cancelling(rng, n, lo, hi):
    """n fp32 values that cancel in pairs (v at one place, -v at another): their sum is what the roundings leave."""
    v = wide(rng, (n // 2,), lo, hi)
    out = np.concatenate([v, -v, wide(rng, (n - 2 * (n // 2),), lo - 60, lo - 59)])
    return out[rng.permutation(n)]


# ---- volume_losses: one workgroup per 256 x 8 rays, six sums ----------------------------------------------------------------------------
VL_MASK_WEIGHT = 0.1
VL_CANCEL_SEED = {2049: 1, 524289: 1}   # seeds of the cancelling terms at which all four orders leave different residues
# per batch size: the ray that holds H = 1.0, and the bit patterns of the two tuned colour values (rays 5 and b - 3); all in channel 0
VL_TIE = {2049: (1130, (866232823, 612692622)), 524289: (94, (853970860, 650664194))}


def vloss_case(b, seed, tie=None, cancel_seed=None):
    rng = np.random.RandomState(seed)
    inp = {"color_fine": wide(rng, (b, 3), -30, 1), "true_rgb": wide(rng, (b, 3), -30, 1), "mask": rng.rand(b, 1).astype(F32),
           "weight_sum": (rng.rand(b, 1) * 0.98 + 0.01).astype(F32), "weight_max": wide(rng, (b, 1), -40, 1),
           "cdf_fine": wide(rng, (b, 4), -40, 1), "gradient_error": np.asarray(0.125, dtype=F32)}
    if b > 1:
        h_at, tuned = VL_TIE[b] if tie is None else tie
        inp["true_rgb"][:] = 0.0
        inp["color_fine"] = ((1.0 + rng.rand(b, 3)) * 2.0 ** -54).astype(F32)   # a quarter to a half ulp of 1.0
        for ray, value in zip((h_at, 5, b - 3), (F32(1.0),) + tuple(f32_from_bits(t) for t in tuned)):
            inp["mask"][ray] = 0.75
            inp["color_fine"][ray] = (value, 0.0, 0.0)
        inside = np.flatnonzero(inp["mask"][:, 0] > F32(0.5))
        rng = np.random.RandomState(VL_CANCEL_SEED[b] if cancel_seed is None else cancel_seed)
        inp["cdf_fine"][inside, 0] = cancelling(rng, len(inside), -45, 1)
        inp["weight_max"][inside, 0] = cancelling(rng, len(inside), -45, 1)
    return inp


def vloss_want(inp, order):
    m = (inp["mask"] > F32(0.5)).astype(F32)                         # [b, 1]
    d = inp["color_fine"] - inp["true_rgb"]
    items = {"abs": np.abs(d * m), "cdf": inp["cdf_fine"][:, :1] * m, "weight_max": inp["weight_max"] * m, "m": m}   # all fp32
    tot = {k: ordered_sum(v, order) for k, v in items.items()}
    mask_sum = tot["m"] + 1e-5
    return {"color_fine_loss": F32(tot["abs"] / mask_sum), "mask_sum": F32(mask_sum), "cdf": F32(tot["cdf"] / mask_sum),
            "weight_max": F32(tot["weight_max"] / mask_sum)}


VL_CASES = [(1, 1), (2049, 1), (524289, 1)]


@pytest.mark.parametrize("b,seed", VL_CASES, ids=["B%d" % b for b, _ in VL_CASES])
def test_volume_losses_order(b, seed):
    from iron_amd.image_losses import volume_losses
    inp = vloss_case(b, seed)
    want = vloss_want(inp, DOCUMENTED)
    if b > 1:   # one ray: one thread adds its three channels from left to right, which is the plain sum
        by_order = dict({"documented": want}, **{name: vloss_want(inp, o) for name, o in OTHER_ORDERS.items()})
        assert_order_decides(by_order, ("color_fine_loss", "cdf", "weight_max"), "volume_losses B=%d" % b)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    out = volume_losses(t["color_fine"], t["true_rgb"], t["mask"], t["weight_sum"], t["weight_max"], t["cdf_fine"], t["gradient_error"],
                        0.1, VL_MASK_WEIGHT)
    for k, v in want.items():
        assert_same_bits(out[k], v, "volume_losses B=%d %s" % (b, k))


# ---- surface_regularisers: one workgroup per 256 x 8 items of [uniform | frame | edge], six sums ---------------------------------------
REG_M, REG_H, REG_W, REG_E = 4097, 33, 31, 3
REG_N = REG_M + REG_H * REG_W + REG_E
REG_EIK_W, REG_RR_W = 0.1, 0.1
REG_SEED = 2
# (where H sits, the bit patterns of the two tuned inputs).  eik: uniform vectors (x, 0, 0), H = (2^27, 0, 0), tuned vectors 7 and 4090;
# rough: H = 2^54, tuned pixels 11 and 1000
REG_TIE = {"eik": (1133, (1153056586, 1077788510)), "rough": (768, (1303764963, 1083561462))}
REG_EIK_AT, REG_ROUGH_AT = (7, 4090), (11, 1000)


def sq_norm_error(g):
    """(|g| - 1)^2 in fp32 without contraction: ((x x + y y) + z z), a correctly rounded square root, the difference, the square."""
    g = g.astype(F32)
    s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    d = np.sqrt(s) - F32(1.0)
    return d * d


def reg_case(seed=REG_SEED, tie=None):
    tie = REG_TIE if tie is None else tie
    rng = np.random.RandomState(seed)
    n_pix = REG_H * REG_W
    # the uniform vectors (x, 0, 0) with (x - 1)^2 in [1, 2): a quarter to a half ulp of H's 2^54; roughness - 0.5 likewise
    inp = {"eik_grad": np.zeros((REG_M, 3), F32), "normal": wide(rng, (n_pix, 3), -12, 12), "mask": rng.rand(n_pix) < 0.6,
           "roughness": (1.5 + rng.rand(n_pix)).astype(F32), "edge": wide(rng, (REG_E, 3), -12, 12)}
    inp["eik_grad"][:, 0] = 1.0 + np.sqrt(1.0 + rng.rand(REG_M))
    (h_at, tuned), x = tie["eik"], inp["eik_grad"][:, 0]
    x[h_at], x[REG_EIK_AT[0]], x[REG_EIK_AT[1]] = 2.0 ** 27, f32_from_bits(tuned[0]), f32_from_bits(tuned[1])
    (h_at, tuned), r = tie["rough"], inp["roughness"]
    inp["mask"][[h_at, REG_ROUGH_AT[0], REG_ROUGH_AT[1]]] = True
    r[h_at], r[REG_ROUGH_AT[0]], r[REG_ROUGH_AT[1]] = 2.0 ** 54, f32_from_bits(tuned[0]), f32_from_bits(tuned[1])
    return inp


def reg_items(inp):
    """The four sums' terms over the concatenated index space [uniform | frame | edge], fp32."""
    n_pix = REG_H * REG_W
    sel = inp["mask"] & (inp["roughness"] > F32(0.5))
    cols = {k: np.zeros(REG_N, dtype=F32) for k in ("uniform", "masked", "edge", "rough")}
    cols["uniform"][:REG_M] = sq_norm_error(inp["eik_grad"])
    cols["masked"][REG_M:REG_M + n_pix] = np.where(inp["mask"], sq_norm_error(inp["normal"]), F32(0.0))
    cols["edge"][REG_M + n_pix:] = sq_norm_error(inp["edge"])
    cols["rough"][REG_M:REG_M + n_pix] = np.where(sel, inp["roughness"] - F32(0.5), F32(0.0))
    return cols, int(inp["mask"].sum()), int(sel.sum())


def reg_want(cols, n_mask, n_sel, order):
    tot = {k: ordered_sum(v, order) for k, v in cols.items()}
    cnt = REG_M + n_mask + REG_E
    ws = float(F32(REG_EIK_W)) / float(cnt)
    wr = float(F32(REG_RR_W)) / float(n_sel)
    return {"eik_loss": F32((tot["uniform"] + (tot["masked"] + tot["edge"])) * ws), "roughrange_loss": F32(tot["rough"] * wr),
            "counts": np.array([cnt, n_mask, n_sel], dtype=np.int64)}


def test_surface_regularisers_order():
    from iron_amd.image_losses import surface_regularisers
    inp = reg_case()
    assert -(-REG_N // (DOCUMENTED[0] * DOCUMENTED[1])) == 3   # three workgroups
    items = reg_items(inp)
    want = reg_want(*items, DOCUMENTED)
    for key, others in (("eik_loss", OTHER_ORDERS), ("roughrange_loss", ROUGH_OTHER_ORDERS)):
        by_order = dict({"documented": want}, **{name: reg_want(*items, o) for name, o in others.items()})
        assert_order_decides(by_order, (key,), "surface_regularisers")
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    eik, rr, counts = surface_regularisers(t["eik_grad"], t["normal"].reshape(REG_H, REG_W, 3), t["mask"].reshape(REG_H, REG_W),
                                           t["roughness"].reshape(REG_H, REG_W), t["edge"], REG_EIK_W, REG_RR_W, return_counts=True)
    assert_same_bits(counts, want["counts"], "surface_regularisers counts")
    assert_same_bits(rr, want["roughrange_loss"], "surface_regularisers roughrange_loss")
    assert_same_bits(eik, want["eik_loss"], "surface_regularisers eik_loss")


# ---- how H's place and the tuned terms were found (python tests/test_gpu_fixed_sums.py prints them; needs no GPU) ------------------------
def tune(out, lo, hi, item_step, others):
    """out(y, z, order) -> the fp32 result with the two tuned fp32 inputs y and z; it grows with either.  Bisection over the bit patterns
    in [lo, hi] finds the largest y that leaves the documented result where it is, then the z at which it moves on; around that z, in
    steps of half an ulp of the fp64 total (item_step(z) as a step of z), the first z at which every other order gives other bits."""
    def first_change(f, lo, hi):
        base = f(lo)
        assert f(hi) != base
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if f(mid) != base else (mid, hi)
        return hi
    val = lambda pattern: float(f32_from_bits(pattern))   # noqa: E731
    y = first_change(lambda b: out(val(b), val(lo), DOCUMENTED), lo, hi) - 1
    z0 = val(first_change(lambda b: out(val(y), val(b), DOCUMENTED), lo, y))
    for k in sorted(range(-200, 201), key=abs):
        z = F32(z0 + k * item_step(z0))
        doc = out(val(y), float(z), DOCUMENTED)
        if all(bits(out(val(y), float(z), o)) != bits(doc) for o in others.values()):
            return y, f32_bits(z)
    return None


def place_and_tune(case_items, places, out, lo, hi, item_step, others=OTHER_ORDERS):
    """Tries H at each of `places` (case_items(h_at) -> the sum's terms, which out() changes in place) until the documented total lies on
    one side of every other order's, then tunes."""
    for h_at in places:
        items = case_items(h_at)
        doc = ordered_sum(items, DOCUMENTED)
        gaps = [ordered_sum(items, o) - doc for o in others.values()]
        if all(g < 0 for g in gaps) or all(g > 0 for g in gaps):
            tuned = tune(out, lo, hi, item_step, others)
            if tuned:
                return h_at, tuned
    raise AssertionError("no place for H at which the documented order is the extreme one")


def tuned_terms():
    found, now = {}, {}
    for b, seed in VL_CASES[1:]:
        low = f32_bits(2.0 ** -80)

        def case_items(h_at, b=b, seed=seed, low=low):
            inp = vloss_case(b, seed, (h_at, (low, low)))
            m = (inp["mask"] > F32(0.5)).astype(F32)
            now["items"], now["mask_sum"] = np.abs((inp["color_fine"] - inp["true_rgb"]) * m), float(m.sum()) + 1e-5
            return now["items"]

        def out(y, z, order, b=b):
            now["items"][5, 0], now["items"][b - 3, 0] = y, z
            return F32(ordered_sum(now["items"], order) / now["mask_sum"])
        found["VL_TIE[%d]" % b] = place_and_tune(case_items, range(20, 2048, 37), out, low, f32_bits(1.0), lambda z: 2.0 ** -53)
    sq = lambda x: sq_norm_error(np.array([[x, 0, 0]], dtype=F32))[0]   # noqa: E731
    two = (f32_bits(2.0), f32_bits(2.0))
    tie = {"eik": (20, two), "rough": (20, two)}

    def case_items(key, col):
        def f(h_at):
            tie[key] = (h_at, two)
            now["reg"] = reg_items(reg_case(tie=tie))
            return now["reg"][0][col]
        return f

    def out_rough(y, z, order):
        rough = now["reg"][0]["rough"]
        rough[REG_M + REG_ROUGH_AT[0]], rough[REG_M + REG_ROUGH_AT[1]] = F32(y) - F32(0.5), F32(z) - F32(0.5)
        return reg_want(*now["reg"], order)["roughrange_loss"]

    def out_eik(y, z, order):
        uniform = now["reg"][0]["uniform"]
        uniform[REG_EIK_AT[0]], uniform[REG_EIK_AT[1]] = sq(y), sq(z)
        return reg_want(*now["reg"], order)["eik_loss"]
    # the roughness first: where its H sits decides the mask count, which the eikonal loss divides by
    tie["rough"] = place_and_tune(case_items("rough", "rough"), range(20, REG_H * REG_W, 17), out_rough, f32_bits(1.0), f32_bits(2.0 ** 55),
                                  lambda z: 2.0, ROUGH_OTHER_ORDERS)
    tie["eik"] = place_and_tune(case_items("eik", "uniform"), range(20, REG_M, 53), out_eik, f32_bits(2.0), f32_bits(2.0 ** 28),
                                lambda z: 2.0 / (2 * (z - 1)))
    found["REG_TIE"] = tie
    return found


if __name__ == "__main__":
    for name, value in tuned_terms().items():
        print(name, "=", value)
