"""volume_losses (iron_amd/image_losses.py over csrc/volume_loss.hip: iron_volume_loss) against the torch expressions of
render_volume.py:458-496 (and the statistics of :507-510) evaluated in fp64 under autograd.

Error bound (the rule of tests/test_gpu_surface_reg.py): the floor is the same expressions in fp32 on the CPU against fp64; the
HIP result is allowed 4 x that floor, and never less than 1e-6 relative to the sum of the absolute terms of the quantity -- every
scalar here is a sum of non-negative terms (or, psnr, a logarithm of one), so that is the fp64 value itself; for a gradient tensor,
whose elements are single products, its largest fp64 element.  Where autograd has an exact zero the HIP gradient is exactly zero.
Forward and backward are bitwise equal from run to run.

The clip bounds: torch clamps a float32 tensor at 1e-3 and 1 - 1e-3 ROUNDED TO float32, and its backward passes the gradient on
that closed interval.  The fp64 evaluation therefore clamps at those two float32 numbers (as fp64 values), not at the fp64 numbers
1e-3 and 0.999: a weight_sum that sits exactly on a bound in fp32 sits on it in fp64 as well."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
IGR_W = 0.1
UP = 1.25   # upstream gradient of the loss
LO, HI = float(np.float32(1e-3)), float(np.float32(1.0 - 1e-3))
KEYS = ("loss", "color_fine_loss", "eikonal_loss", "mask_loss", "psnr", "cdf", "weight_max", "mask_sum")


def restated(inp, mask_weight, dtype):
    """render_volume.py:458-496, 507-510 with the reference's names, on the CPU in `dtype` -> (scalars, gradients)."""
    color_fine, weight_sum, gradient_error = (inp[k].detach().to(dtype).requires_grad_(True) for k in ("color_fine", "weight_sum", "gradient_error"))
    true_rgb, mask, cdf_fine, weight_max = (inp[k].to(dtype) for k in ("true_rgb", "mask", "cdf_fine", "weight_max"))
    if mask_weight > 0.0:                                                                       # :458-461
        mask = (mask > 0.5).to(dtype)
    else:
        mask = torch.ones_like(mask)
    mask_sum = mask.sum() + 1e-5                                                                # :463
    color_error = (color_fine - true_rgb) * mask                                                # :481
    color_fine_loss = F.l1_loss(color_error, torch.zeros_like(color_error), reduction="sum") / mask_sum   # :484
    psnr = 20.0 * torch.log10(1.0 / (((color_fine - true_rgb) ** 2 * mask).sum() / (mask_sum * 3.0)).sqrt())   # :490
    eikonal_loss = gradient_error                                                               # :492
    mask_loss = F.binary_cross_entropy(weight_sum.clip(LO, HI), mask)                           # :494
    loss = color_fine_loss + eikonal_loss * IGR_W + mask_loss * mask_weight                     # :496
    (loss * UP).backward()
    scalars = {"loss": loss, "color_fine_loss": color_fine_loss, "eikonal_loss": eikonal_loss, "mask_loss": mask_loss, "psnr": psnr,
               "cdf": (cdf_fine[:, :1] * mask).sum() / mask_sum, "weight_max": (weight_max * mask).sum() / mask_sum, "mask_sum": mask_sum}
    grads = {"color_fine": color_fine.grad, "weight_sum": weight_sum.grad, "gradient_error": gradient_error.grad}
    return {k: v.detach() for k, v in scalars.items()}, grads


def native(inp, mask_weight):
    from iron_amd.image_losses import volume_losses
    data = torch.zeros(inp["color_fine"].shape[0], 10)
    data[:, 6:9], data[:, 9:10] = inp["true_rgb"], inp["mask"]
    data = data.to(DEV)                                                    # true_rgb and mask are slices of the batch, as in a step
    leaves = {k: inp[k].detach().clone().to(DEV).requires_grad_(True) for k in ("color_fine", "weight_sum", "gradient_error")}
    out = volume_losses(leaves["color_fine"], data[:, 6:9], data[:, 9:10], leaves["weight_sum"], inp["weight_max"].to(DEV),
                        inp["cdf_fine"].to(DEV), leaves["gradient_error"], IGR_W, mask_weight)
    assert set(out) == set(KEYS) and all(v.dim() == 0 and v.is_cuda for v in out.values())
    assert out["loss"].requires_grad and not any(out[k].requires_grad for k in KEYS[1:])
    (out["loss"] * UP).backward()
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, {k: v.grad.cpu() for k, v in leaves.items()}


def make_case(b, kind="random", seed=0):
    gen = torch.Generator().manual_seed(500 + seed)
    inp = {"color_fine": torch.rand(b, 3, generator=gen), "true_rgb": torch.rand(b, 3, generator=gen), "mask": torch.rand(b, 1, generator=gen),
           "weight_sum": torch.rand(b, 1, generator=gen) * 0.98 + 0.01, "weight_max": torch.rand(b, 1, generator=gen),
           "cdf_fine": torch.rand(b, 8, generator=gen), "gradient_error": torch.rand((), generator=gen) * 0.3}
    if b >= 8:   # the corners ride along in every batch that has room for them
        inp["weight_sum"][0], inp["weight_sum"][1] = LO, HI                    # exactly on the bounds: the gradient passes
        inp["weight_sum"][2], inp["weight_sum"][3] = 5e-4, 0.9995              # outside both: no gradient
        inp["weight_sum"][4], inp["weight_sum"][5] = 0.0, 1.0
        inp["mask"][0], inp["mask"][2], inp["mask"][4] = 0.9, 0.9, 0.1
        inp["mask"][6] = 0.5                                                   # exactly 0.5 is outside the mask
        inp["color_fine"][7, 1] = inp["true_rgb"][7, 1]                        # c == t in one channel: sign(0) = 0
        inp["mask"][7] = 0.8
    if kind == "zero_mask":
        inp["mask"] = inp["mask"] * 0.5
    elif kind == "one_ray":
        inp["mask"] = inp["mask"] * 0.5
        inp["mask"][b // 2] = 0.75
    elif kind == "equal":
        inp["color_fine"] = inp["true_rgb"].clone()
    return inp


CASES = [("B%d_w%g" % (b, w), dict(b=b), w) for b in (1, 63, 64, 65, 2049) for w in (0.0, 0.1)]
CASES += [("zero_mask", dict(b=65, kind="zero_mask"), 0.1), ("one_ray_mask", dict(b=65, kind="one_ray"), 0.1),
          ("prediction_equals_target", dict(b=65, kind="equal"), 0.1), ("prediction_equals_target_w0", dict(b=63, kind="equal"), 0.0)]


@pytest.mark.parametrize("name, kw, mask_weight", CASES, ids=[c[0] for c in CASES])
def test_against_the_restated_expressions_in_fp64(name, kw, mask_weight):
    inp = make_case(seed=[c[0] for c in CASES].index(name), **kw)
    s64, g64 = restated(inp, mask_weight, torch.float64)
    s32, g32 = restated(inp, mask_weight, torch.float32)
    got, grads = native(inp, mask_weight)
    for k in KEYS:
        w64, w32, g = float(s64[k]), float(s32[k]), float(got[k])
        if not np.isfinite(w64):
            print("%-28s %-16s %s (fp64 %s)" % (name, k, g, w64))
            assert g == w64, (k, g, w64)                                   # psnr = +inf when prediction equals target
            continue
        floor = abs(w32 - w64)
        tol = max(4.0 * floor, 1e-6 * abs(w64))
        err = abs(g - w64)
        print("%-28s %-16s %.9g  err %.2e  fp32 floor %.2e  tol %.2e" % (name, k, g, err, floor, tol))
        assert err <= tol, (k, g, w64)
    for k in ("color_fine", "weight_sum", "gradient_error"):
        w64, w32, g = g64[k], g32[k], grads[k]
        assert g.shape == w64.shape and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), k
        floor = float((w32.double() - w64).abs().max())
        tol = max(4.0 * floor, 1e-6 * float(w64.abs().max()))
        err = float((g.double() - w64).abs().max())
        print("%-28s d %-14s max|.| %.3e  err %.2e  fp32 floor %.2e  tol %.2e" % (name, k, float(w64.abs().max()), err, floor, tol))
        assert err <= tol, k
        assert int(torch.count_nonzero(g[w64 == 0])) == 0, k + ": not exactly 0 where autograd gives 0"
    # the edge cases by name
    b = kw["b"]
    if mask_weight == 0.0:
        assert int(torch.count_nonzero(grads["weight_sum"])) == 0 and float(got["mask_sum"]) == pytest.approx(b + 1e-5, rel=1e-6)
    if kw.get("kind") == "zero_mask":
        assert float(got["color_fine_loss"]) == 0.0 and float(got["psnr"]) == float("inf") and int(torch.count_nonzero(grads["color_fine"])) == 0
        assert float(got["mask_sum"]) == pytest.approx(1e-5, rel=1e-6)
    if kw.get("kind") == "one_ray":
        nz = torch.nonzero(grads["color_fine"].abs().sum(dim=-1)).reshape(-1).tolist()
        assert nz == [b // 2] and float(got["mask_sum"]) == pytest.approx(1.00001, rel=1e-6)
    if kw.get("kind") == "equal":
        assert float(got["psnr"]) == float("inf") and float(got["color_fine_loss"]) == 0.0 and int(torch.count_nonzero(grads["color_fine"])) == 0
    if b >= 8 and mask_weight > 0.0 and kw.get("kind") is None:
        gw = grads["weight_sum"].reshape(-1)
        assert float(gw[0]) != 0.0 and float(gw[1]) != 0.0 and all(float(gw[i]) == 0.0 for i in (2, 3, 4, 5))
        assert all(float(v) == 0.0 for v in grads["color_fine"][6]), "a raw mask of exactly 0.5 is outside"
        assert float(grads["color_fine"][7, 1]) == 0.0 and float(grads["color_fine"][7, 0]) != 0.0
    assert float(grads["gradient_error"]) == pytest.approx(IGR_W * UP, rel=1e-6)


def test_forward_and_backward_are_bitwise_reproducible():
    inp = make_case(b=2049, seed=77)
    a, b = native(inp, 0.1), native(inp, 0.1)
    for k in KEYS:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_layouts_and_bad_inputs():
    from iron_amd import _lib
    from iron_amd.image_losses import volume_losses
    inp = {k: v.to(DEV) for k, v in make_case(b=65, seed=3).items()}
    args = [inp[k] for k in ("color_fine", "true_rgb", "mask", "weight_sum", "weight_max", "cdf_fine", "gradient_error")]
    want = volume_losses(*args, IGR_W, 0.1)
    flat = list(args)
    flat[2], flat[3], flat[4] = args[2].reshape(-1), args[3].reshape(-1), args[4].reshape(-1)      # [B] in place of [B, 1]
    got = volume_losses(*flat, IGR_W, 0.1)
    assert all(torch.equal(want[k], got[k]) for k in KEYS)
    none = volume_losses(args[0], args[1], None, *args[3:], IGR_W, 0.0)                             # no mask at mask_weight = 0
    ones = volume_losses(*args, IGR_W, 0.0)
    assert all(torch.equal(none[k], ones[k]) for k in KEYS)
    with pytest.raises(_lib.IronError):
        volume_losses(args[0], args[1], None, *args[3:], IGR_W, 0.1)
    with pytest.raises(_lib.IronError):
        volume_losses(args[0].cpu(), *args[1:], IGR_W, 0.1)
    with pytest.raises(_lib.IronError):
        volume_losses(args[0], args[1][:-1], *args[2:], IGR_W, 0.1)
    with pytest.raises(_lib.IronError):
        volume_losses(args[0], args[1], args[2], args[3][:-1], *args[4:], IGR_W, 0.1)
    with pytest.raises(_lib.IronError):
        volume_losses(args[0][:0], args[1][:0], args[2][:0], args[3][:0], args[4][:0], args[5][:0], args[6], IGR_W, 0.1)
