"""surface_regularisers (iron_amd/image_losses.py over csrc/optim.hip: iron_surface_reg) against the torch expressions of
render_surface.py:580-613, 639 evaluated in fp64 under autograd.

Error bound (the rule of DESIGN §19 and §20): the floor is the same expressions in fp32 against fp64; the HIP result is allowed
4 x that floor, and never less than 1e-6 relative to the sum of the absolute terms of the quantity -- for the two losses, whose
terms are all non-negative, the fp64 loss itself; for a gradient tensor, whose elements are single products, its largest fp64
element.  Counts are exact; forward and backward are bitwise equal from run to run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EIK_W, RR_W = 0.1, 0.1
UP_EIK, UP_RR = 1.25, 0.75   # upstream gradients of the two losses


def restated(eik_grad, normal, mask, roughness, edge, dtype):
    """render_surface.py:580-613, 639 with the reference's names; `roughness` is results["specular_roughness"] ([H, W] from the
    ggx render_fn, [H, W, 1] from the comp one).  -> (eik_loss, roughrange_loss, (eik_cnt, n_mask, n_selected), gradients)."""
    leaves = [t.detach().to(dtype).requires_grad_(True) if t is not None else None for t in (eik_grad, normal, roughness, edge)]
    eik_grad, normal, roughness, edge = leaves
    roughrange_loss = torch.zeros((), dtype=dtype, device=mask.device)
    n_mask = n_sel = 0
    eik_cnt = eik_grad.shape[0]                                          # :582
    eik_loss = ((eik_grad.norm(dim=-1) - 1) ** 2).sum()                  # :583
    if mask.any():                                                       # :591
        g = normal[mask]                                                 # :601
        n_mask = g.shape[0]
        eik_cnt += g.shape[0]                                            # :602
        eik_loss = eik_loss + ((g.norm(dim=-1) - 1) ** 2).sum()          # :603
        if edge is not None:                                             # :604
            eik_cnt += edge.shape[0]                                     # :606
            eik_loss = eik_loss + ((edge.norm(dim=-1) - 1) ** 2).sum()   # :607
        r = roughness[mask]                                              # :609
        r = r[r > 0.5]                                                   # :610-611
        n_sel = r.numel()
        if r.numel() > 0:                                                # :612
            roughrange_loss = (r - 0.5).mean() * RR_W                    # :613
    eik_loss = eik_loss / eik_cnt * EIK_W                                # :639
    (UP_EIK * eik_loss + UP_RR * roughrange_loss).backward()
    grads = [None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad) for t in leaves]
    return eik_loss.detach(), roughrange_loss.detach(), (eik_cnt, n_mask, n_sel), grads


def native(eik_grad, normal, mask, roughness, edge):
    from iron_amd.image_losses import surface_regularisers
    leaves = [t.detach().clone().requires_grad_(True) if t is not None else None for t in (eik_grad, normal, roughness, edge)]
    eik, rr, counts = surface_regularisers(leaves[0], leaves[1], mask, leaves[2], leaves[3], EIK_W, RR_W, return_counts=True)
    (UP_EIK * eik + UP_RR * rr).backward()
    torch.cuda.synchronize()
    grads = [None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad) for t in leaves]
    return eik.detach(), rr.detach(), tuple(int(c) for c in counts.cpu()), grads


def make_case(m, h, w, e, layout, mask_kind="random", rough_kind="random", zero_normal=False, seed=0):
    gen = torch.Generator().manual_seed(100 + seed)
    eik = torch.nn.functional.normalize(torch.randn(m, 3, generator=gen), dim=-1) * (1.0 + 0.3 * torch.randn(m, 1, generator=gen))
    normal = torch.randn(h, w, 3, generator=gen) * 0.7
    if mask_kind == "random":
        mask = torch.rand(h, w, generator=gen) < 0.6
    elif mask_kind == "none":
        mask = torch.zeros(h, w, dtype=torch.bool)
    else:  # one pixel
        mask = torch.zeros(h, w, dtype=torch.bool)
        mask[h // 2, w // 3] = True
    rough = torch.rand(h, w, generator=gen)
    if rough_kind == "low":          # nothing above 0.5
        rough = rough * 0.5
    elif rough_kind == "half":       # exactly 0.5 inside the mask, which is not selected, beside ordinary values
        rough[::2, ::3] = 0.5
    elif rough_kind == "only_half":  # the only candidates are exactly 0.5
        rough = torch.where(rough > 0.5, torch.full_like(rough, 0.5), rough)
    if mask_kind == "one" and rough_kind == "random":
        rough[h // 2, w // 3] = 0.8
    if zero_normal:
        ys, xs = torch.nonzero(mask, as_tuple=True)
        normal[ys[0], xs[0]] = 0.0
    if layout == "comp":
        rough = rough.unsqueeze(-1)
    edge = torch.randn(e, 3, generator=gen) if e > 0 else None
    return [t.to(DEV) if t is not None else None for t in (eik, normal, mask, rough, edge)]


CASES = {
    "M1_ggx": dict(m=1, h=5, w=7, e=0, layout="ggx"),
    "M65_comp_edges_zero_normal_half": dict(m=65, h=9, w=11, e=3, layout="comp", rough_kind="half", zero_normal=True),
    "M4097_ggx_edges": dict(m=4097, h=33, w=31, e=3, layout="ggx"),
    "M4097_comp": dict(m=4097, h=64, w=48, e=0, layout="comp", zero_normal=True),
    "all_false_mask": dict(m=65, h=9, w=11, e=3, layout="ggx", mask_kind="none"),
    "one_pixel_mask": dict(m=65, h=9, w=11, e=0, layout="ggx", mask_kind="one"),
    "roughness_all_low": dict(m=65, h=9, w=11, e=3, layout="comp", rough_kind="low"),
    "roughness_only_half": dict(m=1, h=9, w=11, e=0, layout="ggx", rough_kind="only_half"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restated_expressions_in_fp64(name):
    case = make_case(seed=list(CASES).index(name), **CASES[name])
    eik_grad, normal, mask, rough, edge = case
    e64, r64, c64, g64 = restated(eik_grad, normal, mask, rough, edge, torch.float64)
    e32, r32, _, g32 = restated(eik_grad, normal, mask, rough, edge, torch.float32)
    eik, rr, counts, grads = native(*case)
    assert counts == c64, (counts, c64)
    for label, got, w64, w32 in (("eik_loss", eik, e64, e32), ("roughrange_loss", rr, r64, r32)):
        floor = abs(float(w32) - float(w64))
        tol = max(4.0 * floor, 1e-6 * abs(float(w64)))
        err = abs(float(got) - float(w64))
        print("%-34s %-16s %.9g  err %.2e  fp32 floor %.2e  tol %.2e" % (name, label, float(got), err, floor, tol))
        assert err <= tol, (label, float(got), float(w64))
    for label, got, w64, w32 in zip(("d eik_grad", "d normal", "d roughness", "d edge"), grads, g64, g32):
        if got is None:
            assert w64 is None
            continue
        assert got.shape == w64.shape and bool(torch.isfinite(got).all()), label
        floor = float((w32.double() - w64).abs().max())
        tol = max(4.0 * floor, 1e-6 * float(w64.abs().max()))
        err = float((got.double() - w64).abs().max())
        print("%-34s %-16s max|.| %.3e  err %.2e  fp32 floor %.2e  tol %.2e" % (name, label, float(w64.abs().max()), err, floor, tol))
        assert err <= tol, label
        assert int(torch.count_nonzero(got[w64 == 0])) == 0, label + ": not exactly 0 where autograd gives 0"   # unmasked, zero vectors, r <= 0.5
    # the edge cases by name
    kw = CASES[name]
    if kw.get("mask_kind") == "none":
        assert counts == (kw["m"], 0, 0) and float(rr) == 0.0 and bool(torch.isfinite(eik))
        assert all(int(torch.count_nonzero(g)) == 0 for g in grads[1:] if g is not None)
    if kw.get("rough_kind") in ("low", "only_half"):
        assert counts[2] == 0 and float(rr) == 0.0 and int(torch.count_nonzero(grads[2])) == 0
    if kw.get("rough_kind") == "half":
        assert bool(((rough.reshape(mask.shape) == 0.5) & mask).any()) and int(torch.count_nonzero(grads[2][rough == 0.5])) == 0
    if kw.get("zero_normal"):
        zero = (normal == 0).all(dim=-1) & mask
        assert bool(zero.any()) and int(torch.count_nonzero(grads[1][zero])) == 0


def test_forward_and_backward_are_bitwise_reproducible():
    case = make_case(seed=42, **CASES["M4097_ggx_edges"])
    a, b = native(*case), native(*case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)


def test_bad_inputs_are_refused():
    from iron_amd import _lib
    from iron_amd.image_losses import surface_regularisers
    eik_grad, normal, mask, rough, edge = make_case(seed=1, **CASES["M1_ggx"])
    with pytest.raises(_lib.IronError):
        surface_regularisers(eik_grad.cpu(), normal, mask, rough)
    with pytest.raises(_lib.IronError):
        surface_regularisers(eik_grad, normal, mask[:-1], rough)
    with pytest.raises(_lib.IronError):
        surface_regularisers(eik_grad, normal, mask.float(), rough)
    with pytest.raises(_lib.IronError):
        surface_regularisers(eik_grad, normal, mask, rough[..., :-1])
    lib = _lib.load_train()
    a = _lib.iron_surface_reg_args()
    a.m = -1
    assert lib.iron_surface_reg(a, None, None, None, None, None, 0, None) == _lib.IRON_ERR_BAD_ARG
    assert lib.iron_surface_reg_backward(a, None, None, None, None, None, None, None, None) == _lib.IRON_ERR_BAD_ARG
