"""The stage-2 image losses on the GPU (csrc/losses.hip behind iron_amd.image_losses): parity with the reference's fp64 run
(golden G20), the masked SSIM against the torch restatement on the same GPU tensors, input layouts, determinism, the errors,
and one S1 training step with both losses."""
import json
import warnings

import numpy as np
import pytest
import torch

import _loss_oracle as O
from _util import golden, t

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g20():
    return golden("g20_image_losses.npz")


def _inputs(g, case):
    meta = json.loads(str(g["meta_json"]))["cases"][case]
    xu, yu = O.g20_images(meta["image"])
    x = (torch.from_numpy(xu).float() / 255.0).to(DEV)
    y = (torch.from_numpy(yu).float() / 255.0).to(DEV)
    m = None if meta["mask"] is None else torch.from_numpy(O.g20_mask(meta["mask"])).bool().to(DEV)
    return meta, x, y, m


def _native(kind, x, y, m=None, scale=1.0, **kw):
    from iron_amd.image_losses import PyramidL2Loss, ssim_loss_fn
    x = x.detach().clone().requires_grad_(True)
    y = y.detach().clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = PyramidL2Loss()(x, y) if kind == "pyr" else ssim_loss_fn(x, y, m, **kw)
    (scale * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad, y.grad


def _oracle(kind, x, y, m=None, scale=1.0, **kw):
    x = x.detach().clone().requires_grad_(True)
    y = y.detach().clone().requires_grad_(True)
    loss = O.pyramid_l2(x, y) if kind == "pyr" else O.ssim(x, y, m, **kw)
    (scale * loss).backward()
    return loss.detach(), x.grad, y.grad


def test_parity_with_the_reference_fp64_on_every_g20_case(g20):
    cases = json.loads(str(g20["meta_json"]))["cases"]
    n = 0
    for case in cases:
        meta, x, y, m = _inputs(g20, case)
        idx = torch.from_numpy(g20["case__%s__idx" % case]).to(DEV)
        for kind in meta["losses"]:
            p = "case__%s__%s__" % (case, kind)
            loss, dx, dy = _native(kind, x, y, m)
            ref64, ref32 = float(g20[p + "loss64"]), float(g20[p + "loss32"])
            err = abs(float(loss) - ref64)
            tol = max(1e-6 * abs(ref64), 1.5 * abs(ref32 - ref64))
            print("%-20s %-4s loss err %.2e (tol %.2e)" % (case, kind, err, tol), end="")
            assert err <= tol, (case, kind, float(loss), ref64)
            for name, got in (("dx", dx), ("dy", dy)):
                want = g20[p + name + "64"]
                e = float(np.abs(got.reshape(-1)[idx].double().cpu().numpy() - want).max())
                gtol = max(1e-5 * float(g20[p + name + "max64"]), 1.5 * float(g20[p + name + "gap"]))
                print("  %s %.2e (tol %.2e)" % (name, e, gtol), end="")
                assert e <= gtol, (case, kind, name, e, gtol)
            print()
            n += 1
    assert n == 15


def _masks(b, h, w):
    gen = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(h) / h, torch.arange(w) / w, indexing="ij")
    holes = (((yy - 0.5) / 0.35) ** 2 + ((xx - 0.5) / 0.4) ** 2 < 1) & (torch.rand(h, w, generator=gen) > 0.01)
    holes[h // 3:h // 3 + 6, w // 4:w // 4 + 9] = False
    border = ((yy - 0.8) ** 2 + (xx - 0.1) ** 2) < 0.4
    out = {"holes": holes, "border": border, "all": torch.ones(h, w, dtype=torch.bool), "empty": torch.zeros(h, w, dtype=torch.bool)}
    return {k: v[None, None].expand(b, 1, h, w).contiguous() for k, v in out.items()}


@pytest.mark.parametrize("shape", [(1, 3, 96, 96), (2, 3, 77, 130)])
def test_masked_ssim_vs_oracle(shape):
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(shape, generator=gen).to(DEV)
    y = (x.cpu() + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1).to(DEV)
    for name, m in _masks(shape[0], shape[2], shape[3]).items():
        for mm in (m.to(DEV), m.to(DEV, torch.uint8), m.to(DEV, torch.float32)):
            loss, dx, dy = _native("ssim", x, y, mm)
            rl, rx, ry = _oracle("ssim", x.double(), y.double(), mm)
            if name == "empty":
                assert torch.isnan(loss) and torch.isnan(rl)
                assert not bool(dx.any()) and not bool(dy.any())  # nothing selected: no gradient, as torch's indexing backward
                continue
            assert abs(float(loss) - float(rl)) <= 1e-6 * abs(float(rl)) + 1e-7, (name, float(loss), float(rl))
            for got, want in ((dx, rx), (dy, ry)):
                assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max()), name
    # a pixel gets gradient only from kept pixels of the valid map whose window covers it (the border band has none)
    m = _masks(*shape[:1], *shape[2:])["border"].to(DEV)
    _, dx, _ = _native("ssim", x, y, m)
    keep = O.erosion(m.float(), torch.ones(11, 11, device=DEV)) > 0.5
    interior = torch.zeros_like(keep)
    interior[:, :, 5:-5, 5:-5] = True
    reach = torch.nn.functional.max_pool2d((keep & interior).float(), 11, stride=1, padding=5) > 0.5
    assert bool((keep & ~interior).any())
    assert not bool(dx[(~reach).expand_as(dx)].any())


def test_layouts_requires_grad_upstream_scale_and_batch():
    from iron_amd.image_losses import PyramidL2Loss, ssim_loss_fn
    gen = torch.Generator().manual_seed(7)
    hwc = torch.rand(64, 80, 3, generator=gen).to(DEV)
    gt = torch.rand(64, 80, 3, generator=gen).to(DEV)
    mask = (torch.rand(64, 80, generator=gen) > 0.05).to(DEV)
    # the drivers' layout: results["color"].permute(2, 0, 1)[None], strided
    a = hwc.clone().requires_grad_(True)
    pred = a.permute(2, 0, 1)[None]
    assert not pred.is_contiguous()
    gt_img = gt.permute(2, 0, 1)[None]
    lam = 0.37
    loss = PyramidL2Loss()(pred, gt_img) + lam * ssim_loss_fn(pred, gt_img, mask[None, None])
    loss.backward()
    b = hwc.clone().double().requires_grad_(True)
    ref = O.pyramid_l2(b.permute(2, 0, 1)[None], gt_img.double()) + lam * O.ssim(b.permute(2, 0, 1)[None], gt_img.double(), mask[None, None])
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
    assert a.grad.shape == hwc.shape
    assert float((a.grad.double() - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max())
    # Y with requires_grad, an upstream scale other than 1, batch 2
    x = torch.rand(2, 3, 48, 40, generator=gen).to(DEV)
    y = torch.rand(2, 3, 48, 40, generator=gen).to(DEV)
    for kind in ("pyr", "ssim"):
        loss, dx, dy = _native(kind, x, y, scale=-2.5)
        rl, rx, ry = _oracle(kind, x.double(), y.double(), scale=-2.5)
        assert abs(float(loss) - float(rl)) <= 1e-6 * abs(float(rl))
        for got, want in ((dx, rx), (dy, ry)):
            assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max()), kind
        if kind == "pyr":
            assert torch.equal(dy, -dx)
    # only X requires grad
    xx = x.clone().requires_grad_(True)
    PyramidL2Loss()(xx, y).backward()
    assert xx.grad is not None


def test_two_runs_are_bit_equal(g20):
    _, x, y, _ = _inputs(g20, "s512")
    m = torch.from_numpy(O.g20_mask("holes512")).bool().to(DEV)
    for kind, mm in (("pyr", None), ("ssim", None), ("ssim", m)):
        a = _native(kind, x, y, mm)
        b = _native(kind, x, y, mm)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), kind


def test_errors():
    from iron_amd._lib import IronError
    from iron_amd.image_losses import PyramidL2Loss, gaussian_filter, ssim_loss_fn, _fspecial_gauss_1d
    x = torch.rand(1, 3, 32, 32, device=DEV)
    for h, w in ((15, 32), (32, 15), (8, 8)):
        with pytest.raises(IronError):
            PyramidL2Loss()(torch.rand(1, 3, h, w, device=DEV), torch.rand(1, 3, h, w, device=DEV))
    with pytest.raises(IronError):
        PyramidL2Loss()(torch.rand(1, 2, 32, 32, device=DEV), torch.rand(1, 2, 32, 32, device=DEV))
    with pytest.raises(IronError):
        PyramidL2Loss()(x.cpu(), x.cpu())
    with pytest.raises(IronError):
        PyramidL2Loss()(x.double(), x.double())
    with pytest.raises(IronError):
        ssim_loss_fn(x.cpu(), x.cpu())
    with pytest.raises(IronError):
        ssim_loss_fn(x.double(), x.double())
    short = torch.rand(1, 3, 8, 64, device=DEV)
    with pytest.warns(UserWarning, match="Skipping Gaussian Smoothing"):
        with pytest.raises(IronError):
            ssim_loss_fn(short, short, torch.ones(1, 1, 8, 64, dtype=torch.bool, device=DEV))
    with pytest.warns(UserWarning, match="Skipping Gaussian Smoothing"):
        v = ssim_loss_fn(short, short)
    assert abs(float(v)) < 1e-6
    win = _fspecial_gauss_1d(11, 1.5).repeat(3, 1, 1, 1)
    with pytest.raises(IronError):
        gaussian_filter(torch.rand(1, 3, 4, 16, 16, device=DEV), win.unsqueeze(2))
    with pytest.raises(NotImplementedError):
        gaussian_filter(x.requires_grad_(True), win)


def test_gaussian_filter_vs_conv2d():
    from iron_amd.image_losses import _fspecial_gauss_1d, gaussian_filter
    gen = torch.Generator().manual_seed(9)
    for shape in ((2, 3, 40, 57), (1, 3, 8, 30)):
        x = torch.rand(shape, generator=gen).to(DEV)
        win = _fspecial_gauss_1d(11, 1.5).repeat(3, 1, 1, 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = gaussian_filter(x, win)
        want = O._blur(x.double(), win[:1].double().to(DEV))
        assert got.shape == want.shape
        assert float((got.double() - want).abs().max()) <= 1e-6


def test_s1_training_step_with_both_losses():
    """One 96x96 S1 step as render_surface.py trains: render_camera(handle_edges=True, is_training=True), loss = pyramid L2 +
    SSIM with the render mask; every parameter gradient equals the same step through the torch restatement on the same tensors."""
    from iron_amd import scenes
    from iron_amd.image_losses import PyramidL2Loss, ssim_loss_fn
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    g = golden("g15_train_edges_S1.npz")
    nets = {k: v.cuda() for k, v in scenes.build_networks("S1").items()}
    cam = Camera(int(g["W"]), int(g["H"]), t(g["K"]).cuda(), t(g["W2C"]).cuda())
    res = render_camera(cam, nets["sdf_network"], RayTracer(), nets, make_render_fn(GGXColocatedRenderer(use_cuda=True)),
                        fill_holes=False, handle_edges=True, is_training=True, depth_edge_mask=t(g["depth_edge_mask_input"]).cuda())
    pred = res["color"].permute(2, 0, 1)[None]
    gen = torch.Generator().manual_seed(13)
    gt = (pred.detach().cpu() * 0.8 + 0.1 * torch.rand(pred.shape, generator=gen)).to(DEV)
    mask = res["convergent_mask"][None, None]
    assert 100 < int(mask.sum()) < mask.numel()
    params = [p for k in sorted(nets) for p in nets[k].parameters() if p.requires_grad]
    native = PyramidL2Loss()(pred, gt) + 0.5 * ssim_loss_fn(pred, gt, mask)
    ref = O.pyramid_l2(pred.double(), gt.double()) + 0.5 * O.ssim(pred.double(), gt.double(), mask)
    assert abs(float(native.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    ga = torch.autograd.grad(native, params, retain_graph=True, allow_unused=True)
    gb = torch.autograd.grad(ref, params, allow_unused=True)
    n = 0
    for a, b in zip(ga, gb):
        assert (a is None) == (b is None)
        if a is None:
            continue
        den = float(b.double().norm())
        assert float((a.double() - b.double()).norm()) <= 1e-5 * max(den, 1e-30), (a.shape, den)
        n += 1
    assert n > 20
