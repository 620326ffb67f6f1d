"""SurfaceTrainer (iron_amd/train_surface.py) and load_datadir (iron_amd/dataset.py) on a dataset the test writes itself: four
48 x 48 views of scenes.build_networks("S1", seed=5) at four yaws of the fixture camera, as PNG plus cam_dict_norm.json."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZE = 48
# the JSON lists the names in this order; the loader sorts them by their integer (2 before 10, unlike the string order)
NAMES = ["10.png", "0.png", "2.png", "1.png"]
YAWS = {"0.png": 0.0, "1.png": 90.0, "2.png": 180.0, "10.png": 270.0}
ORDERED = ["0.png", "1.png", "2.png", "10.png"]


def _target_networks():
    from iron_amd import scenes
    return {k: m.to(DEV) for k, m in scenes.build_networks("S1", seed=5).items()}


def _start_networks():
    """Re-seeded material networks (seed 0) on the target's SDF."""
    from iron_amd import scenes
    nets = {k: m.to(DEV) for k, m in scenes.build_networks("S1", seed=0).items()}
    nets["sdf_network"] = _target_networks()["sdf_network"]
    return nets


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from iron_amd import scenes
    from iron_amd.dataset import to8b
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    root = tmp_path_factory.mktemp("s1_views")
    os.makedirs(root / "image")
    nets = _target_networks()
    fn = make_render_fn(GGXColocatedRenderer(use_cuda=True))
    cam_dict, pixels, mats = {}, {}, {}
    for name in NAMES:
        K, W2C = scenes.fixture_camera_matrices(SIZE, SIZE, yaw_deg=YAWS[name])
        with torch.no_grad():
            res = render_camera(Camera(SIZE, SIZE, K.to(DEV), W2C.to(DEV)), nets["sdf_network"], RayTracer(), nets, fn, fill_holes=True,
                                handle_edges=True, is_training=False)
        img8 = to8b(res["color"].cpu().numpy())
        Image.fromarray(img8).save(str(root / "image" / name))
        cam_dict[name] = {"K": [float(x) for x in K.reshape(-1)], "W2C": [float(x) for x in W2C.reshape(-1)], "img_size": [SIZE, SIZE]}
        pixels[name], mats[name] = img8, (K, W2C)
    with open(root / "cam_dict_norm.json", "w") as fp:
        json.dump(cam_dict, fp)
    assert all(p.max() > 0 for p in pixels.values())
    return {"dir": str(root), "pixels": pixels, "mats": mats}


def _trainer(dataset, out_dir=None, networks=None, **kw):
    from iron_amd.train_surface import SurfaceTrainer
    kw.setdefault("patch_size", 32)
    kw.setdefault("renderer_name", "ggx")
    return SurfaceTrainer(data_dir=dataset["dir"], out_dir=out_dir, networks=_start_networks() if networks is None else networks, **kw)


def _named_params(tr):
    out = {"sdf_network." + n: p for n, p in tr.sdf_network.named_parameters()}
    for k, net in tr.color_network_dict.items():
        out.update({k + "." + n: p for n, p in net.named_parameters()})
    return out


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
def test_load_datadir_returns_the_written_pixels_and_matrices_in_the_reference_order(dataset):
    from iron_amd.dataset import load_datadir
    fpaths, images, Ks, W2Cs = load_datadir(dataset["dir"])
    assert [os.path.basename(p) for p in fpaths] == ORDERED
    assert images.dtype == torch.float32 and tuple(images.shape) == (4, SIZE, SIZE, 3)
    assert Ks.dtype == torch.float32 and tuple(Ks.shape) == (4, 4, 4) and tuple(W2Cs.shape) == (4, 4, 4)
    for i, name in enumerate(ORDERED):
        assert torch.equal(images[i], torch.from_numpy(dataset["pixels"][name].astype(np.float32) / 255.0))
        assert torch.equal(Ks[i], dataset["mats"][name][0]) and torch.equal(W2Cs[i], dataset["mats"][name][1])


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
def restated_losses(tr, results, gt_patch, eik_grad, reg_dtype):
    """render_surface.py:571-647 with the reference's names: PyramidL2Loss and ssim_loss_fn as the reference calls them, torch
    expressions for the rest; the regularisers in `reg_dtype`."""
    from iron_amd.image_losses import ssim_loss_fn
    mask = results["convergent_mask"] | results["edge_mask"]                                     # :567-569
    zero = torch.zeros((), device=DEV)
    img_l2_loss, img_ssim_loss, roughrange_loss = zero, zero, zero.to(reg_dtype)                  # :571-574
    eik_grad = eik_grad.to(reg_dtype)
    eik_cnt = eik_grad.shape[0]                                                                  # :582
    eik_loss = ((eik_grad.norm(dim=-1) - 1) ** 2).sum()                                          # :583
    if mask.any():                                                                               # :591
        pred_img = results["color"].permute(2, 0, 1).unsqueeze(0)                                # :592
        gt_img = gt_patch.permute(2, 0, 1).unsqueeze(0).to(pred_img.device, dtype=pred_img.dtype)
        pred_img, gt_img = pred_img[:, :3, :, :], gt_img[:, :3, :, :]                            # :595-596
        img_l2_loss = tr.pyramidl2_loss_fn(pred_img, gt_img)                                     # :597
        img_ssim_loss = tr.ssim_weight * ssim_loss_fn(pred_img, gt_img, mask.unsqueeze(0).unsqueeze(0))   # :598
        g = results["normal"].to(reg_dtype)[mask]                                                # :601
        eik_cnt += g.shape[0]
        eik_loss = eik_loss + ((g.norm(dim=-1) - 1) ** 2).sum()                                  # :603
        if "edge_pos_neg_normal" in results:                                                     # :604
            g = results["edge_pos_neg_normal"].to(reg_dtype)
            eik_cnt += g.shape[0]
            eik_loss = eik_loss + ((g.norm(dim=-1) - 1) ** 2).sum()                              # :607
        roughness = results["specular_roughness"].to(reg_dtype)[mask]                            # :609
        roughness = roughness[roughness > 0.5]                                                   # :611
        if roughness.numel() > 0:
            roughrange_loss = (roughness - 0.5).mean() * tr.roughrange_weight                    # :613
    eik_loss = eik_loss / eik_cnt * tr.eik_weight                                                # :639
    loss = (img_l2_loss + img_ssim_loss).to(reg_dtype) + eik_loss + roughrange_loss              # :647
    return {"loss": loss, "img_l2_loss": img_l2_loss, "img_ssim_loss": img_ssim_loss, "eik_loss": eik_loss, "roughrange_loss": roughrange_loss}


def _rel_l2(a, b):
    nb = float(b.double().norm())
    return float((a.double() - b.double()).norm()) / nb if nb > 0 else float(a.double().norm())


def test_losses_and_parameter_gradients_match_the_restated_loop_on_a_fixed_render(dataset):
    tr = _trainer(dataset)
    idx, origin = 0, (8, 8)
    eik_points = tr.draw()[2]
    params = _named_params(tr)

    def run(kind):
        tr.optimizer.zero_grad(set_to_none=True)
        results = tr.render_patch(idx, origin)   # an identical render for every run: nothing steps in between
        eik_grad = tr.sdf_network.gradient(eik_points).view(-1, 3)
        gt = tr.gt_patch(idx, origin)
        out = tr.compute_losses(results, gt, eik_grad) if kind == "ours" else restated_losses(tr, results, gt, eik_grad, kind)
        out["loss"].backward()
        torch.cuda.synchronize()
        return ({k: float(v.detach()) for k, v in out.items() if k != "n_mask"}, int(out["n_mask"]) if "n_mask" in out else None,
                {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None})

    ours, n_mask, g_ours = run("ours")
    base, _, g_base = run(torch.float32)
    _, _, g_again = run(torch.float32)
    f64, _, g_64 = run(torch.float64)
    assert n_mask is not None and n_mask > 0
    for k in ("img_l2_loss", "img_ssim_loss", "eik_loss", "roughrange_loss", "loss"):
        floor = abs(base[k] - f64[k])
        tol = max(4.0 * floor, 1e-6 * abs(f64[k]))
        print("%-16s ours %.9g  restated fp32 %.9g  fp64-regularisers %.9g  tol %.2e" % (k, ours[k], base[k], f64[k], tol))
        assert abs(ours[k] - f64[k]) <= tol, k
    assert set(g_ours) == set(g_base) == set(g_64) and len(g_ours) > 60
    worst = (0.0, 0.0, 0.0)
    for n in sorted(g_base):
        floor, spread, err = _rel_l2(g_base[n], g_64[n]), _rel_l2(g_again[n], g_base[n]), _rel_l2(g_ours[n], g_base[n])
        allow = max(4.0 * floor, 1e-6) + spread
        worst = max(worst, (err, floor, spread))
        assert err <= allow, "%s: rel-L2 %.3e beyond 4 x %.3e (floor 1e-6) + run-to-run %.3e" % (n, err, floor, spread)
    print("parameter gradients, rel-L2 per tensor: largest error %.3e (its fp64-regulariser floor %.3e, its run-to-run spread %.3e)" % worst)
    print("largest floor %.3e, largest spread %.3e" % (max(_rel_l2(g_base[n], g_64[n]) for n in g_base),
                                                     max(_rel_l2(g_again[n], g_base[n]) for n in g_base)))


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
def test_same_seed_draws_the_same_and_fused_and_torch_optimisers_agree_after_one_step(dataset):
    """Both trainers see the same views, origins and eikonal points.  Their gradients differ by the backward library's float
    atomics, so each optimiser is held to the Adam allowance (tests/test_gpu_fused_adam.py: 2 x the fp32 floor of torch.optim.Adam
    against fp64, plus one ulp) against the fp64 CPU step fed ITS OWN gradient; across the two, an element may differ by the two
    updates' full lengths, 2 lr of its group (a first Adam step moves an element by lr g / (|g| + eps), and the sign of a
    gradient near zero is at the atomics' mercy)."""
    a, b = _trainer(dataset, seed=7), _trainer(dataset, seed=7)
    for _ in range(2):
        da, db = a.draw(), b.draw()
        assert da[0] == db[0] and da[1] == db[1] and torch.equal(da[2], db[2])
    assert _trainer(dataset, seed=8).draw()[2].ne(_trainer(dataset, seed=7).draw()[2]).any()

    fused, plain = _trainer(dataset, seed=3, optimizer="fused"), _trainer(dataset, seed=3, optimizer="torch")
    p0 = {n: p.detach().clone() for n, p in _named_params(fused).items()}
    of, ot = fused.step(), plain.step()
    assert of["view"] == ot["view"] and of["origin"] == ot["origin"]
    assert torch.equal(fused.device_rng.get_state(), plain.device_rng.get_state())
    assert fused.rng.bit_generator.state == plain.rng.bit_generator.state
    lf, lt = float(of["loss"]), float(ot["loss"])
    print("first-step loss: fused %.9g, torch %.9g" % (lf, lt))
    assert np.isfinite(lf) and abs(lf - lt) <= 1e-6 * abs(lt)   # the same forward code on the same parameters
    lr_of = {}
    for tr in (fused, plain):
        for g in tr.optimizer.param_groups:
            for p in g["params"]:
                lr_of[p] = g["lr"]
    pf, pt = _named_params(fused), _named_params(plain)
    worst = 0.0
    for n in sorted(p0):
        for tr_p in (pf[n], pt[n]):
            assert tr_p.grad is not None, n
            ref, low = [torch.nn.Parameter(p0[n].cpu().to(dt)) for dt in (torch.float64, torch.float32)]
            for q in (ref, low):
                q.grad = tr_p.grad.detach().cpu().to(q.dtype)
                torch.optim.Adam([q], lr=lr_of[tr_p]).step()
            floor = float((low.detach().double() - ref.detach()).abs().max())
            ulp = torch.from_numpy(np.asarray(np.spacing(np.abs(ref.detach().float().numpy())), dtype=np.float64))
            err = (tr_p.detach().double().cpu() - ref.detach()).abs()
            if tr_p is pf[n]:
                assert bool((err <= 2.0 * floor + ulp).all()), "%s: FusedAdam beyond the Adam allowance (floor %.3e, error %.3e)" % (
                    n, floor, float(err.max()))
                worst = max(worst, float((err / ulp).max()))
        gap = float((pf[n].detach() - pt[n].detach()).abs().max())
        assert gap <= 2.0 * lr_of[pf[n]] * (1.0 + 1e-6) + float(np.spacing(np.float32(p0[n].abs().max().item()))), (n, gap)
    print("FusedAdam after one trainer step: largest error %.2f ulp of the element's own magnitude (elements that end next to zero)" % worst)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
def test_thirty_steps_reduce_the_loss(dataset):
    tr = _trainer(dataset, seed=0)
    losses = []
    for _ in range(30):
        out = tr.step()
        losses.append({k: float(out[k]) for k in ("loss", "img_l2_loss", "img_ssim_loss", "eik_loss", "roughrange_loss")})
    assert all(np.isfinite(v) for rec in losses for v in rec.values())
    first, last = np.mean([r["loss"] for r in losses[:5]]), np.mean([r["loss"] for r in losses[-5:]])
    print("total loss: first five %.5f, last five %.5f, ratio %.3f" % (first, last, last / first))
    assert last < first


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_loads_into_relight_and_a_restart_resumes_bitwise(dataset, tmp_path):
    from iron_amd import relight
    out_dir = str(tmp_path / "run")
    a = _trainer(dataset, out_dir=out_dir, seed=4)
    a.step()
    a.step()
    ckpt, state = a.save_checkpoint()
    assert os.path.basename(ckpt) == "ckpt_1.pth" and os.path.basename(state) == "state_1.pth"
    sdf, nets = relight.load_networks(ckpt, DEV)
    for (n, p), (m, q) in zip(sdf.named_parameters(), a.sdf_network.named_parameters()):
        assert n == m and torch.equal(p, q)
    for k in relight.MATERIAL_KEYS:
        assert all(torch.equal(p, q) for p, q in zip(nets[k].parameters(), a.color_network_dict[k].parameters()))
    raw = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert set(raw) == {"sdf_network"} | set(a.color_network_dict)   # the reference's format: one state-dict per network

    b = _trainer(dataset, out_dir=out_dir, seed=99)   # the seed is overridden by the restored generator states
    assert b.global_step == 1
    pa, pb = _named_params(a), _named_params(b)
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
        sa, sb = a.optimizer.state[pa[n]], b.optimizer.state[pb[n]]
        assert float(sa["step"]) == float(sb["step"]) == 2
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    assert a.rng.bit_generator.state == b.rng.bit_generator.state
    assert torch.equal(a.device_rng.get_state(), b.device_rng.get_state())
    oa, ob = a.step(), b.step()
    assert oa["view"] == ob["view"] and oa["origin"] == ob["origin"]
    assert torch.equal(a.device_rng.get_state(), b.device_rng.get_state())   # the same eikonal points were drawn
    assert a.global_step == b.global_step == 2
    assert abs(float(oa["loss"]) - float(ob["loss"])) <= 1e-6 * abs(float(oa["loss"]))


def test_train_writes_its_line_checkpoints_and_validation_pictures_and_the_command_renders_all(dataset, tmp_path, capsys):
    from PIL import Image
    from iron_amd.train_surface import main
    out_dir = str(tmp_path / "loop")
    tr = _trainer(dataset, out_dir=out_dir, seed=2)
    last = tr.train(3, log_every=2, ckpt_every=2, image_every=2)
    assert tr.global_step == 2 and np.isfinite(float(last["loss"]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "global_step=" in ln]
    assert len(lines) == 2 and "global_step=0 " in lines[0] and "global_step=2 " in lines[1] and "roughrange_loss=" in lines[1]
    names = sorted(os.listdir(out_dir))
    assert [n for n in names if n.endswith(".pth")] == ["ckpt_0.pth", "ckpt_2.pth", "state_0.pth", "state_2.pth"]
    pictures = [n for n in names if n.startswith("logim_")]
    assert pictures == ["logim_0_0.png", "logim_2_2.png"]
    with Image.open(os.path.join(out_dir, pictures[1])) as im:
        assert im.size == (SIZE // 4, SIZE // 4) and im.mode == "RGB"
    tr.train(3)                      # nothing left to do
    assert tr.global_step == 2
    # the command on the same directory: picks up ckpt_2.pth and renders every view
    main(["--data_dir", dataset["dir"], "--out_dir", out_dir, "--renderer_name", "ggx", "--patch_size", "32", "--render_all"])
    rendered = os.path.join(out_dir, "render_%s_2" % os.path.basename(dataset["dir"]))
    assert sorted(os.listdir(rendered)) == sorted(s + suffix + ".png" for s in ("0", "1", "2", "10") for suffix in ("", "_normal", "_diff", "_specular"))
    with Image.open(os.path.join(rendered, "10.png")) as im:
        assert im.size == (SIZE, SIZE) and np.asarray(im).max() > 0


def test_two_steps_with_the_composite_renderer(dataset):
    """`comp` is the command's default (render_surface.py:107): 148 tensors, two launch tables, roughness as [H, W, 1]."""
    from iron_amd import scenes
    from iron_amd.network_conf import COMP_OPTIMIZED
    nets = {k: m.to(DEV) for k, m in scenes.build_comp_networks(seed=0).items()}
    nets["sdf_network"] = _target_networks()["sdf_network"]
    tr = _trainer(dataset, networks=nets, renderer_name="comp", seed=1)
    assert sum(len(g["params"]) for g in tr.optimizer.param_groups) > 80
    before = {n: p.detach().clone() for n, p in _named_params(tr).items()}
    outs = [tr.step(), tr.step()]
    assert all(np.isfinite(float(o[k])) for o in outs for k in ("loss", "img_l2_loss", "img_ssim_loss", "eik_loss", "roughrange_loss"))
    assert all(int(o["n_mask"]) > 0 for o in outs)
    moved = {k: False for k in COMP_OPTIMIZED if k in tr.color_network_dict}
    for n, p in _named_params(tr).items():
        assert bool(torch.isfinite(p).all()), n
        k = n.split(".")[0]
        if (k in moved or k == "sdf_network") and len(tr.optimizer.state.get(p, {})) > 0:
            assert float(tr.optimizer.state[p]["step"]) == 2, n
            if k in moved and not torch.equal(p, before[n]):
                moved[k] = True
    print("networks the composite loss moved:", sorted(k for k, v in moved.items() if v), "-- left alone:", sorted(k for k, v in moved.items() if not v))
    assert all(moved[k] for k in ("diffuse_albedo_network", "specular_albedo_network", "specular_roughness_network", "point_light_network")), moved


# ---- (f) ------------------------------------------------------------------------------------------------------------------------
def test_an_empty_mask_steps_on_the_eikonal_term_alone(dataset):
    from iron_amd import scenes
    from iron_amd.train_surface import SurfaceTrainer
    K, W2C = scenes.fixture_camera_matrices(SIZE, SIZE)
    away = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0])) @ W2C   # the same position, looking the other way
    tr = SurfaceTrainer(images=torch.zeros(1, SIZE, SIZE, 3), Ks=K[None], W2Cs=away[None], renderer_name="ggx", patch_size=32,
                        networks=_start_networks())
    before = {n: p.detach().clone() for n, p in _named_params(tr).items()}
    out = tr.step()
    assert int(out["n_mask"]) == 0 and float(out["img_l2_loss"]) == 0.0 and float(out["img_ssim_loss"]) == 0.0
    assert float(out["roughrange_loss"]) == 0.0 and float(out["eik_loss"]) > 0.0 and float(out["loss"]) == float(out["eik_loss"])
    for n, p in _named_params(tr).items():
        if n.startswith("sdf_network."):
            # (the last layer's bias shifts the SDF by a constant: its eikonal gradient is exactly zero, and so is its update)
            assert float(tr.optimizer.state[p]["step"]) == 1 and torch.equal(p, before[n]) == (int(torch.count_nonzero(p.grad)) == 0), n
        else:
            assert len(tr.optimizer.state[p]) == 0 and torch.equal(p, before[n]), n
