"""VolumeTrainer (iron_amd/train_volume.py) and VolumeDataset (iron_amd/dataset.py) on a dataset the test writes itself: four
32 x 32 views of scenes.build_networks("S1", seed=5) at four yaws of the fixture camera, as PNG plus cam_dict_norm.json, and a
settings text with the model blocks of tests/golden/womask_iron.conf."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZE = 32
NAMES = ["10.png", "0.png", "2.png", "1.png"]
YAWS = {"0.png": 0.0, "1.png": 90.0, "2.png": 180.0, "10.png": 270.0}
ORDERED = ["0.png", "1.png", "2.png", "10.png"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from iron_amd import scenes
    from iron_amd.dataset import to8b
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    root = tmp_path_factory.mktemp("s1_volume_views")
    os.makedirs(root / "image")
    nets = {k: m.to(DEV) for k, m in scenes.build_networks("S1", seed=5).items()}
    fn = make_render_fn(GGXColocatedRenderer(use_cuda=True))
    cam_dict, pixels = {}, {}
    for name in NAMES:
        K, W2C = scenes.fixture_camera_matrices(SIZE, SIZE, yaw_deg=YAWS[name])
        with torch.no_grad():
            res = render_camera(Camera(SIZE, SIZE, K.to(DEV), W2C.to(DEV)), nets["sdf_network"], RayTracer(), nets, fn, fill_holes=True,
                                handle_edges=True, is_training=False)
        img8 = to8b(res["color"].cpu().numpy())
        Image.fromarray(img8).save(str(root / "image" / name))
        cam_dict[name] = {"K": [float(x) for x in K.reshape(-1)], "W2C": [float(x) for x in W2C.reshape(-1)], "img_size": [SIZE, SIZE]}
        pixels[name] = img8
    with open(root / "cam_dict_norm.json", "w") as fp:
        json.dump(cam_dict, fp)
    assert all(p.max() > 0 for p in pixels.values())
    return {"dir": str(root), "pixels": pixels}


def conf_text(dataset, exp_dir, **train):
    """The model blocks of womask_iron.conf under the test's own general / dataset / train blocks."""
    text = open(os.path.join(GOLDEN, "womask_iron.conf")).read()
    model = text[text.index("model {"):]
    values = dict(learning_rate="5e-4", learning_rate_alpha=0.05, end_iter=3, batch_size=64, validate_resolution_level=4, warm_up_end=2,
                  anneal_end=4, use_white_bkgd=False, save_freq=2, val_freq=1000, val_mesh_freq=1000, report_freq=1, igr_weight=0.1,
                  mask_weight=0.0)
    values.update(train)
    perturb = values.pop("perturb", None)
    if perturb is not None:
        model = model.replace("perturb = 1.0", "perturb = %s" % perturb)
        assert "perturb = %s" % perturb in model
    lines = "\n".join("    %s = %s" % kv for kv in values.items())
    return ("general {\n    base_exp_dir = %s\n    recording = [\n        ./,\n        ./models\n    ]\n}\n\n"
            "dataset {\n    data_dir = %s/\n    render_cameras_name = cameras_sphere.npz\n}\n\ntrain {\n%s\n}\n\n%s" % (exp_dir, dataset["dir"], lines, model))


def _stage1():
    """Stage-1 networks at torch.manual_seed(0) in the construction order of tests/test_gpu_neus.py::_stage1."""
    from iron_amd.fields import NeRF, RenderingNetwork, SDFNetwork, SingleVarianceNetwork
    torch.manual_seed(0)
    return {
        "sdf_network": SDFNetwork(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=[4], multires=6, bias=0.5, scale=1.0,
                                  geometric_init=True, weight_norm=True),
        "color_network": RenderingNetwork(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=8, skip_in=[4],
                                          weight_norm=True, multires=10, multires_view=4, squeeze_out=True),
        "nerf": NeRF(D=8, d_in=4, d_in_view=3, W=256, multires=10, multires_view=4, output_ch=4, skips=[4], use_viewdirs=True),
        "deviation_network": SingleVarianceNetwork(0.3),
    }


def _fixed_batch(batch=32):
    """The synthetic rays and targets of tools/neus_train_step.py (generator seed 1), with a mask of ones -> [batch, 10] on the CPU."""
    g = torch.Generator().manual_seed(1)
    d = F.normalize(torch.randn(batch, 3, generator=g) * torch.tensor([0.25, 0.25, 0.0]) + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    o = torch.tensor([[0.0, 0.0, -2.5]]).expand(batch, 3).contiguous()
    true_rgb = torch.rand(batch, 3, generator=g)
    return torch.cat([o, d, true_rgb, torch.ones(batch, 1)], dim=-1)


# ---- the dataset -------------------------------------------------------------------------------------------------------------------
def test_random_rays_of_two_datasets_with_one_seed_are_equal_and_show_the_written_pixels(dataset):
    from iron_amd.conf import parse_string
    from iron_amd.dataset import VolumeDataset
    a = VolumeDataset(parse_string(conf_text(dataset, "unused"))["dataset"], device=DEV)
    b = VolumeDataset(data_dir=dataset["dir"], device=DEV)
    assert (a.n_images, a.H, a.W) == (4, SIZE, SIZE) and [os.path.basename(p) for p in a.images_lis] == ORDERED
    for view in (0, 3):
        ga, gb = torch.Generator(device=DEV).manual_seed(11), torch.Generator(device=DEV).manual_seed(11)
        ra, rb = a.gen_random_rays_at(view, 64, generator=ga), b.gen_random_rays_at(view, 64, generator=gb)
        assert tuple(ra.shape) == (64, 10) and torch.equal(ra, rb)
        g = torch.Generator(device=DEV).manual_seed(11)
        px = torch.randint(low=0, high=SIZE, size=[64], device=DEV, generator=g).cpu().numpy()
        py = torch.randint(low=0, high=SIZE, size=[64], device=DEV, generator=g).cpu().numpy()
        want = torch.from_numpy(dataset["pixels"][ORDERED[view]][py, px].astype(np.float32) / 255.0)
        assert torch.equal(ra[:, 6:9].cpu(), want) and bool((ra[:, 9] == 1).all())
        near, far = a.near_far_from_sphere(ra[:, :3], ra[:, 3:6])
        assert bool((far - near - 2.0).abs().max() < 1e-5)


# ---- the two tails on one batch ----------------------------------------------------------------------------------------------------
def test_first_step_losses_of_the_two_tails_agree(dataset, tmp_path):
    """The HIP tail against the torch expressions on ONE render: within 4 x the error of the fp32 torch evaluation against the fp64
    one, and never less than 1e-6 of the value (the yardstick of tests/test_gpu_volume_loss.py).  Then a step of each arm on the
    same batch from the same networks and seed: their losses agree within 3e-4, the bound the fixed-batch test below gives a
    colour loss (three channels x the project's 1e-4 per-ray colour bound)."""
    import copy
    from iron_amd.dataset import VolumeDataset
    from iron_amd.train_volume import LOSS_KEYS, VolumeTrainer, torch_losses
    ds = VolumeDataset(data_dir=dataset["dir"], device=DEV)
    nets = _stage1()
    kw = dict(dataset=ds, mode="validate", seed=4)
    hip = VolumeTrainer(conf_text(dataset, str(tmp_path / "hip"), mask_weight=0.1, warm_up_end=0), networks=copy.deepcopy(nets), **kw)
    tor = VolumeTrainer(conf_text(dataset, str(tmp_path / "torch"), mask_weight=0.1, warm_up_end=0), networks=copy.deepcopy(nets),
                        tail="torch", optimizer="torch", **kw)
    batch = ds.gen_random_rays_at(2, 64, generator=torch.Generator(device=DEV).manual_seed(5))
    with torch.no_grad():
        render_out = hip.render_batch(batch)
    got = hip.compute_losses(render_out, batch)
    as32 = torch_losses(render_out, batch[:, 6:9], batch[:, 9:10], 0.1, 0.1)
    out64 = {k: v.double() for k, v in render_out.items()}
    as64 = torch_losses(out64, batch[:, 6:9].double(), batch[:, 9:10].double(), 0.1, 0.1)
    for k in LOSS_KEYS:
        w64, w32, g = float(as64[k]), float(as32[k]), float(got[k])
        tol = max(4.0 * abs(w32 - w64), 1e-6 * abs(w64))
        print("%-16s hip %.9g  torch fp32 %.9g  fp64 %.9g  tol %.2e" % (k, g, w32, w64, tol))
        assert abs(g - w64) <= tol, k
    hip.generator.manual_seed(4)   # the render above drew its jitter from it: both arms start from the seed again
    a, b = hip.step(batch), tor.step(batch)
    assert hip.iter_step == tor.iter_step == 1 and a["view"] is None
    for k in LOSS_KEYS:
        print("step %-16s hip %.9g  torch %.9g" % (k, float(a[k]), float(b[k])))
        assert abs(float(a[k]) - float(b[k])) <= 3e-4 * max(1.0, abs(float(b[k]))), k
    # a drawn batch of the torch arm (the reference's host batch) is a batch of the dataset as well
    c = tor.step()
    assert tuple(tor.last_batch.shape) == (64, 10) and c["view"] in range(4) and bool(torch.isfinite(c["loss"]))
    img = torch.from_numpy(dataset["pixels"][ORDERED[c["view"]]].astype(np.float32) / 255.0).reshape(-1, 3)
    rows = (tor.last_batch[:, None, 6:9].cpu() == img[None]).all(dim=-1).any(dim=-1)
    assert bool(rows.all())


# ---- fixed-batch descent against the oracle -------------------------------------------------------------------------------------
def _oracle_descent(batch, steps):
    """The same loop on oracle.neus_ref.render_train with torch.optim.Adam, on the CPU (about 3 s)."""
    from _util import cpu_sd
    from oracle import iron_ref as R
    from oracle import neus_ref as N
    from oracle import train_ref as T
    nets = _stage1()
    sd = {k: T.leaf_state(cpu_sd(nets[k])) for k in ("sdf_network", "color_network", "nerf")}
    var = nets["deviation_network"].variance.detach().clone().requires_grad_(True)
    sc = N.NeusScene(sd["sdf_network"], R.SDFSpec(), sd["color_network"], sd["nerf"], var)
    params = [p for k in ("nerf", "sdf_network") for p in sd[k].values() if p.requires_grad] + [var]
    params += [p for p in sd["color_network"].values() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=5e-4)
    o, d, true_rgb, mask = batch[:, :3], batch[:, 3:6], batch[:, 6:9], batch[:, 9:10]
    mid = -(o * d).sum(-1, keepdim=True)
    history = []
    for _ in range(steps):
        out = N.render_train(sc, o, d, mid - 1.0, mid + 1.0, background_rgb=None, cos_anneal_ratio=1.0)
        mask_sum = mask.sum() + 1e-5
        color_error = (out["color_fine"] - true_rgb) * mask
        color_fine_loss = F.l1_loss(color_error, torch.zeros_like(color_error), reduction="sum") / mask_sum
        mask_loss = F.binary_cross_entropy(out["weight_sum"].clip(1e-3, 1.0 - 1e-3), mask)
        loss = color_fine_loss + out["gradient_error"] * 0.1 + mask_loss * 0.1
        opt.zero_grad()
        loss.backward()
        opt.step()
        history.append((float(color_fine_loss), float(loss)))
    return history


def test_fixed_batch_descent_against_the_oracle(dataset, tmp_path):
    """12 steps on one 32-ray batch at a constant rate of 5e-4, perturb = 0, cos_anneal_ratio = 1, igr_weight = mask_weight = 0.1.
    The oracle's loop gives colour loss 1.4254 -> 0.7654 (ratio 0.54) and total loss 1.4284 -> 0.7728 on the CPU.  Asserted: the
    step-0 colour loss within 3e-4 of the oracle's (three channels x the 1e-4 per-ray colour bound), every loss finite, the step-11
    colour loss below 0.8 x step 0 (the wiring, not a rate).  The later steps are printed beside the oracle's."""
    from iron_amd.dataset import VolumeDataset
    from iron_amd.train_volume import VolumeTrainer
    steps = 12
    batch = _fixed_batch(32)
    oracle = _oracle_descent(batch, steps)
    text = conf_text(dataset, str(tmp_path / "exp"), warm_up_end=0, anneal_end=0, learning_rate_alpha=1.0, end_iter=100, igr_weight=0.1,
                     mask_weight=0.1, perturb="0.0")
    tr = VolumeTrainer(text, mode="validate", dataset=VolumeDataset(data_dir=dataset["dir"], device=DEV), networks=_stage1(), seed=0)
    assert tr.renderer.perturb == 0.0 and tr.get_cos_anneal_ratio() == 1.0
    gpu_batch = batch.to(DEV)
    history = []
    for i in range(steps):
        out = tr.step(gpu_batch)
        assert out["lr"] == 5e-4
        history.append((float(out["color_fine_loss"]), float(out["loss"])))
        print("step %2d  colour %.6f (oracle %.6f)  loss %.6f (oracle %.6f)" % (i, history[-1][0], oracle[i][0], history[-1][1], oracle[i][1]))
    assert abs(oracle[0][0] - 1.4254) < 5e-4 and oracle[-1][0] < 0.8 * oracle[0][0], "the oracle's own run has moved"
    assert abs(history[0][0] - oracle[0][0]) <= 3e-4
    assert all(np.isfinite(v) for h in history for v in h)
    assert history[-1][0] < 0.8 * history[0][0]


# ---- the command: checkpoints, restart, validation -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(dataset, tmp_path_factory):
    """Three steps of `python -m iron_amd.train_volume --conf CONF --case duck` with save_freq = 2."""
    from iron_amd.train_volume import main
    root = tmp_path_factory.mktemp("stage1_run")
    conf_path = str(root / "test.conf")
    with open(conf_path, "w") as fp:
        fp.write(conf_text(dataset, str(root / "exp_CASE_NAME")))
    trainer = main(["--conf", conf_path, "--case", "duck", "--seed", "3"])
    return {"trainer": trainer, "conf": conf_path, "exp": str(root / "exp_duck")}


def test_three_steps_from_the_command_write_the_reference_checkpoint(run, dataset):
    from iron_amd.fields import NeRF, RenderingNetwork, SDFNetwork, SingleVarianceNetwork
    from iron_amd.train_surface import SurfaceTrainer
    tr = run["trainer"]
    assert tr.iter_step == 3 and tr.base_exp_dir == run["exp"]
    folder = os.path.join(run["exp"], "checkpoints")
    assert sorted(os.listdir(folder)) == ["ckpt_000002.pth", "state_000002.pth"]
    assert os.path.isfile(os.path.join(run["exp"], "recording", "config.conf"))
    ckpt = torch.load(os.path.join(folder, "ckpt_000002.pth"), map_location="cpu", weights_only=True)
    assert set(ckpt) == {"nerf", "sdf_network_fine", "variance_network_fine", "color_network_fine", "optimizer", "iter_step"}
    assert ckpt["iter_step"] == 2
    # it loads into the reference's modules' shapes and into torch.optim.Adam over them, in the Runner's parameter order
    conf = tr.conf
    nets = [NeRF(**conf["model.nerf"]), SDFNetwork(**conf["model.sdf_network"]), SingleVarianceNetwork(**conf["model.variance_network"]),
            RenderingNetwork(**conf["model.rendering_network"])]
    for net, key in zip(nets, ("nerf", "sdf_network_fine", "variance_network_fine", "color_network_fine")):
        net.load_state_dict(ckpt[key])
    params = [p for net in nets for p in net.parameters()]
    adam = torch.optim.Adam(params, lr=5e-4)
    adam.load_state_dict(ckpt["optimizer"])
    state = adam.state_dict()["state"]
    assert len(state) > 0 and all(float(s["step"]) == 2.0 and s["exp_avg"].shape == params[i].shape for i, s in state.items())
    # step 0 ran at lr = 0 (warm-up), steps 1 and 2 at 2.5e-4 and 5e-4: the group's rate in the file is the one of the next step
    assert ckpt["optimizer"]["param_groups"][0]["lr"] == pytest.approx(5e-4)
    # stage 2 initialises its SDF from the file, bit for bit
    st2 = SurfaceTrainer(data_dir=dataset["dir"], out_dir=None, patch_size=32, renderer_name="ggx", neus_ckpt_fpath=os.path.join(folder, "ckpt_000002.pth"))
    for k, v in st2.sdf_network.state_dict().items():
        assert torch.equal(v.cpu(), ckpt["sdf_network_fine"][k]), k


def test_restart_restores_everything_and_draws_the_next_batch(run):
    from iron_amd.train_volume import VolumeTrainer
    a = run["trainer"]
    folder = os.path.join(run["exp"], "checkpoints")
    ckpt = torch.load(os.path.join(folder, "ckpt_000002.pth"), map_location="cpu", weights_only=True)
    state = torch.load(os.path.join(folder, "state_000002.pth"), map_location="cpu", weights_only=True)
    b = VolumeTrainer(run["conf"], case="duck", is_continue=True, seed=99)          # another seed: the state comes from the file
    assert b.iter_step == 2 and b.base_exp_dir == run["exp"]
    for key, net in zip(("nerf", "sdf_network_fine", "variance_network_fine", "color_network_fine"), b.networks().values()):
        for k, v in net.state_dict().items():
            assert torch.equal(v.cpu(), ckpt[key][k]), (key, k)
    got = b.optimizer.state_dict()
    assert got["param_groups"] == ckpt["optimizer"]["param_groups"] and sorted(got["state"]) == sorted(ckpt["optimizer"]["state"])
    for i, s in ckpt["optimizer"]["state"].items():
        assert float(got["state"][i]["step"]) == float(s["step"]) == 2.0
        assert torch.equal(got["state"][i]["exp_avg"].cpu(), s["exp_avg"]) and torch.equal(got["state"][i]["exp_avg_sq"].cpu(), s["exp_avg_sq"])
    assert torch.equal(b.generator.get_state(), state["generator"]) and torch.equal(b.host_generator.get_state(), state["host_generator"])
    assert torch.equal(b.image_perm, state["image_perm"])
    assert b.optimizer.param_groups[0]["lr"] == pytest.approx(5e-4)
    out = b.step()
    assert b.iter_step == 3 and torch.equal(b.last_batch, a.last_batch), "the restart draws the uninterrupted run's third batch"
    assert bool(torch.isfinite(out["loss"]))


def test_validate_image_and_mesh(run):
    from PIL import Image
    tr = run["trainer"]
    img_path, normal_path = tr.validate_image(idx=0, resolution_level=4)
    assert img_path == os.path.join(run["exp"], "validations_fine", "00000003_0_0.png")
    assert normal_path == os.path.join(run["exp"], "normals", "00000003_0_0.png")
    with Image.open(img_path) as im:
        assert im.size == (8, 16) and im.mode == "RGB"                 # the render over the ground truth
        both = np.asarray(im)
    assert np.array_equal(both[8:], tr.dataset.image_at(0, 4))
    with Image.open(normal_path) as im:
        assert im.size == (8, 8) and im.mode == "RGB"
        assert np.asarray(im).std() > 0
    path = tr.validate_mesh(resolution=32)
    assert path == os.path.join(run["exp"], "meshes", "00000003.ply")
    raw = open(path, "rb").read()
    head = raw.split(b"end_header\n", 1)[0].decode("ascii").split("\n")
    nv = int([ln for ln in head if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in head if ln.startswith("element face")][0].split()[-1])
    assert nv > 0 and nf > 0 and len(raw) == len(raw.split(b"end_header\n", 1)[0]) + len(b"end_header\n") + 12 * nv + 13 * nf


# ---- the additive argument -----------------------------------------------------------------------------------------------------------
def test_render_with_generator_none_is_render_as_before():
    from iron_amd.renderer import NeuSRenderer
    nets = {k: v.to(DEV) for k, v in _stage1().items()}
    r = NeuSRenderer(nets["nerf"], nets["sdf_network"], nets["deviation_network"], nets["color_network"], n_samples=64, n_importance=64,
                     n_outside=32, up_sample_steps=4, perturb=1.0)
    batch = _fixed_batch(16).to(DEV)
    o, d = batch[:, :3], batch[:, 3:6]
    mid = -(o * d).sum(-1, keepdim=True)
    keys = ("color_fine", "weights", "weight_sum", "cdf_fine", "inside_sphere")

    def render(**kw):
        with torch.no_grad():
            return r.render(o, d, mid - 1.0, mid + 1.0, cos_anneal_ratio=1.0, **kw)
    torch.manual_seed(21)
    before = render()
    torch.manual_seed(21)
    none = render(generator=None)
    for k in keys:
        assert torch.equal(before[k], none[k]), k
    # an own generator replaces the global one: the same seed draws the same jitter, whatever the global generator does
    own = render(generator=torch.Generator(device=DEV).manual_seed(8))
    torch.manual_seed(1234)
    again = render(generator=torch.Generator(device=DEV).manual_seed(8))
    other = render(generator=torch.Generator(device=DEV).manual_seed(9))
    assert all(torch.equal(own[k], again[k]) for k in keys) and not torch.equal(own["weights"], other["weights"])
