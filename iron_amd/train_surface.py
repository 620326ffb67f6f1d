"""Stage-2 training (render_surface.py) as a class and a command, without kornia, imageio, cv2, pyexr, tensorboard,
configargparse, icecream or Blender:

    python -m iron_amd.train_surface --data_dir DIR --out_dir OUT [--folder_name image] [--neus_ckpt_fpath CKPT]
                                     [--num_iters 100001] [--patch_size 128] [--eik_weight 0.1] [--ssim_weight 1.0]
                                     [--roughrange_weight 0.1] [--init_light_scale 8.0] [--inv_gamma_gt] [--gamma_pred]
                                     [--no_edgesample] [--renderer_name comp|ggx] [--seed 0] [--optimizer fused|torch]
                                     [--export_all | --render_all] [--gpu 0]

DIR is what iron_amd.dataset.load_datadir reads.  Every ckpt_every steps OUT receives ckpt_{step}.pth in the reference's format
(a dictionary of state-dicts: sdf_network plus one key per network of the dictionary; iron_amd.relight and the reference load it)
and, beside it, state_{step}.pth with what the reference does not keep: the optimiser state, the states of the two random
generators and the step number.  A run started on an OUT that holds checkpoints continues from the latest one; with its
state_{step}.pth it draws the views, patches and eikonal points the uninterrupted run would have drawn.

One step is one iteration of render_surface.py:533-653: a random patch of a random view rendered with is_training=True, the
pyramid L2 and masked SSIM losses on it, the eikonal and roughness-range regularisers (image_losses.surface_regularisers),
backward through the HIP operators, FusedAdam.  The metallic / dielectric terms of the `comp` branch, which the reference
computes and then leaves out of its loss (:643-645), are not built.
"""
from __future__ import annotations

import argparse
import glob
import json
import os

import numpy as np
import torch

from . import _lib
from .image_losses import PyramidL2Loss, ssim_loss_fn, surface_regularisers
from .network_conf import (COMP_OPTIMIZED, GGX_OPTIMIZED, choose_renderer_func, init_rendering_network_dict, init_sdf_network_dict)
from .optim import FusedAdam
from .raytracer import Camera, RayTracer, render_camera

SDF_LR, MATERIAL_LR, LIGHT_LR = 1e-5, 1e-4, 1e-2   # render_surface.py:112, models/network_conf.py:707-745
LOSS_KEYS = ("loss", "img_l2_loss", "img_ssim_loss", "eik_loss", "roughrange_loss")


def checkpoint_paths(out_dir):
    """The ckpt_*.pth files of `out_dir`, ordered by step as utils/ckpt_loader.py:load_ckpt orders them: [(step, path)]."""
    def step(p):
        return int(os.path.basename(p)[len("ckpt_"):-4])
    return [(step(p), p) for p in sorted(glob.glob(os.path.join(out_dir, "ckpt_*.pth")), key=step)]


def gamma_correction(image, gamma=2.2):
    """models/helper.py:14-18."""
    return torch.pow(image + 1e-6, 1.0 / gamma)


def torch_regularisers(eik_grad, normal, mask, roughness, edge_normal, eik_weight, roughrange_weight):
    """render_surface.py:580-613, 639 as the reference writes them (boolean indexing; `mask` holds at least one pixel): the baseline
    of tools/bench_train_surface.py and SurfaceTrainer(regularisers='torch')."""
    eik_cnt = eik_grad.shape[0]
    eik_loss = ((eik_grad.norm(dim=-1) - 1) ** 2).sum()
    g = normal[mask]
    eik_cnt += g.shape[0]
    eik_loss = eik_loss + ((g.norm(dim=-1) - 1) ** 2).sum()
    if edge_normal is not None:
        eik_cnt += edge_normal.shape[0]
        eik_loss = eik_loss + ((edge_normal.norm(dim=-1) - 1) ** 2).sum()
    r = roughness[mask]
    r = r[r > 0.5]
    rr = (r - 0.5).mean() * roughrange_weight if r.numel() > 0 else torch.zeros((), device=eik_grad.device)
    return eik_loss / eik_cnt * eik_weight, rr


class SurfaceTrainer:
    """Arguments as render_surface.py:42-95 names them.  The pictures come from `data_dir` / `folder_name` (load_datadir) or as
    tensors: images [N, H, W, C] (float in 0 .. 1 or uint8), Ks and W2Cs [N, 4, 4].  `networks` replaces the factory's networks
    (keys sdf_network, the material networks, point_light_network).  optimizer: 'fused' (FusedAdam) or 'torch' (torch.optim.Adam
    over the same three groups); regularisers: 'hip' (surface_regularisers) or 'torch' (torch_regularisers)."""

    def __init__(self, data_dir=None, out_dir=None, folder_name="image", images=None, Ks=None, W2Cs=None, renderer_name="comp",
                 patch_size=128, eik_weight=0.1, ssim_weight=1.0, roughrange_weight=0.1, init_light_scale=8.0, inv_gamma_gt=False,
                 gamma_pred=False, no_edgesample=False, neus_ckpt_fpath=None, seed=0, optimizer="fused", regularisers="hip",
                 networks=None, device=None):
        if renderer_name not in ("ggx", "comp"):
            raise _lib.IronError("SurfaceTrainer: renderer_name is 'ggx' or 'comp', got %r" % (renderer_name,))
        if optimizer not in ("fused", "torch") or regularisers not in ("hip", "torch"):
            raise _lib.IronError("SurfaceTrainer: optimizer is 'fused' or 'torch' and regularisers 'hip' or 'torch'")
        if not torch.cuda.is_available():
            raise _lib.IronError("SurfaceTrainer needs a GPU (iron_amd has no CPU path)")
        self.device = dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.out_dir, self.data_dir, self.renderer_name = out_dir, data_dir, renderer_name
        self.patch_size, self.eik_weight, self.ssim_weight, self.roughrange_weight = int(patch_size), eik_weight, ssim_weight, roughrange_weight
        self.inv_gamma_gt, self.gamma_pred, self.handle_edges = bool(inv_gamma_gt), bool(gamma_pred), not no_edgesample
        self.regularisers = regularisers

        if images is None:
            if data_dir is None:
                raise _lib.IronError("SurfaceTrainer: give data_dir or images, Ks, W2Cs")
            from .dataset import load_datadir
            self.image_fpaths, images, Ks, W2Cs = load_datadir(data_dir, folder_name)
        else:
            if Ks is None or W2Cs is None or len(Ks) != len(images) or len(W2Cs) != len(images):
                raise _lib.IronError("SurfaceTrainer: images, Ks and W2Cs must have one entry per view")
            self.image_fpaths = ["view_%d" % i for i in range(len(images))]
        images = torch.as_tensor(images)
        if images.dim() != 4 or images.shape[-1] < 3:
            raise _lib.IronError("SurfaceTrainer: images must be [N, H, W, C >= 3], got %s" % (tuple(images.shape),))
        if images.dtype != torch.uint8:  # kept on the device as uint8 (x / 255 gives back what an 8-bit picture file held)
            images = (images.to(dev, torch.float32) * 255.0).round().clamp(0.0, 255.0).to(torch.uint8)
        self.gt_u8 = images.to(dev).contiguous()
        n, h, w = self.gt_u8.shape[:3]
        if self.patch_size > min(h, w):
            raise _lib.IronError("SurfaceTrainer: patch_size %d exceeds the %dx%d pictures" % (self.patch_size, w, h))
        self.cameras = [Camera(W=w, H=h, K=torch.as_tensor(Ks[i]).float().to(dev), W2C=torch.as_tensor(W2Cs[i]).float().to(dev)) for i in range(n)]

        # the reference's order: networks, NeuS initialisation, light, latest checkpoint, optimisers
        self.raytracer = RayTracer()
        if networks is None:
            self.sdf_network = init_sdf_network_dict(dev)
            self.color_network_dict = init_rendering_network_dict(renderer_name, dev)
        else:
            self.sdf_network = networks["sdf_network"].to(dev)
            self.color_network_dict = {k: m.to(dev) for k, m in networks.items() if k != "sdf_network"}
        self.render_fn = choose_renderer_func(renderer_name)
        self.pyramidl2_loss_fn = PyramidL2Loss(use_cuda=True)
        self._load_neus_checkpoint(neus_ckpt_fpath)
        dist = float(np.median([float(torch.norm(c.get_camera_origin())) for c in self.cameras]))
        self.color_network_dict["point_light_network"].set_light(init_light_scale * dist * dist)
        self.global_step = -1   # the last finished step
        ckpts = checkpoint_paths(out_dir) if out_dir is not None else []
        if ckpts:
            self.global_step = self._load_checkpoint(ckpts[-1][1], ckpts[-1][0])

        optimized = COMP_OPTIMIZED if renderer_name == "comp" else GGX_OPTIMIZED
        materials = [p for k in optimized if k in self.color_network_dict and k != "point_light_network"
                     for p in self.color_network_dict[k].parameters()]
        groups = [{"params": list(self.sdf_network.parameters()), "lr": SDF_LR}, {"params": materials, "lr": MATERIAL_LR},
                  {"params": list(self.color_network_dict["point_light_network"].parameters()), "lr": LIGHT_LR}]
        self.optimizer = FusedAdam(groups) if optimizer == "fused" else torch.optim.Adam(groups)
        self.rng = np.random.default_rng(seed)
        self.device_rng = torch.Generator(device=dev).manual_seed(seed)
        if ckpts:
            self._load_state(os.path.join(out_dir, "state_%d.pth" % self.global_step))

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def _load_neus_checkpoint(self, path) -> None:
        """utils/ckpt_loader.py:49-65: sdf_network_fine -> the SDF network, color_network_fine -> the diffuse albedo network."""
        if path is None or not os.path.isfile(path):
            return
        ckpt = torch.load(path, map_location=self.device, weights_only=True)
        self.sdf_network.load_state_dict(ckpt["sdf_network_fine"])
        try:
            self.color_network_dict["diffuse_albedo_network"].load_state_dict(ckpt["color_network_fine"])
        except (KeyError, RuntimeError) as e:   # the reference goes on without it too
            print("train_surface: the diffuse albedo network is not initialised from %s (%s)" % (path, str(e).splitlines()[0]))

    def _load_checkpoint(self, path, step) -> int:
        ckpt = torch.load(path, map_location=self.device, weights_only=True)
        self.sdf_network.load_state_dict(ckpt["sdf_network"])
        for k, net in self.color_network_dict.items():
            if k in ckpt:
                net.load_state_dict(ckpt[k])
        return step

    def _load_state(self, path) -> None:
        if not os.path.isfile(path):   # a checkpoint of the reference: parameters only, the optimiser starts afresh
            return
        st = torch.load(path, map_location="cpu", weights_only=True)
        self.optimizer.load_state_dict(st["optimizer"])
        self.rng.bit_generator.state = json.loads(st["numpy_rng"])
        self.device_rng.set_state(st["device_rng"])
        self.global_step = int(st["global_step"])

    def save_checkpoint(self, step=None):
        """-> (ckpt path, state path)."""
        step = self.global_step if step is None else step
        os.makedirs(self.out_dir, exist_ok=True)
        save_dict = dict([("sdf_network", self.sdf_network.state_dict())]
                         + [(k, net.state_dict()) for k, net in self.color_network_dict.items()])
        ckpt_path, state_path = os.path.join(self.out_dir, "ckpt_%d.pth" % step), os.path.join(self.out_dir, "state_%d.pth" % step)
        torch.save(save_dict, ckpt_path)
        torch.save({"optimizer": self.optimizer.state_dict(), "numpy_rng": json.dumps(self.rng.bit_generator.state),
                    "device_rng": self.device_rng.get_state(), "global_step": step}, state_path)
        return ckpt_path, state_path

    # ---- one step -----------------------------------------------------------------------------------------------------------
    def draw(self):
        """The step's random choices, from the trainer's own generators: (view, (column, row) of the patch, eikonal points)."""
        idx = int(self.rng.integers(0, len(self.cameras)))
        cam, p = self.cameras[idx], self.patch_size
        origin = (int(self.rng.integers(0, cam.W - p)) if cam.W > p else 0, int(self.rng.integers(0, cam.H - p)) if cam.H > p else 0)
        eik_points = torch.empty(p * p // 2, 3, device=self.device).uniform_(-1.0, 1.0, generator=self.device_rng)
        return idx, origin, eik_points

    def gt_patch(self, idx, origin):
        """The float ground truth of a patch, [P, P, C], from the uint8 pictures on the device."""
        p = self.patch_size
        gt = self.gt_u8[idx, origin[1]:origin[1] + p, origin[0]:origin[0] + p].to(torch.float32) / 255.0
        return torch.pow(gt, 2.2) if self.inv_gamma_gt else gt

    def render_patch(self, idx, origin):
        camera_crop, _, _ = self.cameras[idx].crop_region(self.patch_size, self.patch_size, ul_corner=origin)
        results = render_camera(camera_crop, self.sdf_network, self.raytracer, self.color_network_dict, render_fn=self.render_fn,
                                fill_holes=True, handle_edges=self.handle_edges, is_training=True)
        if self.gamma_pred:
            for k in ("color", "diffuse_color", "specular_color"):
                results[k] = gamma_correction(results[k])
        return results

    def compute_losses(self, results, gt_patch, eik_grad):
        """render_surface.py:567-647 on one render: -> {"loss", "img_l2_loss", "img_ssim_loss", "eik_loss", "roughrange_loss",
        "n_mask"}, device scalars.  Reading whether the mask holds any pixel is its one host synchronisation (the reference's)."""
        mask = results["convergent_mask"]
        if self.handle_edges:
            mask = mask | results["edge_mask"]
        zero = torch.zeros((), dtype=torch.float32, device=mask.device)
        img_l2_loss = img_ssim_loss = zero
        edge = results.get("edge_pos_neg_normal")
        if bool(mask.any()):
            pred_img = results["color"].permute(2, 0, 1).unsqueeze(0)[:, :3].contiguous()
            gt_img = gt_patch.permute(2, 0, 1).unsqueeze(0).to(pred_img.device, dtype=pred_img.dtype)[:, :3].contiguous()
            img_l2_loss = self.pyramidl2_loss_fn(pred_img, gt_img)
            img_ssim_loss = self.ssim_weight * ssim_loss_fn(pred_img, gt_img, mask.unsqueeze(0).unsqueeze(0))
            if self.regularisers == "torch":
                rough = results["specular_roughness"].reshape(mask.shape)
                eik_loss, rr_loss = torch_regularisers(eik_grad, results["normal"], mask, rough, edge, self.eik_weight, self.roughrange_weight)
                n_mask = mask.sum()
            else:
                eik_loss, rr_loss, counts = surface_regularisers(eik_grad, results["normal"], mask, results["specular_roughness"], edge,
                                                                 self.eik_weight, self.roughrange_weight, return_counts=True)
                n_mask = counts[1]
        else:
            # only the uniform set counts (:591): the frame's maps stay out of the graph, so the material networks get no gradient
            # at all (None, not zeros) and the optimiser leaves them and their step counts alone, as in the reference
            if self.regularisers == "torch":
                eik_loss, rr_loss = ((eik_grad.norm(dim=-1) - 1) ** 2).sum() / eik_grad.shape[0] * self.eik_weight, zero
            else:
                eik_loss, rr_loss = surface_regularisers(eik_grad, results["normal"].detach(), mask, results["specular_roughness"].detach(),
                                                         None, self.eik_weight, self.roughrange_weight)
            n_mask = torch.zeros((), dtype=torch.int64, device=mask.device)
        loss = img_l2_loss + img_ssim_loss + eik_loss + rr_loss
        return {"loss": loss, "img_l2_loss": img_l2_loss, "img_ssim_loss": img_ssim_loss, "eik_loss": eik_loss, "roughrange_loss": rr_loss,
                "n_mask": n_mask}

    def step(self):
        """One iteration; -> the losses (detached device scalars), "n_mask", and the host values "view" and "origin"."""
        self.optimizer.zero_grad(set_to_none=True)
        idx, origin, eik_points = self.draw()
        results = self.render_patch(idx, origin)
        eik_grad = self.sdf_network.gradient(eik_points).view(-1, 3)
        out = self.compute_losses(results, self.gt_patch(idx, origin), eik_grad)
        out["loss"].backward()
        self.optimizer.step()
        self.global_step += 1
        out = {k: v.detach() for k, v in out.items()}
        out["view"], out["origin"] = idx, origin
        return out

    # ---- the loop -----------------------------------------------------------------------------------------------------------
    def validation_image(self, step, idx=None):
        """A quarter-size render of one view (is_training=False) written as logim_{step}_{name}.png; -> its path."""
        idx = step % len(self.cameras) if idx is None else idx
        camera_resize, _ = self.cameras[idx].resize(factor=0.25)
        with torch.no_grad():
            results = render_camera(camera_resize, self.sdf_network, self.raytracer, self.color_network_dict, render_fn=self.render_fn,
                                    fill_holes=True, handle_edges=self.handle_edges, is_training=False)
        color = results["color"][..., :3]
        if self.gamma_pred or self.inv_gamma_gt:
            color = gamma_correction(color)
        from .export_materials import _write_png, to8b
        os.makedirs(self.out_dir, exist_ok=True)
        name = os.path.splitext(os.path.basename(self.image_fpaths[idx]))[0]
        path = os.path.join(self.out_dir, "logim_%d_%s.png" % (step, name))
        _write_png(path, to8b(color.cpu().numpy()))
        return path

    def train(self, num_iters, log_every=100, ckpt_every=1000, image_every=None):
        """Steps global_step + 1 .. num_iters - 1 (render_surface.py:533).  image_every: None = log_every, 0 = never."""
        image_every = log_every if image_every is None else image_every
        out = None
        for step in range(self.global_step + 1, int(num_iters)):
            out = self.step()
            if ckpt_every and step % ckpt_every == 0 and self.out_dir is not None:
                self.save_checkpoint(step)
            if log_every and step % log_every == 0:
                v = {k: float(out[k]) for k in LOSS_KEYS}
                print("%s global_step=%d loss=%.6g img_loss=%.6g img_l2_loss=%.6g img_ssim_loss=%.6g eik_loss=%.6g roughrange_loss=%.6g light=%.6g"
                      % (self.out_dir, step, v["loss"], v["img_l2_loss"] + v["img_ssim_loss"], v["img_l2_loss"], v["img_ssim_loss"],
                         v["eik_loss"], v["roughrange_loss"], float(self.color_network_dict["point_light_network"].get_light())), flush=True)
            if image_every and step % image_every == 0 and self.out_dir is not None:
                self.validation_image(step)
        return out

    def render_all(self, out_dir=None):
        """Every view at full size (is_training=False): NAME.png, NAME_normal.png, NAME_diff.png, NAME_specular.png."""
        from .export_materials import _write_png, to8b
        out_dir = out_dir or os.path.join(self.out_dir, "render_%s_%d" % (os.path.basename(os.path.normpath(self.data_dir or "views")), self.global_step))
        os.makedirs(out_dir, exist_ok=True)
        for cam, fpath in zip(self.cameras, self.image_fpaths):
            with torch.no_grad():
                res = render_camera(cam, self.sdf_network, self.raytracer, self.color_network_dict, render_fn=self.render_fn,
                                    fill_holes=True, handle_edges=True, is_training=False)
            if self.gamma_pred:
                res["color"], res["diffuse_color"] = gamma_correction(res["color"]), gamma_correction(res["diffuse_color"])
                res["specular_color"] = torch.clamp(res["color"] - res["diffuse_color"], min=0.0)
            name = os.path.splitext(os.path.basename(fpath))[0]
            normal = res["normal"] / (res["normal"].norm(dim=-1, keepdim=True) + 1e-10)
            for suffix, img in (("", res["color"]), ("_normal", (normal + 1.0) / 2.0), ("_diff", res["diffuse_color"]),
                                ("_specular", res["specular_color"])):
                _write_png(os.path.join(out_dir, name + suffix + ".png"), to8b(img[..., :3].cpu().numpy()))
        return out_dir

    def export_all(self, out_dir=None):
        """mesh.obj (export_mesh), its UVs (export_uv) and the baked material textures (export_materials)."""
        from .export_materials import export_materials
        from .export_mesh import export_mesh
        from .export_uv import export_uv
        from .rendering_func import MaterialPredictor
        out_dir = out_dir or os.path.join(self.out_dir, "mesh_and_materials_%d" % self.global_step)
        os.makedirs(out_dir, exist_ok=True)
        mesh = os.path.join(out_dir, "mesh.obj")
        with torch.no_grad():
            export_mesh(lambda x: self.sdf_network(x)[..., 0], mesh)
            export_uv(mesh, mesh)
            export_materials(mesh, MaterialPredictor(self.sdf_network, self.color_network_dict), out_dir)
        return out_dir


def config_parser():
    """render_surface.py:42-95's names and defaults for what is built, plus --renderer_name, --seed, --optimizer and the loop's
    three periods."""
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--data_dir", type=str, default=None, help="input data directory")
    parser.add_argument("--out_dir", type=str, default=None, help="output directory")
    parser.add_argument("--folder_name", type=str, default="image", help="dataset image folder")
    parser.add_argument("--neus_ckpt_fpath", type=str, default=None, help="checkpoint to load")
    parser.add_argument("--num_iters", type=int, default=100001, help="number of iterations")
    parser.add_argument("--patch_size", type=int, default=128, help="width and height of the rendered patches")
    parser.add_argument("--eik_weight", type=float, default=0.1, help="weight for eikonal loss")
    parser.add_argument("--ssim_weight", type=float, default=1.0, help="weight for ssim loss")
    parser.add_argument("--roughrange_weight", type=float, default=0.1, help="weight for roughness range loss")
    parser.add_argument("--no_edgesample", action="store_true", help="whether to disable edge sampling")
    parser.add_argument("--inv_gamma_gt", action="store_true", help="whether to inverse gamma correct the ground-truth photos")
    parser.add_argument("--gamma_pred", action="store_true", help="whether to gamma correct the predictions")
    parser.add_argument("--init_light_scale", type=float, default=8.0, help="scaling parameters for light")
    parser.add_argument("--export_all", action="store_true", help="whether to export meshes and uv textures")
    parser.add_argument("--render_all", action="store_true", help="whether to render the input image set")
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--renderer_name", type=str, default="comp", choices=("ggx", "comp"))
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--optimizer", type=str, default="fused", choices=("fused", "torch"))
    parser.add_argument("--log_every", type=int, default=100)
    parser.add_argument("--ckpt_every", type=int, default=1000)
    parser.add_argument("--image_every", type=int, default=None)
    return parser


def main(argv=None) -> None:
    parser = config_parser()
    a = parser.parse_args(argv)
    if a.data_dir is None or a.out_dir is None:
        parser.error("--data_dir and --out_dir are required")
    if not torch.cuda.is_available():
        raise SystemExit("iron_amd.train_surface needs a GPU (iron_amd has no CPU path)")
    torch.cuda.set_device(a.gpu)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "args.txt"), "w") as fp:
        fp.writelines("%s = %s\n" % kv for kv in sorted(vars(a).items()))
    trainer = SurfaceTrainer(data_dir=a.data_dir, out_dir=a.out_dir, folder_name=a.folder_name, renderer_name=a.renderer_name,
                             patch_size=a.patch_size, eik_weight=a.eik_weight, ssim_weight=a.ssim_weight,
                             roughrange_weight=a.roughrange_weight, init_light_scale=a.init_light_scale, inv_gamma_gt=a.inv_gamma_gt,
                             gamma_pred=a.gamma_pred, no_edgesample=a.no_edgesample, neus_ckpt_fpath=a.neus_ckpt_fpath, seed=a.seed,
                             optimizer=a.optimizer)
    if a.export_all:
        print("exported to", trainer.export_all())
        return
    if a.render_all:
        print("rendered to", trainer.render_all())
        return
    trainer.train(a.num_iters, log_every=a.log_every, ckpt_every=a.ckpt_every, image_every=a.image_every)
    trainer.export_all()


if __name__ == "__main__":
    main()
