"""Stage-1 training (render_volume.py) as a class and a command, without pyhocon, cv2, trimesh, tensorboard, icecream or tqdm
(DESIGN.md §22):

    python -m iron_amd.train_volume --conf CONF --case NAME [--mode train|validate_image|validate_mesh] [--is_continue]
                                    [--mcube_threshold 0.0] [--gpu 0] [--seed 0] [--optimizer fused|torch] [--tail hip|torch]

CONF is one of the reference's confs/*.conf (iron_amd.conf reads it, CASE_NAME replaced by NAME); dataset.data_dir is a directory
that iron_amd.dataset.load_datadir reads.  Under general.base_exp_dir the run writes

    checkpoints/ckpt_{:0>6d}.pth    the reference's keys: nerf, sdf_network_fine, variance_network_fine, color_network_fine,
                                    optimizer, iter_step (FusedAdam keeps torch.optim.Adam's state layout, so the reference and
                                    torch.optim.Adam load it; `python -m iron_amd.train_surface --neus_ckpt_fpath` consumes it)
    checkpoints/state_{:0>6d}.pth   what the reference does not keep: the states of the two random generators and the current view
                                    permutation; with it --is_continue draws what the uninterrupted run would have drawn
    validations_fine/, normals/     validate_image: {:0>8d}_0_{view}.png (render stacked over the ground truth; the normal picture)
    meshes/{:0>8d}.ply              validate_mesh
    recording/config.conf           the settings file

One step is one iteration of render_volume.py:443-528: the batch of a random view (VolumeDataset.gen_random_rays_at: csrc/volume.hip),
NeuSRenderer.render under autograd, the loss (image_losses.volume_losses: csrc/volume_loss.hip), backward through the HIP
operators, FusedAdam, the learning-rate schedule.  tail='torch' and optimizer='torch' select the reference's own arrangement -- the
batch indexed on the host and copied over, the loss as torch expressions, torch.optim.Adam -- as the baseline of
tools/bench_train_volume.py.
"""
from __future__ import annotations

import argparse
import glob
import os
import shutil

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .conf import Conf, parse_file, parse_string
from .image_losses import volume_losses
from .optim import FusedAdam

NETWORK_KEYS = ("nerf", "sdf_network", "deviation_network", "color_network")   # the optimiser's parameter order (:82-89)
CKPT_KEYS = {"nerf": "nerf", "sdf_network": "sdf_network_fine", "deviation_network": "variance_network_fine",
             "color_network": "color_network_fine"}
LOSS_KEYS = ("loss", "color_fine_loss", "eikonal_loss", "mask_loss", "psnr", "cdf", "weight_max", "mask_sum")


def checkpoint_name(iter_step) -> str:
    return "ckpt_{:0>6d}.pth".format(int(iter_step))


def state_name(iter_step) -> str:
    return "state_{:0>6d}.pth".format(int(iter_step))


def latest_checkpoint(exp_dir):
    """render_volume.py:530-543: the last of checkpoints/*.pth by name (state_*.pth files are ours and do not count), or None."""
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(exp_dir, "checkpoints", "ckpt_*.pth")))
    return names[-1] if names else None


def learning_factor(iter_step, warm_up_end, end_iter, learning_rate_alpha) -> float:
    """render_volume.py:554-560: linear warm-up to warm_up_end, then the cosine down to learning_rate_alpha."""
    if iter_step < warm_up_end:
        return iter_step / warm_up_end
    progress = (iter_step - warm_up_end) / (end_iter - warm_up_end)
    return float((np.cos(np.pi * progress) + 1.0) * 0.5 * (1 - learning_rate_alpha) + learning_rate_alpha)


def cos_anneal_ratio(iter_step, anneal_end) -> float:
    """render_volume.py:548-552."""
    if anneal_end == 0.0:
        return 1.0
    return float(np.min([1.0, iter_step / anneal_end]))


def torch_losses(render_out, true_rgb, mask, igr_weight, mask_weight):
    """render_volume.py:458-496, 507-510 as the reference writes them: the baseline of tools/bench_train_volume.py and
    VolumeTrainer(tail='torch').  -> the dictionary volume_losses returns."""
    if mask_weight > 0.0:
        mask = (mask > 0.5).to(mask.dtype)
    else:
        mask = torch.ones_like(mask)
    mask_sum = mask.sum() + 1e-5
    color_fine, weight_sum = render_out["color_fine"], render_out["weight_sum"].reshape(-1, 1)
    color_error = (color_fine - true_rgb) * mask
    color_fine_loss = F.l1_loss(color_error, torch.zeros_like(color_error), reduction="sum") / mask_sum
    psnr = 20.0 * torch.log10(1.0 / (((color_fine - true_rgb) ** 2 * mask).sum() / (mask_sum * 3.0)).sqrt())
    eikonal_loss = render_out["gradient_error"]
    mask_loss = F.binary_cross_entropy(weight_sum.clip(1e-3, 1.0 - 1e-3), mask)
    loss = color_fine_loss + eikonal_loss * igr_weight + mask_loss * mask_weight
    return {"loss": loss, "color_fine_loss": color_fine_loss, "eikonal_loss": eikonal_loss, "mask_loss": mask_loss, "psnr": psnr,
            "cdf": (render_out["cdf_fine"][:, :1] * mask).sum() / mask_sum,
            "weight_max": (render_out["weight_max"].reshape(-1, 1) * mask).sum() / mask_sum, "mask_sum": mask_sum}


class VolumeTrainer:
    """render_volume.py's Runner for the `Dataset` class.  conf: a settings file's path, its text (CASE_NAME already replaced) or
    a parsed iron_amd.conf.Conf; case replaces CASE_NAME in a file.  dataset: a VolumeDataset instead of conf["dataset"].
    networks: {"nerf", "sdf_network", "deviation_network", "color_network"} instead of the networks of conf["model.*"].
    optimizer: 'fused' (FusedAdam) or 'torch' (torch.optim.Adam); tail: 'hip' (device batches, volume_losses) or 'torch' (the
    reference's host batch and torch expressions)."""

    def __init__(self, conf, mode="train", case="CASE_NAME", is_continue=False, dataset=None, networks=None, seed=0, optimizer="fused",
                 tail="hip", device=None):
        if optimizer not in ("fused", "torch") or tail not in ("hip", "torch"):
            raise _lib.IronError("VolumeTrainer: optimizer is 'fused' or 'torch' and tail 'hip' or 'torch'")
        if not torch.cuda.is_available():
            raise _lib.IronError("VolumeTrainer needs a GPU (iron_amd has no CPU path)")
        self.device = dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.conf_path = None
        if isinstance(conf, Conf):
            self.conf = conf
        elif isinstance(conf, str) and "\n" not in conf and os.path.isfile(conf):
            self.conf_path, self.conf = conf, parse_file(conf, case=case)
        elif isinstance(conf, str):
            self.conf = parse_string(conf)
        else:
            raise _lib.IronError("VolumeTrainer: conf is a settings file, its text or a parsed Conf")
        conf = self.conf
        self.base_exp_dir = conf["general.base_exp_dir"]
        self.tail, self.mode, self.is_continue = tail, mode, is_continue
        self.iter_step = 0

        # training parameters (:47-66), with the reference's defaults
        self.end_iter = conf.get_int("train.end_iter")
        self.save_freq = conf.get_int("train.save_freq")
        self.report_freq = conf.get_int("train.report_freq")
        self.val_freq = conf.get_int("train.val_freq")
        self.val_mesh_freq = conf.get_int("train.val_mesh_freq")
        self.batch_size = conf.get_int("train.batch_size")
        self.validate_resolution_level = conf.get_int("train.validate_resolution_level")
        self.learning_rate = conf.get_float("train.learning_rate")
        self.learning_rate_alpha = conf.get_float("train.learning_rate_alpha")
        self.use_white_bkgd = conf.get_bool("train.use_white_bkgd")
        self.warm_up_end = conf.get_float("train.warm_up_end", default=0.0)
        self.anneal_end = conf.get_float("train.anneal_end", default=0.0)
        self.igr_weight = conf.get_float("train.igr_weight")
        self.mask_weight = conf.get_float("train.mask_weight")

        from .dataset import VolumeDataset
        self.dataset = VolumeDataset(conf["dataset"], mask_weight=self.mask_weight, device=dev) if dataset is None else dataset

        # networks, optimiser, renderer, checkpoint: the Runner's order (:72-131)
        from .fields import NeRF, RenderingNetwork, SDFNetwork, SingleVarianceNetwork
        from .renderer import NeuSRenderer
        if networks is None:
            self.nerf_outside = NeRF(**conf["model.nerf"]).to(dev)
            self.sdf_network = SDFNetwork(**conf["model.sdf_network"]).to(dev)
            self.deviation_network = SingleVarianceNetwork(**conf["model.variance_network"]).to(dev)
            self.color_network = RenderingNetwork(**conf["model.rendering_network"]).to(dev)
        else:
            missing = [k for k in NETWORK_KEYS if k not in networks]
            if missing:
                raise _lib.IronError("VolumeTrainer: networks lacks %s" % ", ".join(missing))
            self.nerf_outside, self.sdf_network = networks["nerf"].to(dev), networks["sdf_network"].to(dev)
            self.deviation_network, self.color_network = networks["deviation_network"].to(dev), networks["color_network"].to(dev)
        params_to_train = [p for net in self.networks().values() for p in net.parameters()]
        self.optimizer = (FusedAdam(params_to_train, lr=self.learning_rate) if optimizer == "fused"
                          else torch.optim.Adam(params_to_train, lr=self.learning_rate))
        self.renderer = NeuSRenderer(self.nerf_outside, self.sdf_network, self.deviation_network, self.color_network,
                                     **conf["model.neus_renderer"])
        self.background_rgb = torch.ones([1, 3], device=dev) if self.use_white_bkgd else None

        # the trainer owns its random numbers: pixels and sample jitter from the device generator, view order from the host one
        self.generator = torch.Generator(device=dev).manual_seed(seed)
        self.host_generator = torch.Generator().manual_seed(seed)
        self.image_perm = None
        self.last_batch = None
        if is_continue:
            name = latest_checkpoint(self.base_exp_dir)
            if name is not None:
                self.load_checkpoint(name)
        if self.image_perm is None:
            self.image_perm = self.get_image_perm()
        self.update_learning_rate()   # :439: before the first step, so step 0 runs at lr = 0 when warm_up_end > 0
        if self.mode[:5] == "train":
            self.file_backup()

    def networks(self) -> dict:
        return dict(zip(NETWORK_KEYS, (self.nerf_outside, self.sdf_network, self.deviation_network, self.color_network)))

    # ---- schedule -----------------------------------------------------------------------------------------------------------
    def get_image_perm(self):
        return torch.randperm(self.dataset.n_images, generator=self.host_generator)

    def get_cos_anneal_ratio(self) -> float:
        return cos_anneal_ratio(self.iter_step, self.anneal_end)

    def update_learning_rate(self) -> None:
        factor = learning_factor(self.iter_step, self.warm_up_end, self.end_iter, self.learning_rate_alpha)
        for g in self.optimizer.param_groups:
            g["lr"] = self.learning_rate * factor

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def file_backup(self) -> None:
        """Only the settings file is kept (the reference also copies its own sources)."""
        os.makedirs(os.path.join(self.base_exp_dir, "recording"), exist_ok=True)
        if self.conf_path is not None:
            shutil.copyfile(self.conf_path, os.path.join(self.base_exp_dir, "recording", "config.conf"))

    def save_checkpoint(self):
        """-> (checkpoint path, state path)."""
        ckpt = {CKPT_KEYS[k]: net.state_dict() for k, net in self.networks().items()}
        ckpt["optimizer"] = self.optimizer.state_dict()
        ckpt["iter_step"] = self.iter_step
        folder = os.path.join(self.base_exp_dir, "checkpoints")
        os.makedirs(folder, exist_ok=True)
        paths = os.path.join(folder, checkpoint_name(self.iter_step)), os.path.join(folder, state_name(self.iter_step))
        torch.save(ckpt, paths[0])
        torch.save({"generator": self.generator.get_state(), "host_generator": self.host_generator.get_state(),
                    "image_perm": self.image_perm, "iter_step": self.iter_step}, paths[1])
        return paths

    def load_checkpoint(self, checkpoint_name) -> None:
        folder = os.path.join(self.base_exp_dir, "checkpoints")
        ckpt = torch.load(os.path.join(folder, checkpoint_name), map_location=self.device, weights_only=True)
        for k, net in self.networks().items():
            net.load_state_dict(ckpt[CKPT_KEYS[k]])
        self.optimizer.load_state_dict(ckpt["optimizer"])
        self.iter_step = int(ckpt["iter_step"])
        self.renderer.invalidate()
        path = os.path.join(folder, state_name(self.iter_step))
        if os.path.isfile(path):   # absent beside a checkpoint of the reference: the generators then start from the seed
            st = torch.load(path, map_location="cpu", weights_only=True)
            self.generator.set_state(st["generator"])
            self.host_generator.set_state(st["host_generator"])
            self.image_perm = st["image_perm"]

    # ---- one step -----------------------------------------------------------------------------------------------------------
    def draw_batch(self):
        """The step's batch from the trainer's own generators -> (data [B, 10], near, far or None, view)."""
        view = int(self.image_perm[self.iter_step % len(self.image_perm)])
        if self.tail == "hip":
            data, near, far = self.dataset.gen_random_rays_with_bounds(view, self.batch_size, generator=self.generator)
            return data, near, far, view
        return self.host_batch(view), None, None, view

    def host_batch(self, view):
        """models/dataset.py:286-300 as the reference does it: pixels drawn and the float picture indexed on the host, one
        concatenation, one copy to the device."""
        ds = self.dataset
        if not hasattr(self, "_host_images"):
            self._host_images = ds.images_u8[..., :3].cpu().to(torch.float32) / 255.0
            self._host_masks = (torch.ones_like(self._host_images) if ds.masks_u8 is None
                                else ds.masks_u8.cpu().to(torch.float32) / 255.0)
        pixels_x = torch.randint(low=0, high=ds.W, size=[self.batch_size], generator=self.host_generator)
        pixels_y = torch.randint(low=0, high=ds.H, size=[self.batch_size], generator=self.host_generator)
        color = self._host_images[view][(pixels_y, pixels_x)]
        mask = self._host_masks[view][(pixels_y, pixels_x)]
        p = torch.stack([pixels_x, pixels_y, torch.ones_like(pixels_y)], dim=-1).float().to(self.device)
        p = torch.matmul(ds.intrinsics_all_inv[view, None, :3, :3], p[:, :, None]).squeeze(-1)
        rays_v = p / torch.linalg.norm(p, ord=2, dim=-1, keepdim=True)
        rays_v = torch.matmul(ds.pose_all[view, None, :3, :3], rays_v[:, :, None]).squeeze(-1)
        rays_o = ds.pose_all[view, None, :3, 3].expand(rays_v.shape)
        return torch.cat([rays_o.cpu(), rays_v.cpu(), color, mask[:, :1]], dim=-1).to(self.device)

    def render_batch(self, data, near=None, far=None):
        rays_o, rays_d = data[:, :3], data[:, 3:6]
        if near is None:
            near, far = self.dataset.near_far_from_sphere(rays_o, rays_d)
        return self.renderer.render(rays_o, rays_d, near, far, background_rgb=self.background_rgb,
                                    cos_anneal_ratio=self.get_cos_anneal_ratio(), generator=self.generator)

    def compute_losses(self, render_out, data):
        true_rgb, mask = data[:, 6:9], data[:, 9:10]
        if self.tail == "torch":
            return torch_losses(render_out, true_rgb, mask, self.igr_weight, self.mask_weight)
        return volume_losses(render_out["color_fine"], true_rgb, mask, render_out["weight_sum"], render_out["weight_max"],
                             render_out["cdf_fine"], render_out["gradient_error"], self.igr_weight, self.mask_weight)

    def step(self, batch=None):
        """One iteration of train() (:443-528).  batch [B, 10] replaces the draw.  -> the losses and statistics (detached device
        scalars) and the host values "lr" (the rate this step ran at) and "view" (None with a given batch)."""
        near = far = view = None
        if batch is None:
            batch, near, far, view = self.draw_batch()
        else:
            batch = _lib.require_cuda_f32(batch, "batch")
            if batch.dim() != 2 or batch.shape[1] != 10:
                raise _lib.IronError("VolumeTrainer.step: batch must be [B, 10], got %s" % (tuple(batch.shape),))
        self.last_batch = batch
        lr = self.optimizer.param_groups[0]["lr"]
        render_out = self.render_batch(batch, near, far)
        out = self.compute_losses(render_out, batch)
        self.optimizer.zero_grad(set_to_none=True)
        out["loss"].backward()
        self.optimizer.step()
        self.iter_step += 1
        self.update_learning_rate()
        if self.iter_step % len(self.image_perm) == 0:
            self.image_perm = self.get_image_perm()
        out = {k: v.detach() for k, v in out.items()}
        out["lr"], out["view"] = lr, view
        return out

    # ---- the loop -----------------------------------------------------------------------------------------------------------
    def train(self):
        """Steps iter_step .. end_iter - 1 with the reference's report line, checkpoints and validations (:437-528)."""
        out = None
        for _ in range(self.end_iter - self.iter_step):
            out = self.step()
            if self.report_freq and self.iter_step % self.report_freq == 0:
                print(self.base_exp_dir)
                print("iter:{:8>d} loss = {} lr={}".format(self.iter_step, float(out["loss"]), out["lr"]), flush=True)
            if self.save_freq and self.iter_step % self.save_freq == 0:
                self.save_checkpoint()
            if self.val_freq and self.iter_step % self.val_freq == 0:
                self.validate_image()
            if self.val_mesh_freq and self.iter_step % self.val_mesh_freq == 0:
                self.validate_mesh()
        return out

    def validate_image(self, idx=-1, resolution_level=-1):
        """render_volume.py:645-756 -> (path of the comparison picture, path of the normal picture)."""
        from .export_materials import _write_png
        ds, dev = self.dataset, self.device
        if idx < 0:
            idx = int(torch.randint(ds.n_images, (1,), generator=self.host_generator))
        print("Validate: iter: {}, camera: {}".format(self.iter_step, idx))
        if resolution_level < 0:
            resolution_level = self.validate_resolution_level
        rays_o, rays_d = ds.gen_rays_at(idx, resolution_level=resolution_level)
        H, W, _ = rays_o.shape
        rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
        n_samples = self.renderer.n_samples + self.renderer.n_importance
        rgb_frame = torch.empty((H * W, 3), dtype=torch.uint8, device=dev)
        normal_frame = torch.empty((H * W, 3), dtype=torch.uint8, device=dev)
        rot = torch.linalg.inv(ds.pose_all[idx, :3, :3]).contiguous()
        lib = _lib.load()
        with torch.no_grad(), torch.cuda.device(dev):
            for at in range(0, H * W, self.batch_size):
                o, d = rays_o[at:at + self.batch_size], rays_d[at:at + self.batch_size]
                near, far = ds.near_far_from_sphere(o, d)
                out = self.renderer.render(o, d, near, far, cos_anneal_ratio=self.get_cos_anneal_ratio(),
                                           background_rgb=self.background_rgb, generator=self.generator)
                color = _lib.require_cuda_f32(out["color_fine"], "color_fine")
                grads = _lib.require_cuda_f32(out["gradients"], "gradients")
                weights = _lib.require_cuda_f32(out["weights"], "weights")
                inside = _lib.require_cuda_f32(out["inside_sphere"], "inside_sphere")
                _lib.check(lib.iron_volume_frame_u8(color.data_ptr(), grads.data_ptr(), weights.data_ptr(), inside.data_ptr(),
                                                    rot.data_ptr(), color.shape[0], n_samples, weights.shape[1], at, H * W,
                                                    rgb_frame.data_ptr(), normal_frame.data_ptr(), _lib.stream_ptr(dev)))
                del out
        os.makedirs(os.path.join(self.base_exp_dir, "validations_fine"), exist_ok=True)
        os.makedirs(os.path.join(self.base_exp_dir, "normals"), exist_ok=True)
        name = "{:0>8d}_{}_{}.png".format(self.iter_step, 0, idx)
        img_path, normal_path = os.path.join(self.base_exp_dir, "validations_fine", name), os.path.join(self.base_exp_dir, "normals", name)
        imggt = ds.image_at(idx, resolution_level=resolution_level)
        _write_png(img_path, np.concatenate([rgb_frame.reshape(H, W, 3).cpu().numpy(), imggt], axis=0))
        _write_png(normal_path, normal_frame.reshape(H, W, 3).cpu().numpy())
        return img_path, normal_path

    def validate_mesh(self, world_space=False, resolution=64, threshold=0.0):
        """render_volume.py:788-800 with the marching cubes of csrc/mcubes.hip -> the path of meshes/{:0>8d}.ply."""
        from .export_materials import write_ply_mesh
        from .mesh import extract_geometry_gpu
        bound_min = torch.tensor(self.dataset.object_bbox_min, dtype=torch.float32)
        bound_max = torch.tensor(self.dataset.object_bbox_max, dtype=torch.float32)
        with torch.no_grad(), torch.cuda.device(self.device):
            vertices, triangles = extract_geometry_gpu(bound_min.to(self.device), bound_max.to(self.device), resolution, threshold,
                                                       lambda pts: -self.sdf_network.sdf(pts))
        vertices, triangles = vertices.cpu().numpy(), triangles.cpu().numpy()
        if world_space:
            vertices = vertices * self.dataset.scale_mats_np[0][0, 0] + self.dataset.scale_mats_np[0][:3, 3][None]
        os.makedirs(os.path.join(self.base_exp_dir, "meshes"), exist_ok=True)
        path = os.path.join(self.base_exp_dir, "meshes", "{:0>8d}.ply".format(self.iter_step))
        write_ply_mesh(path, vertices, triangles)
        return path


def config_parser():
    """render_volume.py:859-867's names and defaults for what is built, plus --seed, --optimizer and --tail."""
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--conf", type=str, default="./confs/base.conf")
    parser.add_argument("--mode", type=str, default="train", choices=("train", "validate_image", "validate_mesh"))
    parser.add_argument("--mcube_threshold", type=float, default=0.0)
    parser.add_argument("--is_continue", default=False, action="store_true")
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--case", type=str, default="")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--optimizer", type=str, default="fused", choices=("fused", "torch"))
    parser.add_argument("--tail", type=str, default="hip", choices=("hip", "torch"))
    return parser


def main(argv=None):
    a = config_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("iron_amd.train_volume needs a GPU (iron_amd has no CPU path)")
    if not os.path.isfile(a.conf):
        raise SystemExit("iron_amd.train_volume: no settings file %s" % a.conf)
    torch.cuda.set_device(a.gpu)
    trainer = VolumeTrainer(a.conf, mode=a.mode, case=a.case, is_continue=a.is_continue, seed=a.seed, optimizer=a.optimizer, tail=a.tail)
    if a.mode == "train":
        trainer.train()
    elif a.mode == "validate_image":
        print("written", *trainer.validate_image())
    else:
        print("written", trainer.validate_mesh(world_space=True, resolution=512, threshold=a.mcube_threshold))
    return trainer


if __name__ == "__main__":
    main()
