"""One stage-1 training step of iron_amd.train_volume.VolumeTrainer at the shapes of confs/womask_iron.conf (512 rays x (64 + 4 x 16
+ 32 outside) samples, perturb = 1, seeded random-init networks, one seeded random 128 x 128 view), split into batch / render / loss /
backward / optimiser, with the launches of each phase counted by torch.profiler -- for the trainer as shipped (device batch, HIP
loss, FusedAdam) and for the same loop with --tail torch --optimizer torch: the reference's host batch, its loss as torch
expressions and torch.optim.Adam, which is how tools/neus_train_step.py arranges the parent commit's pieces.
    python tools/bench_train_volume.py [--batch 512] [--steps 10] [--size 128]
Prints one JSON line.  No threshold is asserted anywhere: DESIGN.md §22 reports what comes out."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("batch", "render", "loss", "backward", "optimiser")
CONF = """
general { base_exp_dir = ./exp_bench_train_volume/ }
train {
    learning_rate = 5e-4
    learning_rate_alpha = 0.05
    end_iter = 100001
    batch_size = %d
    validate_resolution_level = 4
    warm_up_end = 5000
    anneal_end = 50000
    use_white_bkgd = False
    save_freq = 10000
    val_freq = 500
    val_mesh_freq = 5000
    report_freq = 100
    igr_weight = 0.1
    mask_weight = 0.0
}
model {
    nerf { D = 8, d_in = 4, d_in_view = 3, W = 256, multires = 10, multires_view = 4, output_ch = 4, skips=[4], use_viewdirs=True }
    sdf_network { d_out = 257, d_in = 3, d_hidden = 256, n_layers = 8, skip_in = [4], multires = 6, bias = 0.5, scale = 1.0,
                  geometric_init = True, weight_norm = True }
    variance_network { init_val = 0.3 }
    rendering_network { d_feature = 256, mode = idr, d_in = 9, d_out = 3, d_hidden = 256, n_layers = 8, skip_in = [4],
                        weight_norm = True, multires = 10, multires_view = 4, squeeze_out = True }
    neus_renderer { n_samples = 64, n_importance = 64, n_outside = 32, up_sample_steps = 4, perturb = 1.0 }
}
"""


def _phases(tr):
    """One step of VolumeTrainer.step(), cut where the phases meet: a list of callables run in order."""
    s = {}

    def batch():
        s["data"], s["near"], s["far"], s["view"] = tr.draw_batch()

    def render():
        s["render_out"] = tr.render_batch(s["data"], s["near"], s["far"])

    def loss():
        s["out"] = tr.compute_losses(s["render_out"], s["data"])

    def backward():
        tr.optimizer.zero_grad(set_to_none=True)
        s["out"]["loss"].backward()

    def optimiser():
        tr.optimizer.step()
        tr.iter_step += 1
        tr.update_learning_rate()

    return [batch, render, loss, backward, optimiser], s


def _launches(fn):
    """(kernel launches, memcpy / memset operations) of fn() as torch.profiler sees them on the device."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels, copies = 0, 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Optimizer."):
            if e.name.lower().startswith(("memcpy", "memset")) or "copybuffer" in e.name.lower() or "fillbuffer" in e.name.lower():
                copies += 1
            else:
                kernels += 1
    return kernels, copies


def run_one(batch, steps, size, optimizer, tail, warmup=3):
    from iron_amd import scenes
    from iron_amd.dataset import VolumeDataset
    from iron_amd.train_volume import VolumeTrainer
    dev = torch.device("cuda", 0)
    K, W2C = scenes.fixture_camera_matrices(size, size)
    images = torch.randint(0, 256, (1, size, size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(0)
    tr = VolumeTrainer(CONF % batch, mode="bench", dataset=VolumeDataset(images=images, Ks=K[None], W2Cs=W2C[None], device=dev),
                       optimizer=optimizer, tail=tail, seed=0)
    tr.iter_step = 5000   # past the warm-up: every step moves the parameters
    tr.update_learning_rate()
    times = []
    for step in range(warmup + steps):
        fns, state = _phases(tr)
        t = []
        for fn in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        if step >= warmup:
            times.append(t)
    fns, state = _phases(tr)
    counts = [_launches(fn) for fn in fns]
    n = len(PHASES)
    ms = [sum(t[i] for t in times) / len(times) for i in range(n)]
    best = [min(t[i] for t in times) for i in range(n)]
    return {"optimizer": optimizer, "tail": tail,
            "ms": dict(zip(PHASES, (round(v, 3) for v in ms)), step=round(sum(ms), 3)),
            "ms_min": dict(zip(PHASES, (round(v, 3) for v in best)), step=round(sum(best), 3)),
            "kernel_launches": dict(zip(PHASES, (c[0] for c in counts)), step=sum(c[0] for c in counts)),
            "copies_and_fills": dict(zip(PHASES, (c[1] for c in counts)), step=sum(c[1] for c in counts)),
            "loss": float(state["out"]["loss"].detach()), "n_tensors": sum(len(g["params"]) for g in tr.optimizer.param_groups)}


def run(batch=512, steps=10, size=128):
    return {"config": "stage-1 step, %d rays x (64 + 4x16 + 32 outside) samples, perturb = 1, one %dx%d view" % (batch, size, size),
            "steps": steps, "fused": run_one(batch, steps, size, "fused", "hip"), "baseline": run_one(batch, steps, size, "torch", "torch")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    print(json.dumps(run(a.batch, a.steps, a.size)))


if __name__ == "__main__":
    main()
