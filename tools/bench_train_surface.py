"""One stage-2 training step of iron_amd.train_surface.SurfaceTrainer on config C3's scene (S1, 512 x 512, one view, edge sampling
on, a seeded random target as tools/train_step.py uses), split into render / losses / backward / optimiser, with the launches of
each phase counted by torch.profiler -- for the trainer as shipped (HIP regularisers + FusedAdam) and for the same loop on the
pieces of the parent commit as tools/train_step.py arranges them (the regularisers as torch expressions, torch.optim.Adam).
    python tools/bench_train_surface.py [--size 512] [--steps 5] [--no-edges]
Prints one JSON line.  No threshold is asserted anywhere: DESIGN.md §21 reports what comes out."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("render", "losses", "backward", "optimiser")


def _phases(tr):
    """One step of SurfaceTrainer.step(), cut where the phases meet: a list of callables run in order."""
    s = {}

    def render():
        tr.optimizer.zero_grad(set_to_none=True)
        s["idx"], s["origin"], s["eik_points"] = tr.draw()
        s["results"] = tr.render_patch(s["idx"], s["origin"])

    def losses():
        eik_grad = tr.sdf_network.gradient(s["eik_points"]).view(-1, 3)
        s["out"] = tr.compute_losses(s["results"], tr.gt_patch(s["idx"], s["origin"]), eik_grad)

    def backward():
        s["out"]["loss"].backward()

    def optimiser():
        tr.optimizer.step()
        tr.global_step += 1

    return [render, losses, backward, optimiser], s


def _launches(fn):
    """(kernel launches, memcpy / memset operations, {kernel name: launches}) of fn() as torch.profiler sees them on the device."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels, copies, names = 0, 0, {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Optimizer."):   # (not the step's annotation range)
            if e.name.lower().startswith(("memcpy", "memset")) or "copybuffer" in e.name.lower() or "fillbuffer" in e.name.lower():
                copies += 1
            else:
                kernels += 1
                short = e.name[:60]
                names[short] = names.get(short, 0) + 1
    return kernels, copies, names


def run_one(size, steps, no_edges, optimizer, regularisers, warmup=2):
    from iron_amd import scenes
    from iron_amd.train_surface import SurfaceTrainer
    dev = torch.device("cuda", 0)
    nets = scenes.build_networks("S1")
    K, W2C = scenes.fixture_camera_matrices(size, size)
    target = torch.rand(1, size, size, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    tr = SurfaceTrainer(images=target, Ks=K[None], W2Cs=W2C[None], renderer_name="ggx", patch_size=size, no_edgesample=no_edges,
                        networks=nets, optimizer=optimizer, regularisers=regularisers, seed=0)
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
    ms = [sum(t[i] for t in times) / len(times) for i in range(4)]
    return {"optimizer": optimizer, "regularisers": regularisers,
            "ms": dict(zip(PHASES, (round(v, 3) for v in ms)), step=round(sum(ms), 3)),
            "kernel_launches": dict(zip(PHASES, (c[0] for c in counts)), step=sum(c[0] for c in counts)),
            "copies_and_fills": dict(zip(PHASES, (c[1] for c in counts)), step=sum(c[1] for c in counts)),
            "optimiser_kernels": counts[3][2],
            "n_mask": int(state["out"]["n_mask"]), "loss": float(state["out"]["loss"].detach()),
            "n_tensors": sum(len(g["params"]) for g in tr.optimizer.param_groups)}


def run(size=512, steps=5, no_edges=False):
    return {"config": "C3 scene: S1 %dx%d, one view, %s, %d eikonal points" % (size, size, "no edge sampling" if no_edges else "edge sampling",
                                                                                size * size // 2),
            "steps": steps,
            "fused": run_one(size, steps, no_edges, "fused", "hip"),
            "baseline": run_one(size, steps, no_edges, "torch", "torch")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-edges", action="store_true")
    a = ap.parse_args()
    print(json.dumps(run(a.size, a.steps, a.no_edges)))


if __name__ == "__main__":
    main()
