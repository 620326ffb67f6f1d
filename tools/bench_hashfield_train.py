"""One training step of the hash-grid SDF field, plain against fused (TCNNSDF.fused_training): the check configuration
(L 16, F 2, 2^19 entries, N 16, b 1.3819) behind a 64 x 2 ReLU head at n = 2^16, 2^18 and 2^20 uniform points.

    step     get_all(x), loss = mean sdf^2 + 0.1 mean (|grad| - 1)^2, loss.backward()  -- plain (autograd through nn.Linear, the
             encoding's two scatters) against fused (_FieldFn: iron_hashgrid_field_eval, iron_hashgrid_field_backward)
    split    of the fused step, each timed alone on the step's own adjoints: the forward (value and gradient), k_hg_field_bwd with
             the slot reduce (iron_hashgrid_field_backward without the table; the two kernels are not separated here), the pair scatter
    scatter  iron_hashgrid_backward_pair against iron_hashgrid_backward + iron_hashgrid_backward_backward on the step's ybar, e, v'

Times are hipEvent medians over --reps measurements per arm after --warmup, the arms of a comparison alternating inside one loop, with
the arm's 25 % and 75 % quantiles beside them.  Launches per step are counted by the profiler in a step of their own (kernels and
memsets on the device); "not measured" where it is unavailable.  Before timing, the two paths' gradients are compared (rel-L2 per
tensor) twice: on the loss as it is, and with the points left out of the loss that have a hidden pre-activation within 1e-5 of its
sum of term magnitudes of zero (the plain forward's; a ReLU mask there may differ between two fp32 forwards).  Prints one JSON line.

    python tools/bench_hashfield_train.py [--reps 20] [--warmup 3] [--ns 65536,262144,1048576]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from iron_amd import hashgrid, tcnn_fields  # noqa: E402

CHECK = dict(otype="HashGrid", n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.3819)
HEAD = dict(otype="FullyFusedMLP", activation="ReLU", output_activation="None", n_neurons=64, n_hidden_layers=2)


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(arms, reps, warmup):
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(one(fn))
    out = {}
    for k, v in ms.items():
        v.sort()
        q = lambda f: round(v[min(len(v) - 1, int(f * len(v)))], 4)  # noqa: E731
        out[k] = {"median": q(0.5), "q25": q(0.25), "q75": q(0.75)}
    return out


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n if n > 0 else "not measured"
    except Exception:
        return "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns", default="65536,262144,1048576")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "field.json")
        with open(path, "w") as f:
            json.dump({"encoding": CHECK, "network": HEAD}, f)
        torch.manual_seed(0)
        field = tcnn_fields.TCNNSDF(path).to(dev)
    with torch.no_grad():
        field.sdf_encoding.params.uniform_(-0.1, 0.1)
    enc = field.sdf_encoding
    g = torch.Generator().manual_seed(0)
    out = {"encoding": CHECK, "network": HEAD, "runs": []}

    def step(x, fused, keep=None):
        field.fused_training = fused
        for p in field.parameters():
            p.grad = None
        sdf, _, grad = field.get_all(x, is_training=True)
        terms = sdf[:, 0] ** 2 + 0.1 * (grad.norm(dim=-1) - 1.0) ** 2
        loss = terms.mean() if keep is None else (terms * keep).mean()
        loss.backward()
        return sdf, grad

    def away_from_kinks(x):
        """1.0 where every hidden pre-activation of the plain forward is farther from zero than 1e-5 of |W| |h|"""
        with torch.no_grad():
            h = enc(x)
            keep = torch.ones(x.shape[0], device=x.device)
            lin = [m for m in field.sdf_network if isinstance(m, torch.nn.Linear)]
            for m in lin[:-1]:
                z = h @ m.weight.T
                keep = keep * ((z.abs() > 1e-5 * (h.abs() @ m.weight.abs().T)).all(dim=1)).float()
                h = torch.relu(z)
        return keep

    for n in [int(v) for v in a.ns.split(",")]:
        x = torch.rand(n, 3, generator=g).to(dev)
        step(x.clone(), False)
        plain = [p.grad.clone() for p in field.parameters()]
        sdf, grad = step(x.clone(), True)
        fused = [p.grad.clone() for p in field.parameters()]
        gap = [float((u.double() - v.double()).norm() / v.double().norm()) for u, v in zip(fused, plain)]
        keep = away_from_kinks(x)
        step(x.clone(), False, keep)
        plain_k = [p.grad.clone() for p in field.parameters()]
        step(x.clone(), True, keep)
        gap_k = [float((p.grad.double() - v.double()).norm() / v.double().norm()) for p, v in zip(field.parameters(), plain_k)]
        run = {"n": n, "gradient_rel_l2_fused_vs_plain": gap, "points_left_out_near_kinks": int(n - keep.sum().item()),
               "gradient_rel_l2_away_from_kinks": gap_k,
               "step_ms": alternating({"plain": lambda: step(x.clone(), False), "fused": lambda: step(x.clone(), True)}, a.reps, a.warmup),
               "launches": {"plain": launches(lambda: step(x.clone(), False)), "fused": launches(lambda: step(x.clone(), True))}}
        run["fused_over_plain"] = round(run["step_ms"]["fused"]["median"] / run["step_ms"]["plain"]["median"], 3)
        # the fused step's parts on its own adjoints
        with torch.no_grad():
            d_sdf = (2.0 / n) * sdf.detach()
            nrm = grad.detach().norm(dim=-1, keepdim=True)
            d_g = (0.2 / n) * (nrm - 1.0) * grad.detach() / nrm
            desc = field._train_desc()
            pk, tpk, table = field._fused_packed(desc, dev), field._train_packed(desc, dev), enc.params.detach()
            _, _, ybar, e = tcnn_fields.field_backward(desc, x, table, pk, tpk, d_sdf, d_g, want_table=False, want_rows=True)
            parts = alternating({
                "forward": lambda: field.eval_fused(x, gradient=True),
                "field_bwd_and_slot_reduce": lambda: tcnn_fields.field_backward(desc, x, table, pk, tpk, d_sdf, d_g, want_table=False),
                "pair_scatter": lambda: hashgrid.backward_pair(enc.desc, enc.n_params, x, table, ybar, e, d_g),
                "backward_whole": lambda: tcnn_fields.field_backward(desc, x, table, pk, tpk, d_sdf, d_g),
            }, a.reps, a.warmup)

            def two():
                hashgrid.backward(enc.desc, enc.n_params, x, table, ybar, want_x=False)
                hashgrid.backward_backward(enc.desc, enc.n_params, x, table, e, d_g, want_dy=False)

            run["fused_parts_ms"] = parts
            run["scatter_ms"] = alternating({"two": two, "pair": lambda: hashgrid.backward_pair(enc.desc, enc.n_params, x, table, ybar, e, d_g)},
                                            a.reps, a.warmup)
        out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
