"""CPU emulation of the screen's adaptive march (csrc/trace.hip k_sampler_screen).

The screened sampler does not evaluate samples that an evaluated neighbour proves positive: a sample e with screened value f1(e)
certifies the skipped samples m positions away while f1(e) > delta + L * dz * m, where dz is the ray's sample spacing and
L = K_STRIDE * G, G = max |grad f| over the screen's calibration points (central differences at CALIB_H, as k_screen_calib takes
them).  This emulation marches the rays of tools/screen_margin.py's scenes the way the kernel does -- blocks of 8 samples at a
stride of 1 .. STRIDE_MAX, a gap certified from either end, a restart at stride 1 behind the last good sample when a sample of a
strided block is not certainly positive or a gap is not certified -- on the emulated screen's values, and reports

  * the lane evaluations (passes x 8: idle lanes are charged) against the stride-1 march's;
  * the smallest EXACT value of a sample that was skipped, and how many skipped samples are <= 0 (must be none);
  * the slope guard's ratio as the kernel records it (adjacent samples of stride-1 blocks, delta / 2 allowed for the screen's own
    error, relative to L), and the same from exact values without the allowance.

A ray's march ends at its first sample with a negative exact value (the kernel marches a pending ray on at stride 1 to its first
certainly-negative sample; march() does not model those passes).  march_rays() / pending_report() do: they march every ray to its
first certainly-negative screened sample the way the kernel does, with pending rays striding like the others, and report that the
samples the stride-1 code classifies as uncertain or negative are those of the all-stride-1 march, what the stride saves on pending
rays, and the slope guard's ratio and number of observations from each of its three sources (the stride-1 passes, the resolve's
exact value against the screened predecessor, the exact values of adjacent listed samples).  L is empirical, not a
certified bound; tests/test_sampler_stride_margin.py and tests/test_sampler_stride_pending.py pin the figures.

How a good block is followed up is a parameter of both marches (`rule`, see RULES: the kernel's two-sided choice by default, the
one-sided choice it replaced, and the variants that were emulated and not built); stride_report() / pending_report() give passes and
restarts under each, tests/test_sampler_stride_two_sided.py holds the two-sided rule to the one-sided one.

    python3 tools/sampler_stride_margin.py [--res 200] [--scenes S0,S1,S3] [--gen 2] [--stride-max 16] [--l-scale 1.0]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_margin as SM  # noqa: E402
from oracle import iron_ref as R  # noqa: E402

# the constants of csrc/trace.hip (kStrideK, kStrideGuard, kStrideCalibH, kStrideMax, kSamplerBlock)
K_STRIDE = 2.0
GUARD = 0.75
CALIB_H = 1.0 / 128.0
STRIDE_MAX = 16
BLOCK = SM.BLOCK


@torch.no_grad()
def grad_max(sd, spec):
    """G of k_screen_calib: the largest central-difference gradient norm of the exact value over the calibration points."""
    x = SM.calibration_points()
    g = []
    for ax in range(3):
        e = torch.zeros(3)
        e[ax] = CALIB_H
        g.append((R.sdf_forward(sd, spec, x + e)[:, 0] - R.sdf_forward(sd, spec, x - e)[:, 0]) * (0.5 / CALIB_H))
    gn = torch.stack(g, -1).norm(dim=-1)
    return float(gn.max()) if bool(torch.isfinite(gn).all()) else float("inf")


@torch.no_grad()
def ray_samples(sd, spec, res, prm=R.TracerParams()):
    """Every sample of the rays the sampler marches on a res x res view of the fixture camera: exact values, screened values [rays, n_steps],
    the sample spacing along each ray and the width of its range."""
    from iron_amd import scenes
    K, W2C = scenes.fixture_camera_matrices(res, res)
    cam = R.CameraSpec(res, res, K.cpu(), W2C.cpu())
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    hit, near, far = R.intersect_sphere(ro, rd, 1.0)
    f = lambda p: R.sdf_forward(sd, spec, p)[:, 0]
    _, unf, _, s, t = R.sphere_tracing(f, ro, rd, near, far, hit, prm)
    o, d = ro[unf], rd[unf]
    pos = s[unf] > 0
    smin = torch.where(pos, t[unf], near[unf])
    smax = torch.where(pos, far[unf], t[unf])
    n = prm.n_steps
    lin = torch.linspace(0, 1, steps=n).float()
    width = smax - smin
    z = smin[:, None] + lin[None, :] * width[:, None]
    p = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    fe = torch.cat([f(c) for c in p.split(200000)]).reshape(-1, n)
    f1 = torch.cat([SM.screen_forward(sd, spec, c) for c in p.split(200000)]).reshape(-1, n)
    dz = width.abs() * float(lin[1] - lin[0]) * d.norm(dim=-1)
    return fe, f1, dz, width


def _reach(v, delta, ld, smax):
    c = 0
    for m in range(1, smax):
        if v > delta + ld * m:
            c += 1
    return c


# How a good block is followed up (k_sampler_screen).  The next block's first sample sits 1 + reach(e_7) behind e_7
# under every rule: that gap has only e_7 to vouch for it.  The rules differ in the stride inside the next block, whose gaps have an
# evaluated sample at each end:
#   one_sided       1 + reach(e_7), the first gap's size (the kernel before the two-sided choice; iron_sampler_screen_debug(6, 1));
#   two_sided_any   min(smax, 1 + 2 * reach(e_7)) when f1(e_7) >= f1(e_6) -- behind a grazing ray's closest approach the values rise,
#                   so each end of a gap certifies at least what e_7 did -- and the first gap's size otherwise;
#   two_sided       the same, but the rise must be a slope worth the name: f1(e_7) - f1(e_6) >= RISE * L * (distance e_6 .. e_7).  A
#                   flat tail (a bumpy field at a local maximum) is no evidence that the values go on rising (the kernel's rule);
#   two_sided_calm  two_sided_any, but one_sided for the block that follows a restart's stride-1 block (a gate that was tried, not built).
# Whatever is chosen is certified after the evaluation, gap by gap, or the block is discarded: the rule decides passes, never results.
RULES = ("one_sided", "two_sided", "two_sided_any", "two_sided_calm")
RULE = "two_sided"
RISE = 1.0 / 12.0   # kStrideRise of csrc/trace.hip


def _follow_up(rule, reach_last, rise, ld_block, smax, after_restart=False):
    """(first gap, stride inside the block) behind a block whose last sample certifies reach_last skipped samples and stands `rise`
    above the sample before it; ld_block = L * the distance between the two."""
    if rule not in RULES:
        raise ValueError("stride rule %r: one of %s" % (rule, ", ".join(RULES)))
    gap = 1 + reach_last
    rising = rise >= RISE * ld_block if rule == "two_sided" else rise >= 0.0
    if rule == "one_sided" or not rising or (rule == "two_sided_calm" and after_restart):
        return gap, gap
    return gap, min(smax, 1 + 2 * reach_last)


def march(fe, f1, dz, width, delta, L, smax=STRIDE_MAX, rule=RULE):
    """The adaptive march over every ray.  Returns passes, strided passes, the stride-1 march's passes, the smallest exact value of a
    skipped sample, the skipped samples <= 0, and the guard ratio from screened (with allowance) and exact values."""
    n_rays, n = fe.shape
    fe_l, f1_l = fe.tolist(), f1.tolist()
    dz_l, w_l = dz.tolist(), width.tolist()
    passes = strided = base = nonpos = restarts = 0
    worst = math.inf
    guard1 = guard_ex = 0.0
    for r in range(n_rays):
        a, b = f1_l[r], fe_l[r]
        ld = L * dz_l[r]
        if not (w_l[r] > 0.0 and 0.0 < ld < math.inf):
            ld = 0.0
        first = next((i for i in range(n) if b[i] < 0), n)
        base += min(first // BLOCK + 1, (n + BLOCK - 1) // BLOCK)
        seen = [False] * n
        pos, s, pend, prev, calm = 0, 1, False, -1, False
        while pos < n:
            idx = [pos + s * k for k in range(BLOCK) if pos + s * k < n]
            passes += 1
            strided += s > 1
            for e in idx:
                seen[e] = True
            reach = [_reach(a[e], delta, ld, smax) if ld > 0.0 else 0 for e in idx]
            if s > 1:
                last_good = None
                for k, e in enumerate(idx):
                    if not a[e] > delta:
                        last_good = k - 1
                        break
                    if k < BLOCK - 1:
                        gap = min(s - 1, n - 1 - e)
                        if reach[k] + (reach[k + 1] if k + 1 < len(idx) else 0) < gap:
                            last_good = k
                            break
                if last_good is not None:   # the rest of the block is discarded
                    for e in idx[last_good + 1:]:
                        seen[e] = False
                    restarts += 1
                    if last_good < 0:   # as the kernel: the previous sample is 1 + reach(its value) in front of pos
                        pos = pos - _reach(a[prev], delta, ld, smax)
                        assert pos == prev + 1, (r, pos, prev)
                    else:
                        prev = idx[last_good]
                        pos = prev + 1
                    s, calm = 1, True
                    continue
            else:
                ended, watch = False, True
                for k, e in enumerate(idx):
                    if k > 0 and watch and ld > 0.0:   # the slope guard: pairs up to the block's first sample that is not certainly positive
                        guard1 = max(guard1, max(abs(a[e] - a[e - 1]) - 0.5 * delta, 0.0) / ld)
                        guard_ex = max(guard_ex, abs(b[e] - b[e - 1]) / ld)
                    if b[e] < 0:
                        ended = True
                        break
                    if not a[e] > delta:   # listed for the resolve: the ray is pending and stays at stride 1
                        pend, watch = True, False
                if ended:
                    break
            if len(idx) < BLOCK:
                break
            last = prev = idx[-1]
            sb, gap, s = s, 1, 1
            if ld > 0.0 and not pend and a[last] > delta:
                gap, s = _follow_up(rule, reach[-1], a[last] - a[idx[-2]], ld * sb, smax, calm)
            calm = False
            pos = last + gap
        for i in range(first):
            if not seen[i]:
                v = b[i]
                worst = min(worst, v)
                nonpos += not v > 0
    return {"passes": passes, "strided_passes": strided, "restarts": restarts, "baseline_passes": base, "min_exact_skipped": worst,
            "skipped_nonpositive": nonpos, "guard": guard1, "guard_exact": guard_ex}


def march_rays(fe, f1, dz, width, delta, L, smax=STRIDE_MAX, pending_stride=True, rule=RULE):
    """The march of k_sampler_screen ray by ray, to each ray's first certainly-negative screened sample or its end, pending rays
    (those that have listed an uncertain sample) included: with `pending_stride` they stride by the rules of the others, without
    it they keep stride 1 (the march before they strode); L = 0 is the all-stride-1 march.  Returns the pass counts, per ray what
    the stride-1 code classified (the listed uncertain samples and the first certainly-negative one), and the slope guard's three
    sources as the kernels take them, each with its number of observations:
      march    adjacent screened samples of stride-1 passes up to the first that is not certainly positive, delta / 2 allowed;
      resolve  the exact value of a listed sample against the screened value of its predecessor, delta / 2 allowed;
      pair     the exact values of two adjacent samples listed by one pass, no allowance.
    `rule` is how a good block is followed up (RULES).  Progress is counted as the kernel's termination needs it: a pass that is not a
    restart must end the ray or leave pos behind where it was; a restart must leave pos one sample behind an evaluated good sample
    (the one the pass accepted last, or the ray's previous one: `restarts_first`, the case last_good < 0) at stride 1, where the
    next pass cannot restart.  `stalls` counts the passes that did neither (must be none)."""
    n_rays, n = fe.shape
    fe_l, f1_l = fe.tolist(), f1.tolist()
    dz_l, w_l = dz.tolist(), width.tolist()
    c = {"passes": 0, "strided_passes": 0, "restarts": 0, "restarts_first": 0, "stalls": 0, "stride1_behind": 0, "stride1_fresh": 0,
         "obs_march": 0, "obs_resolve": 0, "obs_pair": 0, "guard_march": 0.0, "guard_resolve": 0.0, "guard_pair": 0.0, "pending_rays": 0}
    classified = []
    for r in range(n_rays):
        a, b = f1_l[r], fe_l[r]
        ld = L * dz_l[r]
        if not (w_l[r] > 0.0 and 0.0 < ld < math.inf):
            ld = 0.0
        listed, first_neg = [], n
        pos, s, pend, prev, calm = 0, 1, False, -1, False   # prev: the ray's last accepted sample
        while pos < n:
            idx = [pos + s * k for k in range(BLOCK) if pos + s * k < n]
            c["passes"] += 1
            c["stalls"] += not pos > prev
            reach = [_reach(a[e], delta, ld, smax) if ld > 0.0 else 0 for e in idx]
            if s > 1:
                c["strided_passes"] += 1
                last_good = None
                for k, e in enumerate(idx):
                    if not a[e] > delta:
                        last_good = k - 1
                        break
                    if k < BLOCK - 1:
                        gap = min(s - 1, n - 1 - e)
                        if reach[k] + (reach[k + 1] if k + 1 < len(idx) else 0) < gap:
                            last_good = k
                            break
                if last_good is not None:   # the rest of the block is discarded
                    c["restarts"] += 1
                    if last_good < 0:   # as the kernel: the previous sample is 1 + reach(its value) in front of pos, whatever s is
                        c["restarts_first"] += 1
                        pos = pos - _reach(a[prev], delta, ld, smax)
                    else:
                        prev = idx[last_good]
                        pos = prev + 1
                    c["stalls"] += pos != prev + 1 or not a[prev] > delta
                    s, calm = 1, True
                    continue
            else:
                ngood = [k for k, e in enumerate(idx) if not a[e] > delta]
                if pend and not ngood:
                    c["stride1_behind"] += 1
                if not pend:
                    c["stride1_fresh"] += 1
                if ld > 0.0:
                    for k in range(1, len(idx)):
                        if ngood and k > ngood[0]:
                            break
                        c["obs_march"] += 1
                        c["guard_march"] = max(c["guard_march"], max(abs(a[idx[k]] - a[idx[k] - 1]) - 0.5 * delta, 0.0) / ld)
                neg = next((k for k, e in enumerate(idx) if a[e] < -delta), None)
                unc = [e for e in idx[:neg] if not a[e] > delta and not a[e] < -delta]
                for j, e in enumerate(unc):
                    if ld > 0.0 and e > 0:
                        c["obs_resolve"] += 1
                        c["guard_resolve"] = max(c["guard_resolve"], max(abs(b[e] - a[e - 1]) - 0.5 * delta, 0.0) / ld)
                    if ld > 0.0 and j > 0 and unc[j - 1] == e - 1:
                        c["obs_pair"] += 1
                        c["guard_pair"] = max(c["guard_pair"], abs(b[e] - b[e - 1]) / ld)
                listed += unc
                pend = pend or bool(unc)
                if neg is not None:
                    first_neg = idx[neg]
                    break
            last = pos + s * (BLOCK - 1)
            sb, gap, s = s, 1, 1
            if ld > 0.0 and (pending_stride or not pend) and last < n and a[last] > delta:
                gap, s = _follow_up(rule, reach[-1], a[last] - a[last - sb], ld * sb, smax, calm)
            c["stalls"] += not last + gap > pos
            calm = False
            prev, pos = idx[-1], last + gap
        c["pending_rays"] += pend
        classified.append((tuple(listed), first_neg))
    c["classified"] = classified
    return c


@torch.no_grad()
def pending_report(sd, spec, res, smax=STRIDE_MAX, l_scale=1.0, samples=None):
    """Pending rays striding (march_rays) against the march that kept them on stride 1 and against the all-stride-1 march: the pass
    counts of the three, the rays whose stride-1 classification (listed samples, first certainly-negative sample) differs from the
    all-stride-1 march's (must be none), and the guard's ratio and observation count per source, before and after."""
    delta = SM.delta_of(sd, spec)
    L = K_STRIDE * grad_max(sd, spec) * l_scale
    if not (0.0 < L < math.inf):
        L = 0.0
    fe, f1, dz, width = samples if samples is not None else ray_samples(sd, spec, res)
    one = march_rays(fe, f1, dz, width, delta, 0.0, smax)
    old = march_rays(fe, f1, dz, width, delta, L, smax, pending_stride=False)
    new = march_rays(fe, f1, dz, width, delta, L, smax, pending_stride=True)
    out = {"sampled_rays": int(fe.shape[0]), "pending_rays": new["pending_rays"], "passes_stride1": one["passes"],
           "class_mismatch_rays": sum(x != y for x, y in zip(new["classified"], one["classified"])),
           "class_mismatch_rays_before": sum(x != y for x, y in zip(old["classified"], one["classified"])),
           "listed_samples": sum(len(x[0]) for x in one["classified"])}
    for tag, m in (("before", old), ("after", new)):
        for k, v in m.items():
            if k not in ("classified", "pending_rays"):
                out["%s_%s" % (k, tag)] = v
    # how a good block is followed up: the kernel's rule ("after" above) against the others
    for rule in RULES:
        m = new if rule == RULE else march_rays(fe, f1, dz, width, delta, L, smax, rule=rule)
        out["rule_" + rule] = {"passes": m["passes"], "strided_passes": m["strided_passes"], "restarts": m["restarts"],
                               "restarts_first": m["restarts_first"], "stalls": m["stalls"],
                               "class_mismatch_rays": sum(x != y for x, y in zip(m["classified"], one["classified"]))}
    return out


@torch.no_grad()
def stride_report(sd, spec, res, smax=STRIDE_MAX, l_scale=1.0, samples=None):
    """The figures of the module docstring for one network; `samples` = ray_samples(sd, spec, res) when the caller has them."""
    delta = SM.delta_of(sd, spec)
    G = grad_max(sd, spec)
    L = K_STRIDE * G * l_scale
    fe, f1, dz, width = samples if samples is not None else ray_samples(sd, spec, res)
    out = {"sampled_rays": int(fe.shape[0]), "no_root": int((~(fe < 0).any(1)).sum()), "delta": delta, "G": G, "L": L,
           "dz_min": float(dz.min()), "dz_median": float(dz.median())}
    if not (0.0 < L < math.inf):
        L = 0.0   # the kernel's rule: stride 1
    m = march(fe, f1, dz, width, delta, L, smax)
    out.update(m)
    for rule in RULES:
        o = m if rule == RULE else march(fe, f1, dz, width, delta, L, smax, rule)
        out["rule_" + rule] = {k: o[k] for k in ("passes", "strided_passes", "restarts", "skipped_nonpositive")}
    out["lane_evals"] = m["passes"] * BLOCK
    out["baseline_lane_evals"] = m["baseline_passes"] * BLOCK
    out["ratio"] = m["passes"] / max(m["baseline_passes"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--scenes", default="S0,S1,S3")
    ap.add_argument("--gen", type=int, default=2, help="generalised 8 x 256 nets (tests/_nets.py), seeds 0..gen-1")
    ap.add_argument("--stride-max", type=int, default=STRIDE_MAX)
    ap.add_argument("--l-scale", type=float, default=1.0, help="scale the slope bound (0.1: what trips the guard)")
    a = ap.parse_args()
    nets = [(s, SM.scene_net(s)) for s in a.scenes.split(",") if s] + [("gen%d" % g, SM.generalised_net(g)) for g in range(a.gen)]
    for name, (sd, spec) in nets:
        samples = ray_samples(sd, spec, a.res)
        print(name, json.dumps(stride_report(sd, spec, a.res, a.stride_max, a.l_scale, samples)), flush=True)
        print(name, "pending", json.dumps(pending_report(sd, spec, a.res, a.stride_max, a.l_scale, samples)), flush=True)


if __name__ == "__main__":
    main()
