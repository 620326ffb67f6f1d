"""SDF fields on which the tracer's rarely taken paths are common, and the oracle's side of a stage-by-stage comparison on them.
Shared by tests/test_hard_fields_oracle.py (CPU) and tests/test_gpu_trace_hard_fields.py.

S0 and S1 are near-spheres: of the 491 rays of a 56 x 56 view of S1 that sphere tracing leaves unfinished exactly one has overshot
(sdf < 0), so raytracer.py:59-65's choice of the sampler range [min_dis, acc_dis] instead of [acc_dis, max_dis] is all but
never compared with the reference.  The fields below need no fitting and no fixture, they fall out of seeds:

  bumpy(sigma, seed)   S0's network, lin0.weight_v[:, 3:] += sigma * randn(seed) (S1's recipe is sigma = 0.01 without the
                       re-centring), then _nets._recentre
  gen(i)               the generalised production net of tests/test_gpu_sampler_stride.py: generalise(prod, 1000 + i)

They have hundreds of overshoot rays, rays with three and more sign changes along the sampler's 128 samples (the first bracket must
be taken) and, the gen fields, rays whose first sample is already negative (no root) and reversed sampler ranges (s_max < s_min).

Everything here runs the oracle (oracle/iron_ref.py) on the CPU in fp64 on fp32 inputs: the inputs of every stage are fp32 tensors
that the GPU test hands to the kernels unchanged, so both sides of a stage comparison start from identical numbers.  The tolerance
`tau` of a field comes from the reference alone (its fp32 run against its fp64 run), never from the GPU.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

from oracle import iron_ref as R
from iron_amd import scenes

import _nets as N

RES = 56                 # the comparison view: RES x RES rays of the fixture camera
N_STEPS = 128
CHUNK = 1000             # max_num_rays of the whole-tracer comparison: several bisection chunks

# name -> (builder, arguments, camera yaw in degrees)
FIELDS = {
    "bumpy02_s1": ("bumpy", (0.02, 1), 0.0),
    "bumpy03_s1": ("bumpy", (0.03, 1), 0.0),
    "bumpy03_s2_yaw135": ("bumpy", (0.03, 2), 135.0),
    "bumpy04_s1": ("bumpy", (0.04, 1), 0.0),
    "gen0": ("gen", (0,), 0.0),
    "gen1": ("gen", (1,), 0.0),
}
# rooted rays with a reversed sampler range (s_max < s_min: the oracle's root then lies in [z_hi, z_lo]) that a field must offer.
# gen0 has 14-17 of them (the fp64 sphere tracing of a field of slope ~20 differs by a few rays from CPU to CPU).  gen1 has 12-14
# reversed ranges and on every one the first sample is negative, so none has a root: the oracle offers no such ray there, the floor
# is asked of gen0 alone, and gen1's reversed rays must come back as exact zeros.
REVERSED_ROOTED_FLOOR = {"gen0": 1, "gen1": 0}
BUMPY = tuple(k for k, v in FIELDS.items() if v[0] == "bumpy")
GEN = tuple(k for k, v in FIELDS.items() if v[0] == "gen")


# ---- builders (CPU; the GPU side is a .cuda() of a second build: bit-identical parameters) ---------------------------------------
@torch.no_grad()
def bumpy(sigma: float, seed: int):
    net = scenes.build_networks("S0")["sdf_network"]
    v = net.lin0.weight_v
    v[:, 3:] += sigma * torch.randn(v[:, 3:].shape, generator=torch.Generator().manual_seed(seed))
    N._recentre(net)
    return net


@torch.no_grad()
def gen(i: int):
    from iron_amd.fields import SDFNetwork
    return N.generalise(N.build(SDFNetwork, N.sdf_kw("prod"), "prod"), 1000 + i)


def build(name: str):
    kind, args, _ = FIELDS[name]
    return {"bumpy": bumpy, "gen": gen}[kind](*args)


def yaw_of(name: str) -> float:
    return FIELDS[name][2]


# ---- the oracle's two precisions ----------------------------------------------------------------------------------------------
def oracle_fns(net):
    """(f64, f32): x [m, 3] -> sdf [m], the oracle's network in fp64 and in fp32 (the reference's own precision)."""
    spec = N.sdf_spec(N.sdf_kw("prod"))
    sd64 = N.sd64(net)
    sd32 = {k: v.float() for k, v in sd64.items()}
    return (lambda x: R.sdf_forward(sd64, spec, x.double())[:, 0]), (lambda x: R.sdf_forward(sd32, spec, x.float())[:, 0])


def fixture_rays(res: int, yaw: float):
    """fp32 rays of the fixture camera and their unit-sphere segment, from the oracle's camera: the inputs of both sides."""
    K, W2C = scenes.fixture_camera_matrices(res, res, yaw)
    cam = R.CameraSpec(res, res, K, W2C)
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    hit, near, far = R.intersect_sphere(ro, rd, 1.0)
    return ro, rd, near, far, hit


def sampler_ranges(s, t, near, far):
    """raytracer.py:59-65 as R.raytracer_forward forms it, on the unfinished rays: [acc_dis, max_dis] where the last distance is
    positive, [min_dis, acc_dis] where the ray has overshot."""
    pos = (s > 0.0).to(t.dtype)
    return pos * t + (1.0 - pos) * near, pos * far + (1.0 - pos) * t


# ---- the sampler stage with its inner quantities -------------------------------------------------------------------------------
class _Recorder:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, x):
        y = self.fn(x)
        self.calls.append(y)
        return y


def run_sampler(fn, ro, rd, s_min, s_max, dtype, prm=None):
    """R.ray_sampler in `dtype` on the given (fp32) inputs, plus what it computes on the way: the sample distances z and values
    `vals` [k, n], and per ray the bracket (z_lo, f_lo, z_hi, f_hi) it hands to rootfind (defined where `root`)."""
    prm = prm or R.TracerParams(n_steps=N_STEPS)
    o, d, a, b = (x.to(dtype) for x in (ro, rd, s_min, s_max))
    rec = _Recorder(fn)
    root, p, s, t, n_iter = R.ray_sampler(rec, o, d, a.clone(), b.clone(), prm)
    k, n = o.shape[0], prm.n_steps
    n_dense = -(-k * n // prm.max_num_pts)
    vals = torch.cat(rec.calls[:n_dense], dim=0).reshape(k, n)
    lin = torch.linspace(0, 1, steps=n).float().view(1, n)
    z = a.unsqueeze(-1) + lin * (b.unsqueeze(-1) - a.unsqueeze(-1))          # R.ray_sampler's expression, same dtype
    i_neg = first_negative(vals)
    assert torch.equal(root, (i_neg >= 1) & (i_neg < n))                     # this file's reading of the reference's root rule
    i1 = i_neg.clamp(1, n - 1).unsqueeze(-1)
    g = lambda x, i: torch.gather(x, -1, i).squeeze(-1)
    return SimpleNamespace(root=root, p=p, s=s, t=t, n_iter=n_iter, z=z, vals=vals, i_neg=i_neg, z_lo=g(z, i1 - 1), f_lo=g(vals, i1 - 1),
                           z_hi=g(z, i1), f_hi=g(vals, i1))


def first_negative(vals):
    """Index of the first negative sample of every ray; n where there is none."""
    n = vals.shape[1]
    neg = vals < 0
    idx = torch.where(neg, torch.arange(n).view(1, n).expand_as(vals), torch.full_like(vals, n, dtype=torch.long))
    return idx.min(dim=1).values


def sign_changes(vals):
    sg = torch.sign(vals)
    return (sg[:, 1:] != sg[:, :-1]).sum(dim=1)


def classify_sampler(vals64, tau: float):
    """(i_neg, min_abs, decided).  The sampler's outcome on a ray -- root or none, and which bracket -- is fixed by the signs of the
    samples up to and including the first negative one (all of them on a ray without one).  min_abs is the smallest |f| among those;
    the ray is `decided` when it exceeds tau: an evaluation within tau of the oracle's then gives every one of them the same sign."""
    n = vals64.shape[1]
    i_neg = first_negative(vals64)
    keep = torch.arange(n).view(1, n) <= i_neg.view(-1, 1)
    min_abs = torch.where(keep, vals64.abs(), torch.full_like(vals64, float("inf"))).min(dim=1).values
    return i_neg, min_abs, min_abs > tau


def tau_for(vals32, vals64) -> float:
    """max(1e-5, 4 x the largest difference between the oracle's fp32 and fp64 values on the stage's sample points).  1e-5 is 5 x
    the 2e-6 tests/test_gpu_fields.py allows between the h2 core and the oracle on S1."""
    return max(1e-5, 4.0 * float((vals32.double() - vals64.double()).abs().max()))


def bisect64(fn, f_low, f_high, d_low, d_high, ray_o, ray_d, prm=None):
    """R.rootfind restated (raytracer.py:199-220: every ray moves in every iteration, while any initially bracketed ray is wider
    than 2 x threshold), in fp64 on the given inputs; also returns the smallest |f_mid| each ray branched on.  A ray that never met
    |f_mid| <= tau takes the same branches under any evaluation within tau of the oracle's.
    -> (p_mid, d_mid, f_mid, n_iter, min_abs_f_mid)"""
    prm = prm or R.TracerParams(n_steps=N_STEPS)
    f_low, f_high, d_low, d_high, o, d = (x.double().clone() for x in (f_low, f_high, d_low, d_high, ray_o, ray_d))
    work = (f_low > 0) & (f_high < 0)
    d_mid = (d_low + d_high) / 2.0
    met = torch.full_like(d_mid, float("inf"))
    n_iter = 0
    while work.any():
        f_mid = fn(o + d * d_mid.unsqueeze(-1))
        met = torch.minimum(met, f_mid.abs())
        lo = f_mid > 0
        d_low, f_low = torch.where(lo, d_mid, d_low), torch.where(lo, f_mid, f_low)
        d_high, f_high = torch.where(lo, d_high, d_mid), torch.where(lo, f_high, f_mid)
        d_mid = (d_low + d_high) / 2.0
        work &= (d_high - d_low) > 2 * prm.sdf_threshold
        n_iter += 1
    p_mid = o + d * d_mid.unsqueeze(-1)
    return p_mid, d_mid, fn(p_mid), n_iter, met


# ---- one field's stage inputs and oracle results, cached ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
@torch.no_grad()
def stage(name: str, res: int = RES):
    """The oracle's side of the stage comparison on field `name`: fp32 rays; sphere tracing in fp64 (`st`) and fp32 (`st32`); the
    sampler's fp32 ranges on the fp64 run's unfinished rays; the sampler in fp64 (`sa`) and fp32 (`sa32`) on those; tau; the
    classification of the sampler rays."""
    net = build(name)
    f64, f32 = oracle_fns(net)
    prm = R.TracerParams(n_steps=N_STEPS)
    ro, rd, near, far, hit = fixture_rays(res, yaw_of(name))
    st = SimpleNamespace(**dict(zip(("conv", "unf", "p", "s", "t"),
                                    R.sphere_tracing(f64, ro.double(), rd.double(), near.double(), far.double(), hit, prm))))
    st32 = SimpleNamespace(**dict(zip(("conv", "unf", "p", "s", "t"), R.sphere_tracing(f32, ro, rd, near.clone(), far, hit, prm))))
    m = st.unf
    s_min, s_max = (x.float() for x in sampler_ranges(st.s[m], st.t[m], near.double()[m], far.double()[m]))
    sa = run_sampler(f64, ro[m], rd[m], s_min, s_max, torch.float64, prm)
    sa32 = run_sampler(f32, ro[m], rd[m], s_min, s_max, torch.float32, prm)
    # the sampler's own sample points, rounded to fp32 once: what both oracles (and the GPU, test a) are evaluated on for tau
    pts = (ro[m].double().unsqueeze(1) + rd[m].double().unsqueeze(1) * sa.z.unsqueeze(-1)).reshape(-1, 3).float()
    v64, v32 = (torch.cat([f(c) for c in torch.split(pts, prm.max_num_pts)]) for f in (f64, f32))
    tau = tau_for(v32, v64)
    i_neg, min_abs, decided = classify_sampler(sa.vals, tau)
    changes = sign_changes(sa.vals)
    sets = SimpleNamespace(overshoot=st.s[m] < 0, first_neg=i_neg == 0, multi=changes >= 3, reversed=s_max < s_min)
    sets.reversed_rooted = sets.reversed & sa.root
    return SimpleNamespace(name=name, net=net, f64=f64, f32=f32, prm=prm, ro=ro, rd=rd, near=near, far=far, hit=hit, st=st, st32=st32, m=m,
                           s_min=s_min, s_max=s_max, sa=sa, sa32=sa32, tau=tau, i_neg=i_neg, min_abs=min_abs, decided=decided, sets=sets,
                           pts=pts, pts_f64=v64, oracle_noise=float((v32.double() - v64).abs().max()))


def counts(sg) -> dict:
    """The coverage figures of a field (the table of DESIGN.md 3.2)."""
    k = int(sg.m.sum())
    marginal = lambda tau: float((classify_sampler(sg.sa.vals, tau)[1] <= tau).float().mean())
    return {"unfinished": k, "overshoot": int(sg.sets.overshoot.sum()), "roots": int(sg.sa.root.sum()),
            "first_neg": int(sg.sets.first_neg.sum()), "multi": int(sg.sets.multi.sum()),
            "reversed": int(sg.sets.reversed.sum()), "reversed_rooted": int(sg.sets.reversed_rooted.sum()), "marginal_1e-5": marginal(1e-5), "marginal_5e-5": marginal(5e-5),
            "oracle_noise": sg.oracle_noise, "tau": sg.tau, "marginal_tau": float((~sg.decided).float().mean())}


@functools.lru_cache(maxsize=None)
@torch.no_grad()
def oracle_trace(name: str, precision: str = "fp64", res: int = RES, chunk: int = CHUNK):
    """R.raytrace_camera (raytrace_pixels' chunk loop: one raytracer_forward per `chunk` rays, own bisection count each) on field
    `name`: the oracle camera's fp32 rays, everything after them in `precision` -> (result dict, evaluation count, stats)."""
    dtype = torch.float64 if precision == "fp64" else torch.float32
    f64, f32 = oracle_fns(build(name))
    counter = R.EvalCounter()

    def fn(x):
        counter.evals += int(x.shape[0])
        return (f64 if precision == "fp64" else f32)(x)
    K, W2C = scenes.fixture_camera_matrices(res, res, yaw_of(name))
    cam = R.CameraSpec(res, res, K, W2C)
    ro, rd, rn = cam.get_rays(cam.get_uv())
    stats, parts = {}, {}
    for o, d, nrm in zip(*(torch.split(x.to(dtype), chunk, dim=0) for x in (ro.reshape(-1, 3), rd.reshape(-1, 3), rn.reshape(-1)))):
        hit, near, far = R.intersect_sphere(o, d, 1.0)
        r = R.raytracer_forward(fn, o, d, near, far, hit, R.TracerParams(n_steps=N_STEPS), stats)
        r["depth"] = r["distance"] / nrm
        r["ray_d"] = d
        for k, v in r.items():
            parts.setdefault(k, []).append(v)
    out = {k: torch.cat(v, dim=0) for k, v in parts.items()}
    out["depth"] = out["depth"] * out["convergent_mask"].to(dtype)
    return out, counter.evals, stats


def sdf_excess(name: str, ref: dict, sdf, distance, both):
    """How far |sdf - sdf_ref| at the hits of a run exceeds its bound, ray by ray, on the rays `both` runs hit (<= 0: within).  The two
    hits lie |d distance| apart on the same ray, so their values differ by the field's slope along the ray (fp64 oracle, central
    difference) times that distance, plus tau for the evaluation itself (<= tau / 2) and the curvature over <= 2e-4 (second derivative
    ~1e2: 2e-6).  `ref` is oracle_trace(name)'s result.  -> (excess [k], slope [k])"""
    sg = stage(name)
    p_ref, d_ref, h = ref["points"][both].double(), ref["ray_d"][both].double(), 1e-4
    slope = ((sg.f64(p_ref + h * d_ref) - sg.f64(p_ref - h * d_ref)) / (2 * h)).abs()
    d_dist = (distance.double() - ref["distance"].double())[both].abs()
    return (sdf.double() - ref["sdf"].double())[both].abs() - (slope * d_dist + sg.tau), slope
