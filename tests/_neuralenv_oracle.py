"""The oracle's side of the neural relight's checks (iron_amd/neural_relight.py, RayTracer.occluded): shadow rays
off the surface of a field and the reference tracer's answer to them, in fp64 and in fp32 (oracle/iron_ref.py on the CPU).  Shared
by tests/test_neural_relight_oracle.py (CPU) and tests/test_gpu_neural_relight.py.  Test infrastructure: never uses the HIP library.

The shadow-ray recipe: the oracle's fp64 hits of a field on the RES x RES fixture view; K seeded unit directions per hit, reflected
into the hemisphere of the hit's normal (the normalised fp64 gradient); origin x + EPS n; everything rounded to fp32 once, then cut
to the unit sphere by the oracle's intersect_sphere.  Both sides of every comparison start from these fp32 numbers.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

from oracle import iron_ref as R
from iron_amd import scenes

import _hard_fields as H
import _nets as N

RES = 24        # the view whose hits carry the shadow rays
K = 8           # directions per hit
EPS = 1e-3      # the relight's default shadow_eps
SEED = 61
FIELDS = ("S0", "bumpy04_s1", "gen0")


def build(name: str):
    """CPU network of a field: S0 is the scene of iron_amd.scenes, the others are tests/_hard_fields.py's."""
    return scenes.build_networks("S0")["sdf_network"] if name == "S0" else H.build(name)


def yaw_of(name: str) -> float:
    return 0.0 if name == "S0" else H.yaw_of(name)


@functools.lru_cache(maxsize=None)
@torch.no_grad()
def shadow_rays(name: str, res: int = RES, k: int = K, eps: float = EPS, seed: int = SEED):
    """-> o, w [m, 3], near, far [m] (fp32), work [m] bool, n_hits: the recipe's shadow rays of field `name`."""
    net = build(name)
    f64, _ = H.oracle_fns(net)
    ro, rd, near, far, hit = H.fixture_rays(res, yaw_of(name))
    r = R.raytracer_forward(f64, ro.double(), rd.double(), near.double(), far.double(), hit, R.TracerParams(n_steps=H.N_STEPS))
    x = r["points"][r["convergent_mask"]]
    _, _, grad = R.sdf_get_all(N.sd64(net), N.sdf_spec(N.sdf_kw("prod")), x)
    n = grad / grad.norm(dim=-1, keepdim=True)
    w = torch.randn((x.shape[0], k, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    w = w / w.norm(dim=-1, keepdim=True)
    w = torch.where(((w * n[:, None, :]).sum(-1) < 0)[..., None], -w, w)
    o = (x + eps * n)[:, None, :].expand(-1, k, -1)
    o, w = o.reshape(-1, 3).float().contiguous(), w.reshape(-1, 3).float().contiguous()
    work, s_near, s_far = R.intersect_sphere(o, w, 1.0)
    return SimpleNamespace(o=o, w=w, near=s_near.contiguous(), far=s_far.contiguous(), work=work.contiguous(), n_hits=int(x.shape[0]))


@functools.lru_cache(maxsize=None)
@torch.no_grad()
def oracle_occluded(name: str, precision: str = "fp64") -> torch.Tensor:
    """The reference tracer's convergent_mask on shadow_rays(name), everything after the fp32 rays in `precision`."""
    dtype = torch.float64 if precision == "fp64" else torch.float32
    f64, f32 = H.oracle_fns(build(name))
    s = shadow_rays(name)
    r = R.raytracer_forward(f64 if precision == "fp64" else f32, s.o.to(dtype), s.w.to(dtype), s.near.to(dtype), s.far.to(dtype), s.work,
                            R.TracerParams(n_steps=H.N_STEPS))
    return r["convergent_mask"]


def precision_gap(name: str) -> float:
    """The share of shadow_rays(name) on which the oracle's fp32 run and its fp64 run disagree: what the reference's own precision
    leaves open, the allowance of the GPU comparison."""
    a, b = oracle_occluded(name, "fp64"), oracle_occluded(name, "fp32")
    return float((a != b).double().mean())
