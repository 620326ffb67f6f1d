"""High-precision side of the per-operator tests of the silhouette and hole-filling kernels (tests/test_silhouette_oracle.py on the
CPU, tests/test_gpu_silhouette_kernels.py on the GPU): iron_camera_rays, iron_intersect_sphere, iron_fill_holes, iron_edge_pixels,
iron_edge_sides, iron_edge_blend of csrc/pointwise.hip and the surface walk k_edge_walk_h2 of csrc/shade.hip.

The truth is oracle/iron_ref.py evaluated in fp64 from the fp32 tensors the kernels get unchanged (_neus_oracle.run_as / fp64).
Where the oracle does not expose an intermediate -- the side uv and the blend weight of render_edge_pixels, `tmp` of
intersect_sphere, the walk with its per-step dot, the fill rule -- the few lines are restated here, dtype-generic, and the CPU file
asserts that each restatement equals the oracle's own function in fp64 on the same inputs.  The yardstick of every tolerance is the
deviation of an honest fp32 evaluation (torch, CPU) of the same formula from the fp64 one, per block of rows of similar conditioning
(`check_blocks`); discrete decisions no fp32 evaluation can be asked to reproduce are flagged from the fp64 side only.  The input
builders live here so that both test files see the same tensors.  Nothing here touches the GPU.
"""
from __future__ import annotations

import copy
import functools
import math
from types import SimpleNamespace
from typing import Dict, List, Tuple

import numpy as np
import torch

from oracle import iron_ref as R
from iron_amd import scenes

import _hard_fields as HF
import _nets as NETS
from _neus_oracle import run_as, ulp32

FACTOR, ABS = 4.0, 1e-7     # |kernel - fp64| <= FACTOR x fp32 floor + ABS
BIG_N = 2048 * 256 + 257    # one grid-stride trip of the pointwise kernels (2048 blocks of 256) plus a ragged second one
RADIUS = 0.707              # render_edge_pixels' pixel disc
HIT_DEPTH = 1e-2            # fill_holes: closed depth > 1e-2 is a hit
WALK_STEP, WALK_THRESHOLD, WALK_MAX_STEP = 1e-3, 5e-2, 16
WALK_MARGIN = 1e-4          # a candidate is decided when no step's ||n.v| - threshold| came closer than this
WALK_FIELDS = ("bumpy03_s1", "gen0")
WALK_POOL = 300             # per field: 268 on-surface candidates, then WALK_DISPLACED displaced by +-2e-3 along the normal
WALK_DISPLACED = 32
NOMINAL_CUS = 256           # compute units of an MI355X: the walk's grid is min(tiles, CUs)
CAP_UNDECIDED, CAP_PIXEL_FLAGS = 0.03, 0.02


# ---- the tolerance rule ------------------------------------------------------------------------------------------------------
def _rows(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return x.reshape(x.shape[0], -1).max(dim=1)[0] if x.dim() > 1 else x


def check_blocks(tag: str, got: torch.Tensor, ref64: torch.Tensor, dev: torch.Tensor, blocks: Dict[str, torch.Tensor], pop=None) -> float:
    """The rule |got - fp64| <= 4 x floor + 1e-7 per block of rows: `dev` is |fp32 oracle - fp64 oracle| entry by entry, the floor of
    a block its largest entry there.  A floor is the spread of fp32 roundings over a population of rows of one conditioning, which a
    single row or a handful does not sample (the one ray of an n = 1 case may round to within 1e-9 of its fp64 value, and an honest
    kernel lands an ulp away): a case of few rows passes `pop` = (dev, blocks) of the same builder's larger draw, and the floor of a
    block is then the larger of the two -- still the reference's own error on rows built alike, and nothing of the kernel's.
    Prints one `sil-k` line per block (floor, error, ratio) and returns the worst ratio."""
    err = _rows((got.detach().cpu().double().reshape(ref64.shape) - ref64).abs())
    dev = _rows(dev)
    worst = 0.0
    for name, rows in blocks.items():
        if rows.dtype == torch.bool and not bool(rows.any()) or rows.numel() == 0:
            continue
        floor, e = float(dev[rows].max()), float(err[rows].max())
        if pop is not None and name in pop[1] and bool(pop[1][name].any()):
            floor = max(floor, float(_rows(pop[0])[pop[1][name]].max()))
        ratio = e / (FACTOR * floor + ABS)
        print("sil-k %s [%s] rows=%d floor=%.3e err=%.3e ratio=%.3f" % (tag, name, int(rows.sum()) if rows.dtype == torch.bool else rows.numel(),
                                                                         floor, e, ratio))
        worst = max(worst, ratio)
    return worst


# ---- cameras -----------------------------------------------------------------------------------------------------------------
def cam_as(cam: R.CameraSpec, dtype) -> R.CameraSpec:
    """The oracle camera with its four fp32 matrices -- K, W2C and the fp32 inverses the kernels are handed -- cast to `dtype`."""
    c = copy.copy(cam)
    for k in ("K", "W2C", "K_inv", "C2W"):
        setattr(c, k, getattr(cam, k).to(dtype))
    return c


def fixture_camera(res_w: int = 56, res_h: int = 56, yaw: float = 0.0) -> R.CameraSpec:
    K, W2C = scenes.fixture_camera_matrices(res_w, res_h, yaw)
    return R.CameraSpec(res_w, res_h, K, W2C)


def ray_cameras() -> Dict[str, R.CameraSpec]:
    """The fixture camera at yaw 0 and 135, a crop window whose principal point is negative in both axes, and a camera resized by
    the non-integer factors 1.37 and 0.83."""
    c0, c135 = fixture_camera(56, 56, 0.0), fixture_camera(56, 56, 135.0)
    crop = c0.crop(20, 16, (70, 61))
    assert float(crop.K[0, 2]) < 0 and float(crop.K[1, 2]) < 0
    return {"yaw0": c0, "yaw135": c135, "crop": crop, "resized": c135.scaled(int(56 * 1.37), int(56 * 0.83))}


def ray_uv(cam: R.CameraSpec, n: int, seed: int = 7) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """[n, 2] fp32 uv: alternately a pixel centre and an off-centre sample of the kind k_edge_sides produces (centre +- 0.707 x a unit
    vector); the pixels run from 12 outside the image on one side to 12 outside on the other.  -> (uv, blocks)."""
    gen = torch.Generator().manual_seed(seed + n % 1000)
    px = torch.floor(torch.rand(n, 2, generator=gen) * torch.tensor([cam.W + 24.0, cam.H + 24.0]) - 12.0) + 0.5
    ang = torch.rand(n, generator=gen) * (2 * math.pi)
    off = RADIUS * torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1) * torch.where(torch.rand(n, 1, generator=gen) < 0.5, -1.0, 1.0)
    centre = torch.arange(n) % 2 == 0
    uv = torch.where(centre[:, None], px, px + off).contiguous()
    return uv, {"centre": centre, "off-centre": ~centre}


def get_rays(cam: R.CameraSpec, uv: torch.Tensor, dtype) -> Dict[str, torch.Tensor]:
    o, d, dn = run_as(dtype, R.CameraSpec.get_rays, cam_as(cam, dtype), uv)
    return {"ray_o": o, "ray_d": d, "ray_d_norm": dn}


POP_RAYS, POP_SPHERE, POP_EDGE_PIXELS, POP_SIDES = 255, 255, 300, 130   # the draws small cases take their floors from


def rays_pop(cam: R.CameraSpec):
    uv, blocks = ray_uv(cam, POP_RAYS)
    return deviation(get_rays(cam, uv, torch.float32), get_rays(cam, uv, torch.float64)), blocks


def deviation(lo: Dict[str, torch.Tensor], hi: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: (lo[k].double() - hi[k].double()).abs() for k in hi if torch.is_tensor(hi[k]) and hi[k].is_floating_point()}


# ---- intersect_sphere --------------------------------------------------------------------------------------------------------
def intersect_sphere_parts(ray_o, ray_d, r: float):
    """R.intersect_sphere (raytracer.py:223-237) with its `tmp` exposed, in the dtype of the arguments."""
    d1 = -torch.sum(ray_d * ray_o, dim=-1) / torch.sum(ray_d * ray_d, dim=-1)
    p = ray_o + d1.unsqueeze(-1) * ray_d
    tmp = r * r - torch.sum(p * p, dim=-1)
    d2 = torch.sqrt(torch.clamp(tmp, min=0.0)) / torch.norm(ray_d, dim=-1)
    return {"mask": tmp > 0.0, "near": torch.clamp(d1 - d2, min=0.0), "far": d1 + d2, "tmp": tmp}


def r32(r: float) -> float:
    """The radius as the kernel gets it: a C float."""
    return float(np.float32(r))


GRAZE_EPS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7)
SPHERE_RADII = (0.5, 1.0, 1.2)
SPHERE_CASES = tuple((r, n) for r in SPHERE_RADII for n in (1, 255, 257)) + ((1.0, BIG_N),)   # the large call is made once
SPHERE_NAMED = {"through_centre": 0, "inside_origin": 1, "behind": 2}


def sphere_rays(r: float, n: int, seed: int = 3):
    """Hand-built rays for a sphere of radius r about the origin, [n, 3] fp32 origins and directions of length 0.5, 1 or 3:
    row 0 runs through the centre, row 1 starts inside (near = 0), row 2 has the sphere behind it (far < 0, mask true); then a
    regular block -- impact parameter in [0, 0.9 r] or [1.1 r, 2 r], origin in front, behind or inside -- and, the last third, the
    grazing block with impact parameter r (1 +- eps), eps from 1e-2 down to 1e-7.  -> (o, d, blocks)"""
    gen = torch.Generator().manual_seed(seed + n % 1000 + int(r * 10))
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    u = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=-1)        # direction
    a = torch.nn.functional.normalize(torch.cross(u, torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=-1), dim=-1)  # _|_ u
    graze = torch.arange(n) >= n - n // 3
    frac = torch.where(rnd(n) < 0.6, 0.9 * rnd(n), 1.1 + 0.9 * rnd(n))
    eps = torch.tensor(GRAZE_EPS, dtype=torch.float64)[torch.arange(n) % len(GRAZE_EPS)] * torch.where(torch.arange(n) // len(GRAZE_EPS) % 2 == 0, 1.0, -1.0)
    b = r * torch.where(graze, 1.0 + eps, frac)                                                   # impact parameter
    kind = torch.randint(0, 3, (n,), generator=gen)                                               # 0 in front, 1 behind, 2 inside
    kind = torch.where(graze, torch.zeros_like(kind), kind)
    t0 = torch.where(kind == 0, 1.5 + 2.5 * rnd(n), torch.where(kind == 1, -(1.5 + 2.5 * rnd(n)), 0.3 * r * (rnd(n) - 0.5)))
    b = torch.where((kind == 2) & ~graze, b.clamp(max=0.6 * r), b)
    o = b[:, None] * a - t0[:, None] * u
    length = torch.tensor([0.5, 1.0, 3.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=gen)]
    d = u * length[:, None]
    named = torch.zeros(n, dtype=torch.bool)
    if n >= 3:
        o[0], d[0] = -2.5 * u[0], u[0]
        o[1], d[1] = 0.3 * r * a[1], 0.5 * u[1]
        o[2], d[2] = 2.0 * u[2] + 0.2 * r * a[2], 3.0 * u[2]
        named[:3] = True
    elif n == 1:
        graze = torch.zeros(1, dtype=torch.bool)
        o[0], d[0] = -2.5 * u[0] + 0.3 * r * a[0], u[0]
    return o.float().contiguous(), d.float().contiguous(), {"regular": ~graze, "grazing": graze}


def sphere_pop(r: float):
    o, d, blocks = sphere_rays(r, POP_SPHERE)
    return deviation(run_as(torch.float32, intersect_sphere_parts, o, d, r32(r)), run_as(torch.float64, intersect_sphere_parts, o, d, r32(r))), blocks


def sphere_flags(o, d, r: float, blocks) -> torch.Tensor:
    """[n] bool from the fp64 side: |tmp| below 8 x the fp32 floor of tmp on the row's block -- an fp32 tmp may have the other sign."""
    hi = run_as(torch.float64, intersect_sphere_parts, o, d, r32(r))
    lo = run_as(torch.float32, intersect_sphere_parts, o, d, r32(r))
    dev = (lo["tmp"].double() - hi["tmp"]).abs()
    flag = torch.zeros(o.shape[0], dtype=torch.bool)
    for rows in blocks.values():
        if bool(rows.any()):
            flag |= rows & (hi["tmp"].abs() < 8.0 * float(dev[rows].max()))
    return flag


# ---- fill_holes --------------------------------------------------------------------------------------------------------------
def fill_rule(res: Dict[str, torch.Tensor], closed: torch.Tensor):
    """The fill_holes lines of R.raytrace_camera_full (raytracer.py:554-564) on a results dict and a closed depth image, in their
    dtype; not in place.  -> (depth, convergent_mask, distance, points, flag)"""
    depth, conv, distance, points = res["depth"].clone(), res["convergent_mask"].clone(), res["distance"].clone(), res["points"].clone()
    new_conv = closed > HIT_DEPTH
    upd = new_conv & (~conv)
    flag = int(bool(upd.any()))
    if flag:
        depth[upd] = closed[upd]
        conv = new_conv
        distance = depth * res["ray_d_norm"]
        points = res["ray_o"] + res["ray_d"] * distance.unsqueeze(-1)
    return {"depth": depth, "convergent_mask": conv, "distance": distance, "points": points, "flag": flag}


FILL_SHAPES = ((1, 1), (3, 5), (17, 67))
FILL_CASES = ("a", "b", "c")


def fill_inputs(shape, case: str, seed: int = 13):
    """A synthetic results dict (fp32, [H, W, ...]) and a closed depth image for it.  The closing itself is pinned elsewhere, so the
    closed image is drawn on its own: about 60 % hits of depth 0.5 .. 2.5, else 0.  The stored distance and points are random, so an
    untouched buffer and a recomputed one cannot be confused.
    a: closed is 0 wherever the pixel is not convergent -- no hole is filled, the flag stays down -- and 0 on some convergent ones too;
    b: some non-convergent pixels have closed > 1e-2;
    c: as b, plus (where the image has the pixels for it) a convergent pixel with closed = 5e-3, which loses its mask, a convergent
       and a non-convergent one with closed = float32(1e-2) exactly, which are no hits.  A 1 x 1 image has room for one of these only:
       its single convergent pixel has closed = float32(1e-2), nothing is filled and the flag stays down."""
    H, W = shape
    gen = torch.Generator().manual_seed(seed + 100 * H + W + ord(case))
    rnd = lambda *s: torch.rand(*s, generator=gen)
    conv = rnd(H, W) < 0.5
    closed = torch.where(rnd(H, W) < 0.6, 0.5 + 2.0 * rnd(H, W), torch.zeros(H, W))
    special = {}
    if case == "a":
        closed = closed * conv
    else:
        flat_c, flat_z = conv.view(-1), closed.view(-1)
        flat_c[0], flat_z[0] = False, 0.7                       # at least one hole that is filled
        if case == "c":
            if H * W == 1:
                flat_c[0], flat_z[0] = True, float(np.float32(HIT_DEPTH))
                special = {"exact_hit": 0}
            else:
                flat_c[1], flat_z[1] = True, 5e-3
                flat_c[2], flat_z[2] = True, float(np.float32(HIT_DEPTH))
                flat_c[3], flat_z[3] = False, float(np.float32(HIT_DEPTH))
                special = {"loses_mask": 1, "exact_hit": 2, "exact_hole": 3}
    depth = conv.float() * (0.3 + rnd(H, W))
    o = torch.tensor([0.1, -0.2, 2.0]).expand(H, W, 3).contiguous()
    d = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=gen), dim=-1)
    res = {"depth": depth, "convergent_mask": conv, "distance": 5.0 * rnd(H, W), "points": torch.randn(H, W, 3, generator=gen),
           "ray_o": o, "ray_d": d, "ray_d_norm": 1.0 + rnd(H, W)}
    return res, closed.contiguous(), special


# ---- edge pixels: projection and first-candidate-wins ------------------------------------------------------------------------
EDGE_PIXEL_N = (1, 63, 300, 70000)
EDGE_PIXEL_IMAGES = (8, 56)
WRAP_ROWS = {"u<0": 0, "u>=W": 1}


def edge_pixel_inputs(res: int, n: int, seed: int = 17):
    """Candidates for iron_edge_pixels on the res x res fixture camera: uv drawn uniformly from [-res/2, 3 res/2]^2 (so the fractions
    are uniform and all four sides are left), a depth of 0.5 .. 4 along the pixel's ray, three in four in front of the camera and the
    rest behind it (q_z < 0: a finite, mirrored uv).  Rows 0 and 1 are the wrap-around rows, in front and found: u < 0 with
    1 <= v < H, and u >= W with v < H - 1 -- their flat index v W + u is in range.  `found` is mixed (n = 1: found).
    -> (cam, points [n,3] fp32, found [n] bool, blocks)"""
    cam = fixture_camera(res, res)
    gen = torch.Generator().manual_seed(seed + res + n % 1000)
    uv = (torch.rand(n, 2, generator=gen, dtype=torch.float64) * 2.0 - 0.5) * res
    behind = torch.rand(n, generator=gen) < 0.25
    found = torch.rand(n, generator=gen) < 0.7
    if n == 1:
        uv[0] = torch.tensor([res * 0.4 + 0.3, res * 0.6 + 0.37], dtype=torch.float64)
        behind[0], found[0] = False, True
    if n >= 2:
        uv[0] = torch.tensor([-2.3, 3.6], dtype=torch.float64)
        uv[1] = torch.tensor([res + 1.4, 2.2], dtype=torch.float64)
        behind[:2], found[:2] = False, True
    t = 0.5 + 3.5 * torch.rand(n, generator=gen, dtype=torch.float64)
    o, d, dn = R.CameraSpec.get_rays(cam_as(cam, torch.float64), uv)
    pts = o + d * (dn * t * torch.where(behind, -1.0, 1.0))[:, None]     # camera-space depth +-t
    return cam, pts.float().contiguous(), found, {"in front": ~behind, "behind": behind}


def edge_pixels_pop(res: int):
    cam, pts, found, blocks = edge_pixel_inputs(res, POP_EDGE_PIXELS)
    return (project(cam, pts, torch.float32).double() - project(cam, pts, torch.float64)).abs(), blocks


def project(cam: R.CameraSpec, points: torch.Tensor, dtype) -> torch.Tensor:
    return run_as(dtype, R.project, cam_as(cam, dtype), points)


def pixel_of(uv: torch.Tensor, cam) -> torch.Tensor:
    """locate_edge_points' flat pixel index (raytracer.py:487-490): floor(v) W + floor(u), range-checked as a whole; -1 when outside."""
    f = torch.floor(uv).long()
    pix = f[:, 1] * cam.W + f[:, 0]
    return torch.where((pix >= 0) & (pix < cam.H * cam.W), pix, torch.full_like(pix, -1))


def first_winner(pix: torch.Tensor, found: torch.Tensor, n_pix: int) -> torch.Tensor:
    """[n_pix] long: the smallest index of a found candidate that lands in the pixel, n (= none) otherwise."""
    n = pix.shape[0]
    ok = found & (pix >= 0)
    win = torch.full((n_pix,), n, dtype=torch.long)
    return win.scatter_reduce(0, pix[ok], torch.arange(n)[ok], reduce="amin", include_self=True)


def edge_pixel_truth(cam, points, found, blocks):
    """fp64 uv, the fp32 oracle's uv, the per-block uv floor, delta = 8 x floor per candidate, the flagged candidates (u or v within
    delta of an integer), the fp64 winner per pixel and the pixels excused from the `first` comparison: those a flagged, found
    candidate may enter or leave (every pixel floor(v +- delta) W + floor(u +- delta) it can reach) when its index is not above the
    pixel's winner -- a flagged candidate behind the winner cannot change it."""
    uv64, uv32 = project(cam, points, torch.float64), project(cam, points, torch.float32)
    dev = (uv32.double() - uv64).abs().max(dim=1)[0]
    delta = torch.zeros_like(dev)
    pop = edge_pixels_pop(cam.W) if points.shape[0] < POP_EDGE_PIXELS else None
    for name, rows in blocks.items():
        if bool(rows.any()):
            floor = float(dev[rows].max())
            if pop is not None:
                floor = max(floor, float(_rows(pop[0])[pop[1][name]].max()))
            delta[rows] = 8.0 * floor
    near_int = ((uv64 - torch.round(uv64)).abs() < delta[:, None]).any(dim=1)
    n_pix = cam.H * cam.W
    win = first_winner(pixel_of(uv64, cam), found, n_pix)
    excused = torch.zeros(n_pix, dtype=torch.bool)
    idx = (near_int & found).nonzero().reshape(-1)
    for su in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            alt = pixel_of(uv64[idx] + delta[idx, None] * torch.tensor([su, sv], dtype=torch.float64), cam)
            ok = alt >= 0
            hit = idx[ok] <= win[alt[ok]]
            excused[alt[ok][hit]] = True
    return SimpleNamespace(uv64=uv64, uv32=uv32, dev=dev, delta=delta, flagged=near_int, winner=win, excused=excused)


# ---- edge sides and blend ----------------------------------------------------------------------------------------------------
def edge_sides(edge_uv, grads, w2c):
    """The geometry lines of R.render_edge_pixels (raytracer.py:680-698) in the dtype of the arguments: the two side samples and the
    area weight of the positive side, plus the length of the normal's image-plane projection before it is normalised."""
    center = torch.floor(edge_uv) + 0.5
    nrm = grads / (grads.norm(dim=-1, keepdim=True) + 1e-10)
    n2d = torch.matmul(nrm, w2c[:3, :3].transpose(1, 0))[:, :2]
    plen = n2d.norm(dim=-1)
    n2d = n2d / (n2d.norm(dim=-1, keepdim=True) + 1e-10)
    pos_uv = center - RADIUS * n2d
    neg_uv = center + RADIUS * n2d
    dot2d = torch.sum((edge_uv - center) * n2d, dim=-1)
    alpha = 2 * torch.arccos(torch.clamp(dot2d / RADIUS, min=0.0, max=1.0))
    w_pos = 1.0 - (alpha - torch.sin(alpha)) / (2.0 * np.pi)
    return {"pos_uv": pos_uv, "neg_uv": neg_uv, "weight": w_pos, "plen": plen}


ILL_LENGTHS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9)
ILL_ANGLES = 8              # rows per length, at different angles in the image plane
ILL_COMPARED = 1e-3         # ill-conditioned rows with an fp64 projected length >= this are compared like the rest
SIDES_EDGE_ROWS = ("on_centre", "against_normal", "ratio_ge_1", "just_below_1", "just_above_0")


def edge_sides_inputs(n: int, seed: int = 23):
    """edge_uv [n,2], gradients [n,3] (fp32) for the fixture camera.  n = 1: one generic row.  Otherwise, in order: the five edge rows
    of SIDES_EDGE_ROWS (twice: unit and 3.7 x gradients), the ill-conditioned block -- normals whose image-plane projection has
    length ILL_LENGTHS (ILL_ANGLES rows each), then the exactly zero gradient -- and generic rows: random unit and non-unit gradients, uv in [-20, 76).
    -> (cam, edge_uv, grads, kind, rows)   kind: 0 generic, 1 edge row, 2 ill-conditioned; rows: name -> list of row indices"""
    cam = fixture_camera(56, 56)
    gen = torch.Generator().manual_seed(seed + n)
    rot = cam.W2C[:3, :3].double()
    uv = torch.rand(n, 2, generator=gen, dtype=torch.float64) * 96.0 - 20.0
    g = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    g = torch.where(torch.arange(n)[:, None] % 2 == 0, torch.nn.functional.normalize(g, dim=-1), g * 2.0)
    rows = {k: [] for k in SIDES_EDGE_ROWS}
    rows.update({"ill": [], "zero": []})
    kind = torch.zeros(n, dtype=torch.long)             # 0 generic, 1 edge rows, 2 ill-conditioned
    if n > 1:
        i = 0
        diag = torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64) / math.sqrt(2.0)
        for scale in (1.0, 3.7):
            for name in SIDES_EDGE_ROWS:
                centre = torch.tensor([10.5 + i, 20.5 - 3 * i], dtype=torch.float64)
                g[i] = scale * (rot.T @ diag)            # image-plane normal (1, 1) / sqrt 2
                step = {"on_centre": 0.0, "against_normal": -0.3, "ratio_ge_1": 0.4999985 * math.sqrt(2.0),
                        "just_below_1": RADIUS * (1.0 - 1e-4), "just_above_0": 1e-5}[name]
                uv[i] = centre + step * diag[:2]
                rows[name].append(i)
                kind[i] = 1
                i += 1
        for length in ILL_LENGTHS:
            for k in range(ILL_ANGLES):
                phi = 0.7 + i
                g[i] = (1.0 if k % 2 == 0 else 2.3) * (rot.T @ torch.tensor([length * math.cos(phi), length * math.sin(phi), math.sqrt(1.0 - length * length)],
                                                                           dtype=torch.float64))
                rows["ill"].append(i)
                kind[i] = 2
                i += 1
        g[i] = 0.0
        rows["zero"].append(i)
        kind[i] = 2
        i += 1
        assert i < n
    return cam, uv.float().contiguous(), g.float().contiguous(), kind, rows


def sides_pop():
    cam, uv, g, kind, rows = edge_sides_inputs(POP_SIDES)
    return deviation(run_as(torch.float32, edge_sides, uv, g, cam.W2C), run_as(torch.float64, edge_sides, uv, g, cam.W2C)), {"generic": kind == 0}


def edge_blend_inputs(n: int, n_pixels: int, seed: int = 29):
    """Inputs of iron_edge_blend: side colours [2n,3] >= 0, weights in [0,1] (some exactly 0, 0.5 and 1), gradients, uv, points, and
    n distinct pixel indices of which (n > 1) rows 3 and n-2 are -1 and n_pixels: skipped."""
    gen = torch.Generator().manual_seed(seed + n)
    w = torch.rand(n, generator=gen)
    if n > 6:
        w[0], w[1], w[2] = 0.0, 0.5, 1.0
    pixel = torch.randperm(n_pixels, generator=gen)[:n].contiguous()
    if n > 1:
        pixel[3], pixel[n - 2] = -1, n_pixels
    return {"side_color": 3.0 * torch.rand(2 * n, 3, generator=gen), "weight": w, "grads": torch.randn(n, 3, generator=gen),
            "edge_uv": 56.0 * torch.rand(n, 2, generator=gen), "edge_points": torch.randn(n, 3, generator=gen), "pixel": pixel}


def blend(pos_color, neg_color, w):
    """raytracer.py:709 in the dtype of the arguments."""
    return pos_color * w.unsqueeze(-1) + neg_color * (1.0 - w.unsqueeze(-1))


def oracle_edge_geometry(cam, edge_uv, grads, pos_color, neg_color, dtype):
    """R.render_edge_pixels itself in `dtype` with the network, the tracer and the shading replaced by stand-ins that hand it `grads`
    and the two side colours: what it asks the tracer for are its side uv, and the colour it writes is its blend."""
    n = edge_uv.shape[0]
    seen = []
    real = R.sdf_get_all, R.raytrace_pixels, R.render_normal_and_color
    colors = [pos_color.to(dtype), neg_color.to(dtype)]

    def fake_trace(scene, uv, cam_, prm=None):
        seen.append(uv.clone())
        return {"color": colors[len(seen) - 1], "normal": torch.zeros(n, 3, dtype=dtype), "convergent_mask": torch.zeros(n, dtype=torch.bool)}

    R.sdf_get_all = lambda sd, spec, x: (None, None, grads.to(dtype))
    R.raytrace_pixels = fake_trace
    R.render_normal_and_color = lambda scene, res: None
    try:
        res = {"edge_points": torch.zeros(n, 3), "edge_uv": edge_uv, "edge_pixel_idx": torch.arange(n), "color": torch.zeros(n, 3),
               "normal": torch.zeros(n, 3), "uv": torch.zeros(n, 2), "points": torch.zeros(n, 3)}
        scene = SimpleNamespace(sdf_sd=None, sdf_spec=None)
        res = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in res.items()}
        run_as(dtype, R.render_edge_pixels, scene, res, cam_as(cam, dtype))
    finally:
        R.sdf_get_all, R.raytrace_pixels, R.render_normal_and_color = real
    return {"pos_uv": seen[0], "neg_uv": seen[1], "color": res["color"], "normal": res["normal"], "uv": res["uv"], "points": res["points"]}


# ---- the surface walk --------------------------------------------------------------------------------------------------------
def walk_camera_origin() -> torch.Tensor:
    """The camera origin of scenes.fixture_camera_matrices(56, 56), fp32 [3]."""
    return fixture_camera(56, 56).C2W[:3, 3].clone()


def _field(name: str):
    net = HF.build(name)
    return NETS.sd64(net), NETS.sdf_spec(NETS.sdf_kw("prod"))


def _get_all(sd, spec, x):
    s, _, g = R.sdf_get_all(sd, spec, x)
    return s[:, 0], g


@torch.no_grad()
def walk(sd64, spec, start, cam_o, max_step: int, dtype, step_size: float = WALK_STEP, threshold: float = WALK_THRESHOLD):
    """The walk of R.locate_edge_points (raytracer.py:440-478) restated in `dtype` with what it decides on recorded per candidate:
    -> final points [n,3], found [n], the number of moves made, and the smallest ||n.v| - threshold| over the steps at which the
    candidate was still moving (its margin)."""
    def body(start, cam_o):
        sd = {k: v.to(dtype) for k, v in sd64.items()}
        cur = start.clone()
        n = cur.shape[0]
        found = torch.zeros(n, dtype=torch.bool)
        moves = torch.zeros(n, dtype=torch.long)
        margin = torch.full((n,), float("inf"), dtype=torch.float64)
        for i in range(max_step + 1):
            idx = (~found).nonzero().reshape(-1)
            if idx.numel() == 0:
                break
            x = cur[idx]
            view = cam_o.view(1, 3) - x
            view = view / (view.norm(dim=-1, keepdim=True) + 1e-10)
            parts = [R.sdf_get_all(sd, spec, c) for c in torch.split(x, 4096)]
            sdf, nrm = torch.cat([p[0] for p in parts]), torch.cat([p[2] for p in parts])
            nrm = nrm / (nrm.norm(dim=-1, keepdim=True) + 1e-10)
            dot = (nrm * view).sum(dim=-1)
            moving = dot.abs() > threshold
            margin[idx] = torch.minimum(margin[idx], (dot.abs().double() - threshold).abs())
            found[idx] = ~moving
            if i >= max_step:
                break
            w = nrm - view / dot.unsqueeze(-1)
            w = w / (w.norm(dim=-1, keepdim=True) + 1e-10)
            w = w - sdf * nrm
            cur[idx[moving]] += (step_size * w)[moving]
            moves[idx[moving]] += 1
        return cur, found, moves, margin
    return run_as(dtype, body, start, cam_o)


def oracle_walk(sd64, spec, start, cam_o, max_step: int, dtype, step_size: float = WALK_STEP, threshold: float = WALK_THRESHOLD):
    """R.locate_edge_points itself in `dtype`: the found candidates' final points in candidate order, as it hands them to project()."""
    seen = {}
    real = R.project

    def spy(cam, pts):
        seen["points"] = pts.clone()
        return torch.zeros(pts.shape[0], 2, dtype=pts.dtype)

    R.project = spy
    try:
        sd = {k: v.to(dtype) for k, v in sd64.items()}
        scene = SimpleNamespace(sdf_sd=sd, sdf_spec=spec)
        cam = SimpleNamespace(C2W=torch.cat([torch.eye(3, dtype=dtype), cam_o.to(dtype).view(3, 1)], dim=1), H=1, W=1)
        run_as(dtype, R.locate_edge_points, scene, cam, start, torch.ones(start.shape[0], dtype=torch.bool), max_step=max_step,
               step_size=step_size, dot_threshold=threshold)
    finally:
        R.project = real
    return seen.get("points", torch.zeros(0, 3, dtype=dtype))


@functools.lru_cache(maxsize=None)
@torch.no_grad()
def walk_starts(field: str, n: int, seed: int = 31):
    """[n, 3] fp32 start points on the zero level set of `field`: random directions at radius 0.5 (taken from the band in which the
    sphere's own normal has |n.v| < 0.2, so that few draws are wasted), six fp64 Newton steps x -= s g / |g|^2, rounded to fp32, kept
    when |s| <= 1e-4 and |n.v| < 0.12 there.  The candidates at positions WALK_POOL - WALK_DISPLACED .. WALK_POOL - 1 are displaced by
    +-2e-3 along the normal.  A shorter list is a prefix of a longer one."""
    sd, spec = _field(field)
    cam_o = walk_camera_origin().double()
    gen = torch.Generator().manual_seed(seed)
    kept = []
    total = 0
    while total < n:
        d = torch.nn.functional.normalize(torch.randn(4096, 3, generator=gen, dtype=torch.float64), dim=-1)
        v = torch.nn.functional.normalize(cam_o.view(1, 3) - 0.5 * d, dim=-1)
        x = 0.5 * d[(d * v).sum(-1).abs() < 0.2]          # every batch is drawn alike, whatever n: a shorter list is a prefix
        for _ in range(6):
            s, g = _get_all(sd, spec, x)
            x = x - s[:, None] * g / (g * g).sum(-1, keepdim=True)
        x = x.float().double()
        s, g = _get_all(sd, spec, x)
        nrm = torch.nn.functional.normalize(g, dim=-1)
        v = torch.nn.functional.normalize(cam_o.view(1, 3) - x, dim=-1)
        ok = (s.abs() <= 1e-4) & ((nrm * v).sum(-1).abs() < 0.12)
        x, nrm = x[ok], nrm[ok]
        lo, hi = WALK_POOL - WALK_DISPLACED - total, WALK_POOL - total          # positions of this batch that belong to the displaced block
        if hi > 0 and lo < x.shape[0]:
            rows = torch.arange(max(lo, 0), min(hi, x.shape[0]))
            x[rows] = x[rows] + 2e-3 * nrm[rows] * torch.where(rows % 2 == 0, 1.0, -1.0)[:, None]
        kept.append(x.float())
        total += x.shape[0]
    return torch.cat(kept)[:n].contiguous()


@functools.lru_cache(maxsize=None)
def walk_truth(field: str, n: int, max_step: int = WALK_MAX_STEP):
    """The fp64 and the fp32 oracle walk of walk_starts(field, n), cached: final points, found, moves, margin, `decided`
    (margin >= WALK_MARGIN), the classes (found at step 0 / found later / never found), and per candidate the fp32 walk's deviation."""
    sd, spec = _field(field)
    start, cam_o = walk_starts(field, n), walk_camera_origin()
    p64, f64, m64, margin = walk(sd, spec, start, cam_o, max_step, torch.float64)
    p32, f32, m32, _ = walk(sd, spec, start, cam_o, max_step, torch.float32)
    decided = margin >= WALK_MARGIN
    cls = torch.where(f64 & (m64 == 0), 0, torch.where(f64, 1, 2))
    return SimpleNamespace(start=start, cam_o=cam_o, points=p64, found=f64, moves=m64, margin=margin, decided=decided, cls=cls,
                           points32=p32, found32=f32, moves32=m32, dev=(p32.double() - p64).abs().max(dim=1)[0])


def walk_floor(tr) -> float:
    """The point floor of a field: the fp32 oracle walk against the fp64 one over the decided candidates."""
    return float(tr.dev[tr.decided].max())


def tile_sorted_order(cls: torch.Tensor, n_cus: int, tile: int = 32) -> torch.Tensor:
    """A permutation of the candidates in which whole tiles of 32 are of class 0 (found at step 0: the tile leaves the loop after one
    evaluation) and other whole tiles of class 2 (never found: all max_step + 1 evaluations), alternating from tile to tile as long
    as both classes last; the tiles a workgroup takes on its second trip (tile index >= n_cus) are filled with the class opposite to
    that of the workgroup's first tile.  What is left over follows in its original order."""
    n = cls.shape[0]
    pools = {0: (cls == 0).nonzero().reshape(-1).tolist(), 2: (cls == 2).nonzero().reshape(-1).tolist()}
    n_tiles = (n + tile - 1) // tile
    order: List[List[int]] = [[] for _ in range(n_tiles)]
    want = lambda t: (0 if t % 2 == 0 else 2) if t < n_cus else (2 if (t - n_cus) % 2 == 0 else 0)
    for t in list(range(n_cus, n_tiles)) + list(range(min(n_cus, n_tiles))):       # the second-trip tiles get their pick first
        size = min(tile, n - t * tile)
        k = want(t)
        if len(pools[k]) >= size:
            order[t] = pools[k][:size]
            pools[k] = pools[k][size:]
    used = set(i for tl in order for i in tl)
    rest = [i for i in range(n) if i not in used]
    for t in range(n_tiles):
        if not order[t]:
            size = min(tile, n - t * tile)
            order[t], rest = rest[:size], rest[size:]
    perm = torch.tensor([i for tl in order for i in tl], dtype=torch.long)
    assert perm.shape[0] == n and int(torch.unique(perm).shape[0]) == n
    return perm


def walk_big_n(n_cus: int) -> int:
    return 32 * n_cus + 33
