"""fp64 oracle of the multiresolution hash-grid encoding, written from the definition in DESIGN.md "Hash-grid encoding" (tiny-cuda-nn's
published HashGrid with Linear interpolation), a plain-torch restatement of the same definition, and the fp32 emulation of the
kernel's arithmetic.  tests/test_hashgrid_oracle.py pins the three to each other and to finite differences on the CPU; the GPU
tests compare csrc/hashgrid.hip and csrc/hashgrid_train.hip with the oracle on the inputs of CASES.

Level l of cfg = (L, F, log2T, N, b): scale = fp32(exp2(l log2 b) N - 1), res = ceil(scale) + 1, size = min(roundup8(res^3), 2^log2T),
dense iff res^3 <= size.  x is clamped to [0, 1]; pos = x scale + 0.5, cell = floor(pos), w = pos - cell; corner o = o0 + 2 o1 + 4 o2
at cell + o with weight prod (o_d ? w_d : 1 - w_d); index (c0 + c1 res + c2 res^2) mod size on a dense level, (c0 ^ c1 2654435761 ^
c2 805459861) mod size in uint32 arithmetic on a hashed one."""
from __future__ import annotations

import math

import numpy as np
import torch

P1, P2, M32 = 2654435761, 805459861, 0xFFFFFFFF
EPS32 = float(np.finfo(np.float32).eps)   # 2^-23


def levels_of(cfg):
    L, F, log2T, N, b = cfg
    out, off = [], 0
    for l in range(L):
        scale = float(np.float32(2.0 ** (l * math.log2(b)) * N - 1.0))
        res = int(math.ceil(scale)) + 1
        size = min((res ** 3 + 7) // 8 * 8, 1 << log2T)
        out.append(dict(scale=scale, res=res, size=size, offset=off, dense=res ** 3 <= size))
        off += size
    return out, off


def _index(lv, c0, c1, c2, xp=np):
    """entry index of integer corner coordinates (int64 arrays / tensors holding uint32 values)"""
    if lv["dense"]:
        i = (c0 + c1 * lv["res"] + c2 * (lv["res"] * lv["res"])) & M32
    else:
        i = c0 ^ ((c1 * P1) & M32) ^ ((c2 * P2) & M32)
    return i % lv["size"]


def near_face(lv, x):
    """[n, 3] bool: the axis' pos lies within 4 ulp32 of a cell face"""
    pos = np.clip(x, 0.0, 1.0) * lv["scale"] + 0.5
    return np.abs(pos - np.rint(pos)) <= 4.0 * np.spacing(pos.astype(np.float32)).astype(np.float64)


def corner_walk(lv, x, side=None):
    """x float64 [n,3] -> idx [n,8] (within the level), wgt [n,8], dw [n,8,3] (d wgt / d w_d), live [n,3].
    side (0..7, optional): on an axis within 4 ulp32 of a face, take the cell below (bit d clear) or above (bit d set) the face."""
    xc = np.clip(x, 0.0, 1.0)
    live = ((x >= 0.0) & (x <= 1.0)).astype(np.float64)
    pos = xc * lv["scale"] + 0.5
    cell = np.floor(pos)
    if side is not None:
        nf = near_face(lv, x)
        r = np.rint(pos)
        for d in range(3):
            alt = r[:, d] - (0.0 if (side >> d) & 1 else 1.0)
            cell[:, d] = np.where(nf[:, d] & (alt >= 0), alt, cell[:, d])
    w = pos - cell
    c = cell.astype(np.int64)
    n = x.shape[0]
    idx = np.empty((n, 8), np.int64)
    wgt = np.empty((n, 8))
    dw = np.empty((n, 8, 3))
    for o in range(8):
        ob = [(o >> d) & 1 for d in range(3)]
        a = [w[:, d] if ob[d] else 1.0 - w[:, d] for d in range(3)]
        sg = [1.0 if ob[d] else -1.0 for d in range(3)]
        idx[:, o] = _index(lv, c[:, 0] + ob[0], c[:, 1] + ob[1], c[:, 2] + ob[2])
        wgt[:, o] = a[0] * a[1] * a[2]
        dw[:, o, 0], dw[:, o, 1], dw[:, o, 2] = sg[0] * a[1] * a[2], sg[1] * a[0] * a[2], sg[2] * a[0] * a[1]
    return idx, wgt, dw, live


def encode(cfg, x, table, side=None):
    """-> dict y [n, L F], J [n, L F, 3], Sy, SJ (sums of term magnitudes), near [n, L] (a face within 4 ulp32 on some axis)"""
    L, F = cfg[0], cfg[1]
    levels, _ = levels_of(cfg)
    x = np.asarray(x, np.float64)
    table = np.asarray(table, np.float64).reshape(-1, F)
    n = x.shape[0]
    y, Sy = np.zeros((n, L * F)), np.zeros((n, L * F))
    J, SJ = np.zeros((n, L * F, 3)), np.zeros((n, L * F, 3))
    near = np.zeros((n, L), bool)
    for l, lv in enumerate(levels):
        idx, wgt, dw, live = corner_walk(lv, x, side)
        rows = table[lv["offset"] + idx]                                   # [n, 8, F]
        sl = slice(l * F, (l + 1) * F)
        y[:, sl] = np.einsum("no,nof->nf", wgt, rows)
        Sy[:, sl] = np.einsum("no,nof->nf", np.abs(wgt), np.abs(rows))
        J[:, sl] = lv["scale"] * live[:, None, :] * np.einsum("nod,nof->nfd", dw, rows)
        SJ[:, sl] = lv["scale"] * live[:, None, :] * np.einsum("nod,nof->nfd", np.abs(dw), np.abs(rows))
        near[:, l] = near_face(lv, x).any(axis=1)
    return dict(y=y, J=J, Sy=Sy, SJ=SJ, near=near)


def backward(cfg, x, table, dy):
    """-> d_table [P, F], count [P] (contributions an entry receives), mag [P, F] (sum of their magnitudes), d_x [n,3], S_dx"""
    L, F = cfg[0], cfg[1]
    levels, P = levels_of(cfg)
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    d_table, mag, count = np.zeros((P, F)), np.zeros((P, F)), np.zeros(P, np.int64)
    for l, lv in enumerate(levels):
        idx, wgt, _, _ = corner_walk(lv, x)
        t = wgt[:, :, None] * dy[:, None, l * F:(l + 1) * F]               # [n, 8, F]
        np.add.at(d_table, lv["offset"] + idx, t)
        np.add.at(mag, lv["offset"] + idx, np.abs(t))
        np.add.at(count, lv["offset"] + idx, 1)
    e = encode(cfg, x, table)
    return dict(d_table=d_table, count=count, mag=mag, d_x=np.einsum("nk,nkd->nd", dy, e["J"]),
                S_dx=np.einsum("nk,nkd->nd", np.abs(dy), e["SJ"]))


def backward_backward(cfg, x, table, dy, g):
    """g [n,3] arriving at d_x -> d_dy [n, L F], S_ddy, d_table [P, F], count, mag, bound [L] (per-contribution bound as the kernel
    forms it: fp32 ((3 max|g|) scale) max|dy|)"""
    L, F = cfg[0], cfg[1]
    levels, P = levels_of(cfg)
    x, dy, g = np.asarray(x, np.float64), np.asarray(dy, np.float64), np.asarray(g, np.float64)
    e = encode(cfg, x, table)
    d_table, mag, count = np.zeros((P, F)), np.zeros((P, F)), np.zeros(P, np.int64)
    for l, lv in enumerate(levels):
        idx, _, dw, live = corner_walk(lv, x)
        coef = np.einsum("nod,nd->no", dw, g * live * lv["scale"])
        cmag = np.einsum("nod,nd->no", np.abs(dw), np.abs(g) * live * lv["scale"])
        np.add.at(d_table, lv["offset"] + idx, coef[:, :, None] * dy[:, None, l * F:(l + 1) * F])
        np.add.at(mag, lv["offset"] + idx, cmag[:, :, None] * np.abs(dy[:, None, l * F:(l + 1) * F]))
        np.add.at(count, lv["offset"] + idx, 1)
    mg, md = np.float32(np.abs(g).max()), np.float32(np.abs(dy).max())
    bound = [float((np.float32(3.0) * mg) * np.float32(lv["scale"]) * md) for lv in levels]
    return dict(d_dy=np.einsum("nkd,nd->nk", e["J"], g), S_ddy=np.einsum("nkd,nd->nk", e["SJ"], np.abs(g)), d_table=d_table, count=count,
                mag=mag, bound=bound)


def level_of_entry(cfg):
    """[P] level index of every table entry"""
    levels, P = levels_of(cfg)
    out = np.empty(P, np.int64)
    for l, lv in enumerate(levels):
        out[lv["offset"]:lv["offset"] + lv["size"]] = l
    return out


# ---- the same definition in plain torch (differentiable; any dtype / device) ----
def restate(cfg, x, table):
    L, F = cfg[0], cfg[1]
    levels, _ = levels_of(cfg)
    table = table.reshape(-1, F)
    xc = x.clamp(0.0, 1.0)
    outs = []
    for lv in levels:
        pos = xc * lv["scale"] + 0.5
        cell = torch.floor(pos).detach()
        w = pos - cell
        c = cell.to(torch.int64)
        acc = 0
        for o in range(8):
            ob = [(o >> d) & 1 for d in range(3)]
            wt = 1
            for d in range(3):
                wt = wt * (w[:, d] if ob[d] else 1.0 - w[:, d])
            idx = _index(lv, c[:, 0] + ob[0], c[:, 1] + ob[1], c[:, 2] + ob[2], xp=torch)
            acc = acc + wt[:, None] * table[lv["offset"] + idx]
        outs.append(acc)
    return torch.cat(outs, dim=1)


# ---- fp32 emulation of the kernel's arithmetic (csrc/hashgrid_common.h: locate / walk; hashgrid.hip: the corner sums) ----
def _f32(a):
    return np.asarray(a, np.float32)


def _fma32(a, b, c):
    """fl32(a b + c): the product of two fp32 values is exact in fp64; the sum is rounded twice (fp64, then fp32), which differs
    from a true fma in rare last-bit cases only"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_fp32(cfg, x, table, fused=True):
    """-> y32 [n, L F], J32 [n, L F, 3].  fused=False takes the fraction as pos - floor(pos) from the rounded fp32 pos (the form the
    kernel must NOT use)."""
    L, F = cfg[0], cfg[1]
    levels, _ = levels_of(cfg)
    x = _f32(x)
    table = _f32(table).reshape(-1, F)
    n = x.shape[0]
    y, J = np.zeros((n, L * F), np.float32), np.zeros((n, L * F, 3), np.float32)
    one, half = np.float32(1.0), np.float32(0.5)
    for l, lv in enumerate(levels):
        s = np.full((n, 3), lv["scale"], np.float32)
        live = ((x >= 0) & (x <= 1)).astype(np.float32)
        xc = np.minimum(np.maximum(x, np.float32(0)), one)
        pos = _fma32(xc, s, np.full_like(xc, half))
        cell = np.floor(pos)
        if fused:
            w = _fma32(xc, s, half - cell)
            low = w < 0
            cell = np.where(low, cell - one, cell)
            w = np.where(low, _fma32(xc, s, half - cell), w)
            u = _fma32(-xc, s, cell + half)
        else:
            w = pos - cell
            u = one - w
        c = cell.astype(np.int64)
        rows, wgt, dw = [], [], []
        for o in range(8):
            ob = [(o >> d) & 1 for d in range(3)]
            a = [w[:, d] if ob[d] else u[:, d] for d in range(3)]
            rows.append(table[lv["offset"] + _index(lv, c[:, 0] + ob[0], c[:, 1] + ob[1], c[:, 2] + ob[2])])
            wgt.append((a[0] * a[1]) * a[2])
            dw.append([a[1] * a[2] if ob[0] else -(a[1] * a[2]), a[0] * a[2] if ob[1] else -(a[0] * a[2]),
                       a[0] * a[1] if ob[2] else -(a[0] * a[1])])
        for f in range(F):
            acc = np.zeros(n, np.float32)
            for o in range(8):
                acc = _fma32(wgt[o], rows[o][:, f], acc)
            y[:, l * F + f] = acc
            for d in range(3):
                acc = np.zeros(n, np.float32)
                for o in range(8):
                    acc = _fma32(dw[o][d], rows[o][:, f], acc)
                J[:, l * F + f, d] = live[:, d] * (np.float32(lv["scale"]) * acc)
    return y, J


# ---- the inputs the GPU tests and the emulation share ----
CHECK_CFG = (16, 2, 19, 16, 1.3819)
# (name, cfg = (L, F, log2T, N, b), n, point set)
CASES = [
    ("check_uniform", CHECK_CFG, 4099, "uniform"),
    ("check_mixed", CHECK_CFG, 257, "mixed"),
    ("hashed_tiny_table", (2, 1, 4, 16, 2.0), 4099, "uniform"),     # log2T = 4: every level hashed, every entry hit thousands of times
    ("one_level_f4", (1, 4, 14, 16, 1.0), 65, "uniform"),
    ("equal_levels_f8", (2, 8, 14, 2, 1.0), 63, "mixed"),           # b = 1: identical levels
    ("steep_f4", (16, 4, 14, 16, 2.0), 64, "mixed"),
    ("single_point", (1, 2, 19, 16, 1.3819), 1, "uniform"),
    ("hashed_f8_nodes", (2, 8, 4, 16, 1.3819), 257, "mixed"),
]


def case_inputs(name):
    """-> dict cfg, x [n,3] fp32, table [P,F] fp32 in +-0.1, dy [n, L F] fp32 in +-1, g [n,3] fp32 in +-1; the same arrays every time.
    'mixed': grid nodes of a random level, exact 0 and 1, -0.25 and 1.5 (clamped), the rest uniform."""
    k = [c[0] for c in CASES].index(name)
    _, cfg, n, kind = CASES[k]
    L, F = cfg[0], cfg[1]
    levels, P = levels_of(cfg)
    rng = np.random.default_rng(1000 + k)
    x = rng.random((n, 3)).astype(np.float32)
    if kind == "mixed":
        q = n // 4
        lv = [levels[i] for i in rng.integers(0, L, q)]
        sc = np.array([v["scale"] for v in lv], np.float64)[:, None]
        node = rng.integers(0, np.array([v["res"] for v in lv])[:, None], (q, 3))
        x[:q] = np.clip((node + 0.5) / np.maximum(sc, 1.0), 0.0, 1.0).astype(np.float32)         # pos on an integer: a node of the level
        x[q:2 * q] = x[:q]
        x[q:2 * q, rng.integers(0, 3)] = rng.random(q).astype(np.float32)                        # on a face / an edge only
        e = rng.integers(0, 4, (n - 2 * q - q, 3))
        x[2 * q:n - q] = np.array([0.0, 1.0, -0.25, 1.5], np.float32)[e]
    table = (rng.random((P, F)) * 0.2 - 0.1).astype(np.float32)
    dy = (rng.random((n, L * F)) * 2 - 1).astype(np.float32)
    g = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    return dict(cfg=cfg, x=x, table=table, dy=dy, g=g)


# Tolerance constant of the GPU tests: |gpu - oracle64| <= K eps32 S per entry, S the oracle's sum of term magnitudes.  K is twice the
# largest ratio |emulate_fp32 - oracle| / (eps32 S) over every case above (features and Jacobian; measured 2.65, on a feature of
# check_uniform; the Jacobian's largest is 2.45); tests/test_hashgrid_oracle.py re-measures it.  eps32 = 2^-23.
K_MEASURED_RATIO = 2.65
K = 2 * K_MEASURED_RATIO


def chain_bound(m):
    """c such that a fixed-order fp32 chain of m fused multiply-adds errs by at most c eps32 S (S the sum of term magnitudes), from
    the number format alone, for the per-point sums that have no emulation (d_x, d_dy): with u = 2^-24 = eps32 / 2, every term
    carries at most 8 roundings in its factors (w or u: 1 each; their product: 1; dy scale, times the product: 2; or g live scale
    and the three-term coefficient: 2 + 3) and the chain adds one rounding per step, so |error| <= (m + 8) u S to first order."""
    return (m + 8) / 2.0
