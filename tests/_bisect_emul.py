"""The bisection as the tracer's two kernels split it, in plain torch (any device): every ray runs its OWN iterations and then
evaluates the mid-point it ends on, keeping that value; a ray whose chunk ran T > k iterations applies the update the kept
value decides and evaluates T - k more mid-points, the last of which is its result.  The reference (raytracer.py:199-220)
evaluates the same mid-points in the same order: T inside its loop and one after it."""
from __future__ import annotations

import torch


def point(o, d, mid):
    return o + d * mid.unsqueeze(-1)   # separate mul and add, as the reference's torch expression


def own_phase(sdf_fn, f_lo, f_hi, d_lo, d_hi, o, d, thr):
    """-> state dict: lo, hi, k (own count), mid, f (value at mid), p (point of mid)."""
    lo, hi = d_lo.clone(), d_hi.clone()
    work = (f_lo > 0) & (f_hi < 0)
    k = torch.zeros_like(lo, dtype=torch.int64)
    mid = (lo + hi) / 2.0
    while bool(work.any()):
        f = sdf_fn(point(o, d, mid))
        up = work & (f > 0)
        dn = work & ~(f > 0)
        lo = torch.where(up, mid, lo)
        hi = torch.where(dn, mid, hi)
        mid = (lo + hi) / 2.0
        k = k + work.long()
        work = work & ((hi - lo) > 2 * thr) & (k < 64)
    p = point(o, d, mid)
    return {"lo": lo, "hi": hi, "k": k, "mid": mid, "f": sdf_fn(p), "p": p}


def finish_phase(sdf_fn, st, o, d, total):
    """`total` [n] int64: the count every ray has to reach (its chunk's).  -> (p_mid, d_mid, f_mid)."""
    lo, hi, mid, f, p = st["lo"].clone(), st["hi"].clone(), st["mid"].clone(), st["f"].clone(), st["p"].clone()
    rem = total - st["k"]
    act = rem > 0
    # iteration k + 1 on the kept value
    lo = torch.where(act & (f > 0), mid, lo)
    hi = torch.where(act & ~(f > 0), mid, hi)
    mid = (lo + hi) / 2.0
    while bool(act.any()):
        q = point(o, d, mid)
        fq = sdf_fn(q)
        rem = rem - act.long()
        f = torch.where(act, fq, f)
        p = torch.where(act.unsqueeze(-1), q, p)
        cont = act & (rem > 0)
        lo = torch.where(cont & (fq > 0), mid, lo)
        hi = torch.where(cont & ~(fq > 0), mid, hi)
        mid = torch.where(cont, (lo + hi) / 2.0, mid)
        act = cont
    return p, mid, f


def chunk_totals(st, chunk_of, n_chunks):
    """The reference's per-chunk count: the largest own count among the chunk's rays ([n_chunks] int64)."""
    t = torch.zeros(n_chunks, dtype=torch.int64, device=st["k"].device)
    return t.scatter_reduce(0, chunk_of, st["k"], reduce="amax", include_self=True)
