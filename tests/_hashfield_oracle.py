"""fp64 oracle of the fused hash-grid field evaluation (iron_amd/csrc/hashgrid_field.hip), built on
_hashgrid_oracle.encode: the fp32 weights as given, the head carried in fp64, the input gradient in closed form, and the first-order
error scale S of both.  tests/test_hashfield_oracle.py pins it to a plain-torch fp64 restatement and measures the tolerance constant
with an fp32 emulation of the kernel's arithmetic; tests/test_gpu_hashfield.py compares the kernel with it.

Head: z_0 = W_0 y, h_l = act(z_l), z_{l+1} = W_{l+1} h_l, out = z_m (no activation after the last layer; no biases).
Gradient of out[0]: d_{m-1} = act'(z_{m-1}) W_m[0, :], G_l = W_l^T d_l, d_{l-1} = act'(z_{l-1}) G_l, e = G_0, grad_d = sum_k e_k J[k, d].

Error scale (|computed - oracle| <= C eps32 S to first order).  Every rounding error is carried to the result through the SIGNED
Jacobian of everything downstream of it and only then taken in magnitude:
    S_z[l] = sum_{j <= l} |dz_l / dz_j| loc_j + |dz_l / dy| K Sy,      F_z[l] = sum_{j < l} |dz_l / dh_j| C_SP |h_j| (Softplus only),
    loc_j = chain_bound(in_j) (|W_j| |h_{j-1}|): the layer's own fma chain.  S and F of the output are those of z_m.  S collects the
    fma chains, whose bound the measured constant C_HEAD scales; F collects the evaluations of Softplus and its derivative, whose
    constants are the library's own bounds and are not scaled: the tolerance is eps32 (C_HEAD S + F).
The gradient's scale walks the backward chain the same way (U_l = d grad / d G_l, V_l = d grad / d d_l):
    S_g = chain_bound(L F) |e| |J| + |e| K SJ + sum_l |U_l| chain_bound(out_l) (|W_l|^T |d_l|) + |V_l| (|d_l| / 2 + |next| d_act'_l)
with, for Softplus only, d_act'_l = C_SPG |act'_l| (into F) + |act''_l| (S_z[l] into S, F_z[l] into F): the derivative is evaluated
at the computed z_l."""
from __future__ import annotations

import functools

import numpy as np
import torch

import _hashgrid_oracle as O

EPS32 = O.EPS32
HEADS = [(16, 1), (32, 2), (64, 2), (128, 3), (64, 4)]        # (n_neurons, n_hidden_layers)
N_OUTS = (1, 3, 16)
ACTS = ("ReLU", "Softplus", "None")

# Softplus is log1pf(expf(z)) below the threshold: expf within 1 ulp and log1pf within 2 (the device library's published bounds), and
# an error of exp(z) reaches log1p with a factor e^z / ((1 + e^z) log1p(e^z)) <= 1, so |error| <= 3 ulp <= 3 eps32 |h|; C_SP = 4
# leaves one for the threshold's own step (2e-9 at z = 20).  The derivative is -expm1f(-h) of the computed h: h's relative error
# passes with a factor h e^-h / (1 - e^-h) <= 1 and expm1f adds 2 ulp, so C_SPG = C_SP + 2.  test_hashfield_oracle.py checks both
# against the fp32 expressions.
C_SP = 4.0
C_SPG = C_SP + 2.0

# Tolerance of the GPU tests: |gpu - oracle| <= eps32 (C_HEAD S + F).  C_HEAD is twice the largest (|emulation - oracle| - eps32 F) /
# (eps32 S) over every case of _hashgrid_oracle.CASES and every head above (values, and gradients away from kinks and faces;
# measured 0.0873, on a value of hashed_tiny_table with the 16 x 1 head and no activation; the gradients' largest is 0.0734);
# test_hashfield_oracle.py re-measures it.
C_MEASURED_RATIO = 0.0873
C_HEAD = 2 * C_MEASURED_RATIO

CHUNK = 256      # points per batch of per-point Jacobians

# A (case, head) whose first seed broke the near-kink cap (at most max(2 points, 1 % of n) with a hidden pre-activation within its own
# tolerance of zero) takes another seed; the cap is not widened.  check_uniform with 128 x 3: 46 of 4099 points, 34 with this one
# (384 ReLU neurons per point put the share near 1 % whatever the seed: 34 .. 45 over six seeds).
RESEEDED = {("check_uniform", (128, 3)): 1000}


def head_dims(lf, neurons, hidden, n_out):
    return [lf] + [neurons] * hidden + [n_out]


def head_weights(lf, neurons, hidden, n_out, seed=0):
    """fp32 [out, in] matrices of nn.Linear's default initialisation under a fixed seed (the global generator is left alone)"""
    dims = head_dims(lf, neurons, hidden, n_out)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234 + seed)
        return [torch.nn.Linear(dims[i], dims[i + 1], bias=False).weight.detach().numpy().copy() for i in range(len(dims) - 1)]


def act(name, z):
    if name == "ReLU":
        return np.maximum(z, 0.0)
    if name == "Softplus":
        return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))
    return z


def dact(name, z):
    if name == "ReLU":
        return (z > 0.0).astype(np.float64)
    if name == "Softplus":
        return np.where(z > 20.0, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(z, 20.0))))
    return np.ones_like(z)


def d2act(name, z):
    if name == "Softplus":
        s = 1.0 / (1.0 + np.exp(-np.minimum(z, 20.0)))
        return np.where(z > 20.0, 0.0, s * (1.0 - s))
    return np.zeros_like(z)


def _scale_of_z(l, W, hs, da, locs, ksy, name):
    """(S_z[l], F_z[l]) [n, out_l]: every earlier rounding (S) and Softplus evaluation (F) carried through the signed Jacobian
    dz_l / d(.) of its point.  The Jacobians are sensitivity weights and are carried in fp32."""
    n = hs[0].shape[0]
    S, Fn = locs[l].copy(), np.zeros_like(locs[l])
    W32 = [w.astype(np.float32) for w in W]
    for c0 in range(0, n, CHUNK):
        c = slice(c0, min(c0 + CHUNK, n))
        R = np.broadcast_to(W32[l][None], (c.stop - c0,) + W[l].shape)           # dz_l / dh_{l-1}  (dz_0 / dy)
        for j in range(l - 1, -1, -1):
            if name == "Softplus":
                Fn[c] += np.einsum("nok,nk->no", np.abs(R), (C_SP * np.abs(hs[j + 1][c])).astype(np.float32))
            T = R * da[j][c][:, None, :].astype(np.float32)                        # dz_l / dz_j
            S[c] += np.einsum("nok,nk->no", np.abs(T), locs[j][c].astype(np.float32))
            R = T @ W32[j]                                                         # dz_l / dh_{j-1}
        S[c] += np.einsum("nok,nk->no", np.abs(R), ksy[c].astype(np.float32))
    return S, Fn


def evaluate(cfg, x, table, weights, name, gradient=True, enc=None):
    """-> dict out [n, n_out] with S_out, F_out; z (hidden pre-activations); with gradient: S_z, F_z (their scales), grad [n, 3]
    with S_grad, F_grad; near [n] (a level of the point lies within 4 ulp32 of a face), kink [n] (ReLU: a hidden pre-activation
    within its tolerance of zero).  The tolerance of a quantity is eps32 (C_HEAD S + F): tol()."""
    e = enc if enc is not None else O.encode(cfg, x, table)
    W = [np.asarray(w, np.float64) for w in weights]
    m = len(W) - 1
    hs, zs, da = [e["y"]], [], []
    for l in range(m + 1):
        z = hs[l] @ W[l].T
        zs.append(z)
        if l < m:
            hs.append(act(name, z))
            da.append(dact(name, z))
    locs = [O.chain_bound(W[l].shape[1]) * (np.abs(hs[l]) @ np.abs(W[l]).T) for l in range(m + 1)]
    ksy = O.K * e["Sy"]
    res = dict(out=zs[m], z=zs[:m], near=e["near"].any(axis=1))
    res["S_out"], res["F_out"] = _scale_of_z(m, W, hs, da, locs, ksy, name)
    if not gradient:
        return res
    if name == "None":                                                              # neither a kink nor a curvature term
        Sz = [(None, None)] * m
    else:
        Sz = [_scale_of_z(l, W, hs, da, locs, ksy, name) for l in range(m)]
    res["S_z"], res["F_z"] = [s for s, _ in Sz], [f for _, f in Sz]
    kink = np.zeros(x.shape[0], bool)
    if name == "ReLU":
        for l in range(m):
            kink |= (np.abs(zs[l]) <= EPS32 * (C_HEAD * Sz[l][0] + Sz[l][1])).any(axis=1)
    res["kink"] = kink
    # backward chain
    w0 = W[m][0]
    d = [None] * m
    G = [None] * m
    d[m - 1] = da[m - 1] * w0[None]
    for l in range(m - 1, -1, -1):
        G[l] = d[l] @ W[l]
        if l > 0:
            d[l - 1] = da[l - 1] * G[l]
    J, ev = e["J"], G[0]
    res["grad"] = np.einsum("nk,nkd->nd", ev, J)
    lf = W[0].shape[1]
    S = O.chain_bound(lf) * np.einsum("nk,nkd->nd", np.abs(ev), np.abs(J)) + np.einsum("nk,nkd->nd", np.abs(ev), O.K * e["SJ"])
    Fn = np.zeros_like(S)
    U = np.transpose(J, (0, 2, 1))                                                  # d grad / d G_0  [n, 3, L F]
    for l in range(m):
        S += np.einsum("ndk,nk->nd", np.abs(U), O.chain_bound(W[l].shape[0]) * (np.abs(d[l]) @ np.abs(W[l])))
        V = U @ W[l].T                                                              # d grad / d d_l  [n, 3, out_l]
        nxt = np.abs(G[l + 1]) if l < m - 1 else np.broadcast_to(np.abs(w0)[None], d[l].shape)
        derr = 0.5 * np.abs(d[l])
        if name == "Softplus":
            curv = np.abs(d2act(name, zs[l]))
            derr = derr + nxt * curv * Sz[l][0]
            Fn += np.einsum("ndk,nk->nd", np.abs(V), nxt * (C_SPG * np.abs(da[l]) + curv * Sz[l][1]))
        S += np.einsum("ndk,nk->nd", np.abs(V), derr)
        U = V * da[l][:, None, :]
    res["S_grad"], res["F_grad"] = S, Fn
    return res


def tol(ref, what):
    """the GPU tests' tolerance of `what` in ("out", "grad")"""
    return EPS32 * (C_HEAD * ref["S_" + what] + ref["F_" + what])


# ---- fp32 emulation of the kernel's arithmetic: emulate_fp32 for the features, one _fma32 chain in ascending k per product ----
def _chain(A, Wt):
    """[n, K] fp32 times Wt [K, M] fp32 -> [n, M]: acc = fma32(A[:, k], Wt[k, :], acc), k ascending from zero"""
    acc = np.zeros((A.shape[0], Wt.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = O._fma32(A[:, k:k + 1], Wt[k:k + 1, :], acc)
    return acc


def act32(name, z):
    if name == "ReLU":
        return np.maximum(z, np.float32(0))
    if name == "Softplus":
        with np.errstate(over="ignore"):
            return np.where(z > np.float32(20), z, np.log1p(np.exp(z, dtype=np.float32), dtype=np.float32)).astype(np.float32)
    return z


def dact32_from_h(name, h):
    """act'(z) as the kernel recovers it from h = act(z)"""
    if name == "ReLU":
        return (h > 0).astype(np.float32)
    if name == "Softplus":
        return (-np.expm1(-h, dtype=np.float32)).astype(np.float32)
    return np.ones_like(h)


def emulate_head(cfg, x, table, weights, name, gradient=True):
    y, J = O.emulate_fp32(cfg, x, table)
    W = [np.asarray(w, np.float32) for w in weights]
    m = len(W) - 1
    hs = [y]
    for l in range(m):
        hs.append(act32(name, _chain(hs[l], W[l].T.copy())))
    out = _chain(hs[m], W[m].T.copy())
    if not gradient:
        return out, None
    d = dact32_from_h(name, hs[m]) * W[m][0][None]
    for l in range(m - 1, 0, -1):
        d = dact32_from_h(name, hs[l]) * _chain(d, W[l])
    ev = _chain(d, W[0])
    g = np.zeros((x.shape[0], 3), np.float32)
    for k in range(ev.shape[1]):
        for dd in range(3):
            g[:, dd] = O._fma32(ev[:, k], J[:, k, dd], g[:, dd])
    return out, g


# ---- the combinations the tests share: every (case, head); n_out and the activation rotate so that each value meets each case ----
def combos(acts=None):
    out = []
    for ci, case in enumerate(O.CASES):
        for hi, head in enumerate(HEADS):
            for ai, a in enumerate(ACTS):
                if acts is None or a in acts:
                    out.append((case[0], head, N_OUTS[(ci + hi + ai) % 3], a))
    return out


@functools.lru_cache(maxsize=None)
def case_encoding(name):
    c = O.case_inputs(name)
    return c, O.encode(c["cfg"], c["x"], c["table"])


def case_weights(name, head, n_out):
    cfg = O.case_inputs(name)["cfg"]
    ci = [c[0] for c in O.CASES].index(name)
    return head_weights(cfg[0] * cfg[1], head[0], head[1], n_out,
                        seed=100 * ci + 10 * HEADS.index(head) + n_out + RESEEDED.get((name, head), 0))


@functools.lru_cache(maxsize=None)
def reference(name, head, n_out, act_name, gradient=True):
    """The oracle's results of one combination; computed once, shared, left alone."""
    c, enc = case_encoding(name)
    return evaluate(c["cfg"], c["x"], c["table"], case_weights(name, head, n_out), act_name, gradient=gradient, enc=enc)
