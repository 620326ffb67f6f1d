"""fp64 oracle of the fused training backward of the hash-grid field (iron_amd/csrc/hashgrid_field_train.hip), built on
_hashgrid_oracle and _hashfield_oracle: for the adjoints d_out [n, n_out] and d_g [n, 3] of the fused evaluation's two results it
returns ybar and e [n, L F], every Wbar_l, d_table, and the first-order error scales of each.

    forward   y = enc(x);  z_l = W_l h_{l-1};  h_l = act(z_l);  out = z_m
    d chain   d_{m-1} = act'(z_{m-1}) W_m[0,:];  d_{l-1} = act'(z_{l-1}) (W_l^T d_l);  e = W_0^T d_0
    tangent   v'_d = a_d d_g[d] on live axes;  ydot = J v';  zdot_l = W_l hdot_{l-1};  hdot_l = act'(z_l) zdot_l
    curvature s_l = act''(z_l) G_l zdot_l,  G_l = W_{l+1}^T d_{l+1},  G_{m-1} = W_m[0,:]
    adjoint   delta_m = d_out;  delta_l = act'(z_l) (W_{l+1}^T delta_{l+1}) + s_l;  ybar = W_0^T delta_0
    weights   Wbar_l = sum_n delta_l h_{l-1}^T + d_l hdot_{l-1}^T   (d_m: the unit vector of row 0)
    table     O.backward(ybar) + O.backward_backward(e, v')

Error scales (|computed - oracle| <= eps32 (C S + F) to first order, one constant C per quantity).
  ybar and e, per point and entry, take §28's construction: every rounding goes through the SIGNED Jacobian of what follows it and
    only then into magnitude.  Both leave the head through the same per-point matrices U_l = d(.) / d(W_l^T q_l), V_l = U_l W_l^T,
    U_{l+1} = V_l diag(act'_l), with q = d for e and q = delta for ybar: a chain W_l^T q_l enters with |U_l| chain_bound(out_l)
    |W_l|^T |q_l|, an elementwise product with |V_l| |q_l| / 2, the evaluation of act' with |V_l| |its factor| (S, F of act'), and for
    ybar the curvature term s_l with |V_l| (S, F of s_l).
  What feeds those sites from outside the adjoint chain (act' through the scales of z_l, s_l through the tangent chain) and every
    operand of a weight gradient (delta, h, d, hdot) carries (value, S, F) forward as a running bound in magnitudes: W q adds
    chain_bound(k) |W| |q| to |W| S_q, a product half its magnitude to |a| S_b + |b| S_a, the activation and its first and second
    derivative pass the scales of z on with the magnitude of the next derivative and, for Softplus, add the library bounds of
    _hashfield_oracle to F (C_SP |h|; C_SPG sigma; C_SPG sigma + sigma (1 - sigma)).  A weight-gradient entry adds the scales of its
    per-point terms by the product rule and chain_bound(2 C(n)) times the sum of their magnitudes for the slot accumulation: signed
    per-point Jacobians of every entry of every Wbar_l ([n, out, in, sites]) do not fit a test of seconds.  Its bound is therefore the
    looser kind, and its constant is its own: twice what its own emulation shows, not the largest of the three.
The table's tolerance is §27's form with the pair scatter's unit, plus what the tolerances of ybar and e let through the scatter (the
scatter's inputs on the device are the kernel's ybar and e, not the oracle's)."""
from __future__ import annotations

import functools

import numpy as np

import _hashfield_oracle as H
import _hashgrid_oracle as O

EPS32 = O.EPS32
HEADS = [(16, 1), (32, 2), (64, 2), (64, 4)]

# Tolerance of the GPU tests: eps32 (C_TRAIN[quantity] S + F).  Each constant is twice the largest (|emulation - oracle| - eps32 F) /
# (eps32 S) that the fp32 emulation below shows for that quantity over every combination the pin test uses (case x head x
# activation): ybar 0.0906 (check_uniform, 16 x 1, ReLU), e 0.1242 (hashed_f8_nodes, 16 x 1, ReLU), Wbar 0.0271 (single_point, 32 x 2,
# None); tests/test_hashfield_train_oracle.py re-measures all three.
C_TRAIN_MEASURED_RATIO = {"ybar": 0.0906, "e": 0.1242, "Wbar": 0.0271}
C_TRAIN = {k: 2 * v for k, v in C_TRAIN_MEASURED_RATIO.items()}


def slot_points(n):
    """C(n) as the library defines it (iron_hashgrid_field_train_slot; the CPU test compares the two)"""
    return 64 * max(1, -(-n // (64 * 1024)))


# ---- (value, S, F) arithmetic ----
def _exact(v):
    v = np.asarray(v, np.float64)
    return v, np.zeros_like(v), np.zeros_like(v)


def _lin(q, W, k):
    """q [n, in] -> q W^T [n, out], a chain of k terms per output"""
    v, S, F = q
    A = np.abs(W).T
    return v @ W.T, S @ A + O.chain_bound(k) * (np.abs(v) @ A), F @ A


def _mul(a, b, rnd=0.5):
    v = a[0] * b[0]
    return v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + rnd * np.abs(v), np.abs(a[0]) * b[2] + np.abs(b[0]) * a[2]


def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + 0.5 * np.abs(v), a[2] + b[2]


def _acts(name, z):
    """h = act(z), act'(z), act''(z) as triples"""
    v, S, F = z
    a, q = H.dact(name, v), H.d2act(name, v)
    hv = H.act(name, v)
    if name != "Softplus":
        return (hv, a * S, a * F), _exact(a), _exact(q)
    q3 = np.abs(q * (1.0 - 2.0 * a))
    return ((hv, a * S, a * F + H.C_SP * np.abs(hv)), (a, q * S, q * F + H.C_SPG * a), (q, q3 * S, q3 * F + H.C_SPG * a + q))


def backward(cfg, x, table, weights, name, d_out, d_g, a3=(1.0, 1.0, 1.0), enc=None):
    """x: the mapped points (a p + b, fp32).  -> dict of triples ybar, e [n, L F], Wbar (list), and d_table with count / mag, vp"""
    e = enc if enc is not None else O.encode(cfg, x, table)
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    W = [np.asarray(w, np.float64) for w in weights]
    m = len(W) - 1
    a3 = np.asarray(a3, np.float64)
    live = ((x >= 0.0) & (x <= 1.0)).astype(np.float64)
    vpv = a3[None] * np.asarray(d_g, np.float64) * live
    vp = (vpv, (0.0 if (a3 == 1.0).all() else 0.5) * np.abs(vpv), np.zeros_like(vpv))
    hs, da, dq = [(e["y"], O.K * e["Sy"], np.zeros_like(e["y"]))], [], []
    for l in range(m):
        h, a, q = _acts(name, _lin(hs[l], W[l], W[l].shape[1]))
        hs.append(h)
        da.append(a)
        dq.append(q)
    d, c = [None] * (m + 1), [None] * m
    G = _exact(np.broadcast_to(W[m][0][None], (n, W[m].shape[1])))
    Gin, uin = [None] * m, [None] * m                 # what act'(z_l) multiplies in d_l and in delta_l
    for l in range(m - 1, -1, -1):
        Gin[l] = np.abs(G[0])
        d[l], c[l] = _mul(da[l], G), _mul(dq[l], G)
        G = _lin(d[l], W[l].T, W[l].shape[0])
    ev = G
    unit = np.zeros((n, W[m].shape[0]))
    unit[:, 0] = 1.0
    d[m] = _exact(unit)
    J, SJ = e["J"], O.K * e["SJ"]
    ydv = np.einsum("nkd,nd->nk", J, vpv)
    ydS = np.einsum("nkd,nd->nk", SJ, np.abs(vpv)) + np.einsum("nkd,nd->nk", np.abs(J), vp[1] + O.chain_bound(3) * np.abs(vpv))
    hd, s = [(ydv, ydS, np.zeros_like(ydv))], [None] * m
    for l in range(m):
        zd = _lin(hd[l], W[l], W[l].shape[1])
        hd.append(_mul(da[l], zd))
        s[l] = _mul(c[l], zd)
    delta = [None] * (m + 1)
    delta[m] = _exact(d_out)
    for l in range(m - 1, -1, -1):
        u = _lin(delta[l + 1], W[l + 1].T, W[l + 1].shape[0])
        uin[l] = np.abs(u[0])
        delta[l] = _add(_mul(da[l], u, rnd=0.0), s[l]) if name == "Softplus" else _mul(da[l], u)
    ybar = _lin(delta[0], W[0].T, W[0].shape[0])
    # e and ybar: the signed construction.  Both leave the head through the same per-point Jacobians,
    # U_l = d(.)/d(W_l^T q_l) and V_l = U_l W_l^T = d(.)/d q_l with q = d (for e) or delta (for ybar), U_{l+1} = V_l diag(act'_l).
    lf = W[0].shape[1]
    Se, Fe, Sy, Fy = (np.zeros((n, lf)) for _ in range(4))
    for c0 in range(0, n, H.CHUNK):
        k = slice(c0, min(c0 + H.CHUNK, n))
        U = np.broadcast_to(np.eye(lf, dtype=np.float32)[None], (k.stop - c0, lf, lf))
        for l in range(m + 1):
            Wl = W[l].astype(np.float32)
            aU = np.abs(U)
            cb = O.chain_bound(W[l].shape[0])
            Sy[k] += np.einsum("nik,nk->ni", aU, (cb * (np.abs(delta[l][0][k]) @ np.abs(W[l]))).astype(np.float32))
            if l == m:
                break
            Se[k] += np.einsum("nik,nk->ni", aU, (cb * (np.abs(d[l][0][k]) @ np.abs(W[l]))).astype(np.float32))
            aV = np.abs(U @ Wl.T)                       # [chunk, L F, out_l]
            Se[k] += np.einsum("nik,nk->ni", aV, (0.5 * np.abs(d[l][0][k]) + Gin[l][k] * da[l][1][k]).astype(np.float32))
            Fe[k] += np.einsum("nik,nk->ni", aV, (Gin[l][k] * da[l][2][k]).astype(np.float32))
            sS, sF = (s[l][1][k], s[l][2][k]) if name == "Softplus" else (0.0, 0.0)
            Sy[k] += np.einsum("nik,nk->ni", aV, (0.5 * np.abs(delta[l][0][k]) + uin[l][k] * da[l][1][k] + sS).astype(np.float32))
            Fy[k] += np.einsum("nik,nk->ni", aV, (uin[l][k] * da[l][2][k] + sF).astype(np.float32))
            U = (U @ Wl.T) * da[l][0][k][:, None, :].astype(np.float32)
    ybar, ev = (ybar[0], Sy, Fy), (ev[0], Se, Fe)
    acc = O.chain_bound(2 * slot_points(n))
    Wbar = []
    for l in range(m + 1):
        (dv, dS, dF), (hv, hS, hF), (gv, gS, gF), (tv, tS, tF) = delta[l], hs[l], d[l], hd[l]
        mag = np.abs(dv).T @ np.abs(hv) + np.abs(gv).T @ np.abs(tv)
        S = dS.T @ np.abs(hv) + np.abs(dv).T @ hS + gS.T @ np.abs(tv) + np.abs(gv).T @ tS + acc * mag
        Fn = dF.T @ np.abs(hv) + np.abs(dv).T @ hF + gF.T @ np.abs(tv) + np.abs(gv).T @ tF
        Wbar.append((dv.T @ hv + gv.T @ tv, S, Fn))
    return dict(ybar=ybar, e=ev, Wbar=Wbar, vp=vpv)


def tol(q, what):
    """eps32 (C_TRAIN[what] S + F) of a triple; what in ("ybar", "e", "Wbar")"""
    return EPS32 * (C_TRAIN[what] * q[1] + q[2])


def table_reference(cfg, x, table, ref):
    """d_table of the oracle's ybar, e and v', with count, mag (sum of the magnitudes of both orders) and `through`: what the
    tolerances of ybar and e let through the scatter (their magnitudes weighted as the contributions are)"""
    b1 = O.backward(cfg, x, table, ref["ybar"][0])
    b2 = O.backward_backward(cfg, x, table, ref["e"][0], ref["vp"])
    t1 = O.backward(cfg, x, table, tol(ref["ybar"], "ybar"))["mag"]
    t2 = O.backward_backward(cfg, x, table, tol(ref["e"], "e"), ref["vp"])["mag"]
    return dict(d_table=b1["d_table"] + b2["d_table"], count=b1["count"], mag=b1["mag"] + b2["mag"], through=t1 + t2)


# ---- fp32 emulation in the defined orders ----
def emulate(cfg, x, table, weights, name, d_out, d_g, a3=(1.0, 1.0, 1.0)):
    """-> ybar, e [n, L F] fp32 and the Wbar_l fp32, the slot cut of slot_points(n) and the fp64 slot sum included"""
    f32 = np.float32
    y, J = O.emulate_fp32(cfg, x, table)
    x = np.asarray(x, f32)
    n = x.shape[0]
    W = [np.asarray(w, f32) for w in weights]
    m = len(W) - 1
    hs = [y]
    for l in range(m):
        hs.append(H.act32(name, H._chain(hs[l], W[l].T.copy())).astype(f32))
    da = [H.dact32_from_h(name, hs[l + 1]).astype(f32) for l in range(m)]
    dq = [(a * (f32(1) - a)).astype(f32) if name == "Softplus" else np.zeros_like(a) for a in da]
    d, c = [None] * (m + 1), [None] * m
    G = np.broadcast_to(W[m][0][None], (n, W[m].shape[1]))
    for l in range(m - 1, -1, -1):
        d[l], c[l] = (da[l] * G).astype(f32), (dq[l] * G).astype(f32)
        G = H._chain(d[l], W[l])
    ev = G
    d[m] = np.zeros((n, W[m].shape[0]), f32)
    d[m][:, 0] = 1.0
    live = (x >= 0) & (x <= 1)
    vp = np.where(live, np.asarray(a3, f32)[None] * np.asarray(d_g, f32), f32(0)).astype(f32)
    yd = np.zeros_like(y)
    for dd in range(3):
        yd = O._fma32(J[:, :, dd], vp[:, dd:dd + 1], yd)
    hd, s = [yd], [None] * m
    for l in range(m):
        zd = H._chain(hd[l], W[l].T.copy())
        hd.append((da[l] * zd).astype(f32))
        s[l] = (c[l] * zd).astype(f32)
    delta = [None] * (m + 1)
    delta[m] = np.asarray(d_out, f32)
    for l in range(m - 1, -1, -1):
        u = H._chain(delta[l + 1], W[l + 1])
        delta[l] = O._fma32(da[l], u, s[l]) if name == "Softplus" else (da[l] * u).astype(f32)
    ybar = H._chain(delta[0], W[0])
    C = slot_points(n)
    Wbar = []
    for l in range(m + 1):
        total = np.zeros(W[l].shape, np.float64)
        for s0 in range(0, n, C):
            acc = np.zeros(W[l].shape, f32)
            for p0 in range(s0, min(s0 + C, n), 2):           # one MFMA takes two points: delta h^T of both, then d hdot^T of both
                pair = range(p0, min(p0 + 2, s0 + C, n))
                for p in pair:
                    acc = O._fma32(delta[l][p][:, None], hs[l][p][None, :], acc)
                for p in pair:
                    acc = O._fma32(d[l][p][:, None], hd[l][p][None, :], acc)
            total += acc.astype(np.float64)
        Wbar.append(total.astype(f32))
    return ybar, ev, Wbar


# ---- the combinations the tests share ----
def combos(acts=None):
    return [k for k in H.combos(acts) if k[1] in HEADS]


@functools.lru_cache(maxsize=None)
def case_adjoints(name, head, n_out, act_name):
    """d_out [n, n_out], d_g [n, 3] fp32 in +-1 under a fixed seed.  Rows of both are zero where a hidden pre-activation lies within
    its own tolerance of a ReLU kink (§28's mask); rows of d_g alone where the point lies within 4 ulp32 of a face.  -> also the count
    of zeroed rows."""
    ref = H.reference(name, head, n_out, act_name)
    n = ref["out"].shape[0]
    ci = [c[0] for c in O.CASES].index(name)
    rng = np.random.default_rng(7000 + 100 * ci + 10 * HEADS.index(head) + H.ACTS.index(act_name))
    d_out = (rng.random((n, n_out)) * 2 - 1).astype(np.float32)
    d_g = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    d_out[ref["kink"]] = 0.0
    d_g[ref["kink"] | ref["near"]] = 0.0
    return d_out, d_g, int(ref["kink"].sum()), int((ref["near"] & ~ref["kink"]).sum())


@functools.lru_cache(maxsize=None)
def reference(name, head, n_out, act_name):
    """The oracle's results of one combination (identity map); computed once, shared, left alone."""
    c, enc = H.case_encoding(name)
    d_out, d_g, _, _ = case_adjoints(name, head, n_out, act_name)
    return backward(c["cfg"], c["x"], c["table"], H.case_weights(name, head, n_out), act_name, d_out, d_g, enc=enc)
