"""fp64 restatement of the environment render (csrc/envlight.hip), in torch and device-agnostic: CPU for the CPU
tests, the GPU for the larger checks.  Test infrastructure: never uses the HIP library.

No Mitsuba render exists to pin the feature to, so it is pinned to this restatement and to closed forms.  `dtype=torch.float32`
runs the same formulas in fp32: the measure of what fp32 can give, from which the GPU tests take their bounds.  The random numbers
are restated in integers (numpy uint32) and reproduce the kernel's bit for bit.
"""
from __future__ import annotations

import math

import numpy as np
import torch

ETA = 1.48958738
INF = float("inf")


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(a):
    return a / a.norm(dim=-1, keepdim=True)


# ---- the environment map ----
def dir_to_uv(d):
    """Mitsuba 0.6's lat-long convention for a local unit direction: u = atan2(d.x, -d.z) / 2 pi wrapped to [0, 1), v = acos(d.y) / pi."""
    u = torch.atan2(d[..., 0], -d[..., 2]) / (2 * math.pi)
    u = torch.where(u < 0, u + 1, u)
    return u, torch.acos(d[..., 1].clamp(-1, 1)) / math.pi


def uv_to_dir(u, v):
    phi, theta = 2 * math.pi * u, math.pi * v
    st = torch.sin(theta)
    return torch.stack([st * torch.sin(phi), torch.cos(theta), -st * torch.cos(phi)], -1)


class EnvOracle:
    """image [He, We, 3]; texel weight luminance sin(pi (row + 1/2) / He); CDFs in fp64, used in `dtype`."""

    def __init__(self, image, to_world=None, dtype=torch.float64):
        img = torch.as_tensor(image).double()
        self.dev, self.dtype = img.device, dtype
        self.He, self.We = int(img.shape[0]), int(img.shape[1])
        self.image = img
        self.R = (torch.eye(3, dtype=torch.float64) if to_world is None else torch.as_tensor(to_world).double()).to(self.dev)
        lum = (0.2126 * img[..., 0] + 0.7152 * img[..., 1]) + 0.0722 * img[..., 2]
        rows = torch.arange(self.He, dtype=torch.float64, device=self.dev)
        self.weight = lum * torch.sin(math.pi * (rows + 0.5) / self.He)[:, None]
        rowsum = self.weight.sum(1)
        self.total = float(rowsum.sum())
        z = torch.zeros((self.He, 1), dtype=torch.float64, device=self.dev)
        safe = torch.where(rowsum > 0, rowsum, torch.ones_like(rowsum))
        self.rowcdf = torch.cat([z, torch.cumsum(self.weight, 1) / safe[:, None]], 1)
        self.rowcdf[:, -1] = 1.0
        self.rowcdf[rowsum <= 0] = 0.0
        tot = self.total if self.total > 0 else 1.0
        self.mcdf = torch.cat([z[:1, 0], torch.cumsum(rowsum, 0) / tot])
        self.mcdf[-1] = 1.0 if self.total > 0 else 0.0
        self.P = self.weight / tot if self.total > 0 else torch.zeros_like(self.weight)

    def _density(self, r, c, sin_theta):
        p = self.P[r, c].to(self.dtype)
        return torch.where(p > 0, p * (self.We * self.He) / (2 * math.pi ** 2 * sin_theta), torch.zeros_like(p))

    @staticmethod
    def _find(cdf, u):
        """per row of cdf [n, K + 1] the number of entries cdf[1 ..] that are <= u, clamped to K - 1"""
        return (cdf[:, 1:] <= u[:, None]).sum(1).clamp(max=cdf.shape[1] - 2)

    def sample(self, u):
        """u [n, 2] -> (texel [n, 2], dir [n, 3] world, pdf [n]) in self.dtype; also self.boundary_gap [n]: the distance of u to
        the nearest CDF boundary it was compared with, in fp32 ulps of that u (fp64), for the texel-flip allowance."""
        u = torch.as_tensor(u).to(self.dev).double()
        n = u.shape[0]
        if not self.total > 0:
            r = c = torch.zeros(n, dtype=torch.long, device=self.dev)
            dv = du = torch.full((n,), 0.5, dtype=self.dtype, device=self.dev)
            self.boundary_gap = torch.full((n,), INF, dtype=torch.float64, device=self.dev)
        else:
            m = self.mcdf[None].expand(n, -1)
            r = self._find(m, u[:, 1])
            rows = self.rowcdf[r]
            c = self._find(rows, u[:, 0])

            def remap(cdf, k, x):
                lo, hi = cdf.gather(1, k[:, None])[:, 0], cdf.gather(1, k[:, None] + 1)[:, 0]
                f = ((x - lo) / (hi - lo)).to(self.dtype)
                return f.clamp(0.0, 0.99999994)
            dv, du = remap(m, r, u[:, 1]), remap(rows, c, u[:, 0])
            self.boundary_gap = torch.minimum((m - u[:, 1:2]).abs().min(1).values / ulps(u[:, 1], 1),
                                              (rows - u[:, 0:1]).abs().min(1).values / ulps(u[:, 0], 1))
        uu = (c.to(self.dtype) + du) / self.We
        vv = (r.to(self.dtype) + dv) / self.He
        local = uv_to_dir(uu, vv)
        world = local @ self.R.to(self.dtype).T
        to_south = ((self.He - 1 - r).to(self.dtype) + (1.0 - dv)) / self.He  # the kernel's form: sin(theta) through the nearer pole
        pdf = self._density(r, c, torch.sin(math.pi * torch.minimum(vv, to_south)))
        if not self.total > 0:
            pdf = torch.zeros_like(pdf)
        return torch.stack([r, c], -1), world, pdf

    def texel_of(self, dirs):
        d = torch.as_tensor(dirs).to(self.dev).to(self.dtype) @ self.R.to(self.dtype)
        ln = d.norm(dim=-1)
        ok = (ln > 0) & torch.isfinite(ln)
        dn = d / torch.where(ok, ln, torch.ones_like(ln))[:, None]
        u, v = dir_to_uv(dn)
        r = torch.floor(v * self.He).long().clamp(0, self.He - 1)
        c = torch.floor(u * self.We).long().clamp(0, self.We - 1)
        return r, c, torch.sqrt(dn[:, 0] ** 2 + dn[:, 2] ** 2), ok

    def texel_margin(self, dirs):
        """distance (in texels, fp64) of a direction's (u We, v He) to the nearest texel boundary: below ~1e-4 an fp32 lookup may
        land in the neighbouring texel"""
        d = torch.as_tensor(dirs).to(self.dev).double() @ self.R
        u, v = dir_to_uv(d / d.norm(dim=-1, keepdim=True).clamp_min(1e-300))
        a, b = u * self.We, v * self.He
        mu = (a - torch.round(a)).abs() if self.We > 1 else torch.full_like(a, INF)
        mv = torch.where((torch.round(b) > 0) & (torch.round(b) < self.He), (b - torch.round(b)).abs(), torch.full_like(b, INF))
        return torch.minimum(mu, mv)

    def pdf(self, dirs):
        r, c, st, ok = self.texel_of(dirs)
        return torch.where(ok, self._density(r, c, st), torch.zeros_like(st))

    def lookup(self, dirs):
        r, c, st, ok = self.texel_of(dirs)
        return torch.where(ok[:, None], self.image[r, c].to(self.dtype), torch.zeros((1, 3), dtype=self.dtype, device=self.dev))


# ---- the BRDF ----
def _clamp_cos(c):
    return c.clamp(0.00001, 0.99999)


def smith_g1(c, alpha):
    root = alpha * torch.sqrt(1.0 - c * c) / (c + 1e-10)
    return 2.0 / (1.0 + torch.hypot(root, torch.ones_like(root)))


def ggx_ndf(c, alpha):
    c2 = c * c
    root = c2 + (1.0 - c2) / (alpha * alpha + 1e-10)
    return 1.0 / (math.pi * alpha * alpha * root * root + 1e-10)


def fresnel_dielectric_pos(c, eta=ETA):
    cos_t = torch.sqrt(1.0 - (1.0 - c * c) * (1.0 / eta) ** 2)
    rs = (c - eta * cos_t) / (c + eta * cos_t)
    rp = (eta * c - cos_t) / (eta * c + cos_t)
    return 0.5 * (rs * rs + rp * rp)


def table_index(c, alpha):
    """indices into the two Mitsuba tables (100 theta x 50 alpha) as rtrans_lookup forms them"""
    tx = torch.floor(c ** 0.25 * 100).long()
    ty = torch.floor((alpha / 4.0) ** 0.25 * 50).long()
    return (ty * 100 + tx).clamp(0, 4999), ty.clamp(0, 49)


def roughplastic_point(n, v, l, kd, ks, rough, tables, dtype=torch.float64):
    """(diffuse cos_i, specular cos_i) [m, 3] of the rough plastic for normal n, view v, light l (unit, [m, 3]); rough [m]."""
    mt, md = (t.to(n.device).to(dtype) for t in tables)
    n, v, l, kd, ks, rough = (x.to(dtype) for x in (n, v, l, kd, ks, rough))
    nl = _dot(n, l)
    h = v + l
    hl = h.norm(dim=-1)
    ok = (nl > 0) & (hl > 0)
    h = h / torch.where(hl > 0, hl, torch.ones_like(hl))[:, None]
    cos_o, cos_i, cos_h, cos_d = _clamp_cos(_dot(n, v)), _clamp_cos(nl), _clamp_cos(_dot(n, h)), _clamp_cos(_dot(v, h))
    alpha = rough.clamp(min=0.0001)
    spec = fresnel_dielectric_pos(cos_d) * ggx_ndf(cos_h, alpha) * smith_g1(cos_i, alpha) * smith_g1(cos_o, alpha) / (4.0 * cos_o + 1e-10)
    ti, ai = table_index(cos_i, alpha)
    to, _ = table_index(cos_o, alpha)
    fd = 1.0 - (1.0 - md[ai]).clamp(0, 1) + 1e-10
    diff = cos_i * mt[ti].clamp(0, 1) * mt[to].clamp(0, 1) / (ETA * ETA) / fd / math.pi
    zero = torch.zeros_like(kd)
    return torch.where(ok[:, None], kd * diff[:, None], zero), torch.where(ok[:, None], ks * spec[:, None], zero)


def table_margin(n, v, l, rough):
    """fp64 distance (in table steps) of roughplastic_point's three table coordinates to the nearest step: below ~1e-4 an fp32
    evaluation may read the neighbouring entry of the piecewise-constant tables"""
    n, v, l, rough = (x.double() for x in (n, v, l, rough))
    alpha = rough.clamp(min=0.0001)
    co = [_clamp_cos(_dot(n, l)) ** 0.25 * 100, _clamp_cos(_dot(n, v)) ** 0.25 * 100, (alpha / 4.0) ** 0.25 * 50]
    return torch.stack([(c - torch.round(c)).abs() for c in co], -1).min(-1).values


# ---- random numbers, in integers ----
def _lowbias32(x):
    x = x.astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & M
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & M
    x ^= x >> np.uint64(16)
    return x


def env_rand(seed, pixel, sample, dim):
    """numpy float64 (exactly the kernel's fp32 value): (2 k + 1) 2^-24 with k the top 23 bits of the hash"""
    M = np.uint64(0xFFFFFFFF)
    pixel, sample = np.broadcast_arrays(np.asarray(pixel, dtype=np.uint64), np.asarray(sample, dtype=np.uint64))
    h = _lowbias32(np.full(pixel.shape, int(seed) & 0xFFFFFFFF, dtype=np.uint64))
    h = _lowbias32(h ^ (pixel & M))
    h = _lowbias32((h + sample) & M)
    h = _lowbias32((h + np.uint64((0x9e3779b9 * (int(dim) + 1)) & 0xFFFFFFFF)) & M)
    return ((((h >> np.uint64(9)) << np.uint64(1)) | np.uint64(1)).astype(np.float64)) * 2.0 ** -24


# ---- BRDF sampling ----
def tangent_frame(n):
    sg = torch.where(n[:, 2] >= 0, torch.ones_like(n[:, 2]), -torch.ones_like(n[:, 2]))  # copysign(1, n.z); -0.0 does not occur
    a = -1.0 / (sg + n[:, 2])
    q = n[:, 0] * n[:, 1] * a
    t = torch.stack([1.0 + sg * n[:, 0] * n[:, 0] * a, sg * q, -sg * n[:, 0]], -1)
    b = torch.stack([q, sg + n[:, 1] * n[:, 1] * a, -n[:, 1]], -1)
    return t, b


def brdf_pdf(n, v, w, alpha):
    nw = _dot(n, w)
    pc = torch.where(nw > 0, nw / math.pi, torch.zeros_like(nw))
    h = v + w
    hl = h.norm(dim=-1)
    h = h / torch.where(hl > 0, hl, torch.ones_like(hl))[:, None]
    c, vh = _dot(n, h), _dot(v, h)
    x = torch.cross(n, h, dim=-1)
    a2 = alpha * alpha
    den = a2 * c * c + _dot(x, x)
    ok = (hl > 0) & (c > 0) & (vh > 0)
    pg = torch.where(ok, (a2 / (math.pi * den * den)) * c / (4.0 * torch.where(ok, vh, torch.ones_like(vh))), torch.zeros_like(c))
    return 0.5 * (pc + pg)


def brdf_sample(n, v, alpha, u0, u1, u2):
    """-> (w [m, 3] (zero where there is no sample), ok [m])"""
    t, b = tangent_frame(n)
    phi = 2 * math.pi * u1
    cp, sp = torch.cos(phi), torch.sin(phi)
    cosine = u2 < 0.5
    tan2 = alpha * alpha * u0 / (1.0 - u0)
    zg = 1.0 / torch.sqrt(1.0 + tan2)
    s = torch.where(cosine, torch.sqrt(u0), torch.sqrt(tan2) * zg)
    z = torch.where(cosine, torch.sqrt(1.0 - u0), zg)
    d = (s * cp)[:, None] * t + (s * sp)[:, None] * b + z[:, None] * n
    vh = _dot(v, d)
    refl = 2.0 * vh[:, None] * d - v
    ok = cosine | (vh > 0)
    w = torch.where(cosine[:, None], d, refl)
    return torch.where(ok[:, None], w, torch.zeros_like(w)), ok


# ---- visibility, brute force ----
def any_hit(o, d, V, F, skip=None, dtype=torch.float64, chunk=1 << 21):
    """-> (hit [m] bool, margin [m]): is any face (but `skip` [m]) met with t in (0, inf]; margin = over the faces whose plane is
    crossed at t > 0, the smallest |distance of the barycentric weights to the edge test| : a ray with a small margin may go either way."""
    dev = o.device
    o, d = o.to(dtype), d.to(dtype)
    V = torch.as_tensor(V).to(device=dev, dtype=dtype)
    F = torch.as_tensor(F).long().to(dev)
    a, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    m, nf = o.shape[0], F.shape[0]
    hit = torch.zeros(m, dtype=torch.bool, device=dev)
    margin = torch.full((m,), INF, dtype=dtype, device=dev)
    ar = torch.arange(nf, device=dev)
    step = max(1, chunk // nf)
    for i0 in range(0, m, step):
        oo, dd = o[i0:i0 + step, None, :], d[i0:i0 + step, None, :]
        k = oo.shape[0]
        p = torch.cross(dd.expand(k, nf, 3), e2[None].expand(k, nf, 3), dim=-1)
        det = _dot(e1[None], p)
        s = oo - a[None]
        u = _dot(s, p) / det
        q = torch.cross(s, e1[None].expand(k, nf, 3), dim=-1)
        v = _dot(dd, q) / det
        t = _dot(e2[None], q) / det
        front = (det != 0) & (t > 0) & torch.isfinite(t)
        if skip is not None:
            front = front & (ar[None] != skip[i0:i0 + k, None])
        inside = torch.minimum(torch.minimum(u, v), 1 - u - v)
        hit[i0:i0 + k] = (front & (inside >= 0)).any(1)
        margin[i0:i0 + k] = torch.where(front, inside.abs(), torch.full_like(inside, INF)).min(1).values
    return hit, margin


def geometric_normals(V, F):
    V = torch.as_tensor(V).double()
    F = torch.as_tensor(F).long()
    return _unit(torch.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]], dim=-1))


def shadow_origin(x, ng, w, eps_d):
    sg = torch.where(_dot(ng, w) > 0, torch.ones_like(w[:, 0]), -torch.ones_like(w[:, 0]))
    return x + (sg * eps_d)[:, None] * ng


def visibility(x, n, ng, v, w, face, V, F, eps_d, dtype=torch.float64):
    """V(w) of the integrator and the brute-force margin: n.w > 0, (n_g.w)(n_g.v) > 0 and no face but `face` along the shadow ray"""
    x, n, ng, v, w = (t.to(dtype) for t in (x, n, ng, v, w))
    ngw = _dot(ng, w)
    front = (_dot(n, w) > 0) & (ngw * _dot(ng, v) > 0)
    hit, margin = any_hit(shadow_origin(x, ng, w, eps_d), w, V, F, skip=face, dtype=dtype)
    return front & ~hit, margin, front


# ---- the integrator's samples ----
def pixel_samples(env, n, v, alpha, pixel, n_light, n_brdf, seed, dtype=torch.float64):
    """For P pixels (normal n [P, 3], view v [P, 3], alpha [P], pixel index [P]) the N = n_light + n_brdf samples each, environment
    samples first, flattened to [P * N]: dir, p_light, p_brdf, denom (the balance heuristic's), gap (distance of the environment
    sample's u to the nearest CDF boundary, in fp32 ulps), texel (environment samples; -1 else), ok (false: a GGX sample with v.h <= 0)."""
    dev = env.dev
    P, N = n.shape[0], n_light + n_brdf
    k = np.arange(N)[None, :]
    pix = np.asarray(torch.as_tensor(pixel).cpu()).astype(np.int64)[:, None]
    u = [torch.from_numpy(env_rand(seed, pix, k, dim)).to(dev) for dim in range(3)]  # [P, N]
    e3 = lambda a: a.to(dtype)[:, None, :].expand(P, N, 3)  # noqa: E731
    nn, vv = e3(n), e3(v)
    al = alpha.to(dtype)[:, None].expand(P, N)
    w = torch.zeros((P, N, 3), dtype=dtype, device=dev)
    pl = torch.zeros((P, N), dtype=dtype, device=dev)
    gap = torch.full((P, N), INF, dtype=torch.float64, device=dev)
    texel = torch.full((P, N, 2), -1, dtype=torch.long, device=dev)
    ok = torch.ones((P, N), dtype=torch.bool, device=dev)
    if n_light:
        tx, wl, p = env.sample(torch.stack([u[0][:, :n_light].reshape(-1), u[1][:, :n_light].reshape(-1)], -1))
        w[:, :n_light], pl[:, :n_light] = wl.reshape(P, n_light, 3).to(dtype), p.reshape(P, n_light).to(dtype)
        gap[:, :n_light], texel[:, :n_light] = env.boundary_gap.reshape(P, n_light), tx.reshape(P, n_light, 2)
    if n_brdf:
        f = lambda a: a[:, n_light:].reshape(-1, *a.shape[2:])  # noqa: E731
        wb, okb = brdf_sample(f(nn), f(vv), f(al), f(u[0]).to(dtype), f(u[1]).to(dtype), f(u[2]).to(dtype))
        w[:, n_light:], ok[:, n_light:] = wb.reshape(P, n_brdf, 3), okb.reshape(P, n_brdf)
        pl[:, n_light:] = env.pdf(wb).reshape(P, n_brdf).to(dtype)
    pb = torch.where(ok, brdf_pdf(nn.reshape(-1, 3), vv.reshape(-1, 3), w.reshape(-1, 3), al.reshape(-1)).reshape(P, N), torch.zeros_like(pl))
    denom = (n_light * pl if n_light else torch.zeros_like(pl)) + (n_brdf * pb if n_brdf else torch.zeros_like(pl))
    fl = lambda a: a.reshape(P * N, *a.shape[2:])  # noqa: E731
    return {"dir": fl(w), "p_light": fl(pl), "p_brdf": fl(pb), "denom": fl(denom), "gap": fl(gap), "texel": fl(texel), "ok": fl(ok)}


def sample_terms(env, n, v, kd, ks, rough, w, denom, vis, tables, texel=None):
    """fp64 (diffuse, specular) terms [m, 3] of m samples (every argument per sample): L(w) f(w) V / denom; L of the given texel
    (rows >= 0: an environment sample's own) or of the direction."""
    fd, fs = roughplastic_point(n.double(), v.double(), w.double(), kd.double(), ks.double(), rough.double(), tables)
    L = env.lookup(w.double()).double()
    if texel is not None:
        known = texel[:, 0] >= 0
        L = torch.where(known[:, None], env.image[texel[:, 0].clamp(min=0), texel[:, 1].clamp(min=0)], L)
    good = (vis.bool() & (denom > 0))[:, None]
    safe = torch.where(denom > 0, denom.double(), torch.ones_like(denom.double()))[:, None]
    zero = torch.zeros_like(fd)
    return torch.where(good, L * fd / safe, zero), torch.where(good, L * fs / safe, zero)


# ---- quadrature of the full integral, independent of the sampler ----
def quadrature(env, x, n, ng, v, kd, ks, rough, face, V, F, eps_d, tables, sub=8):
    """fp64 integral over the sphere of L f V, every texel split into sub x sub cells in (u, v) (midpoint rule, solid angle
    2 pi^2 sin(theta) du dv), with the brute-force visibility -> (diffuse [3], specular [3])"""
    dev = env.dev
    He, We = env.He, env.We
    vv = (torch.arange(He * sub, dtype=torch.float64, device=dev) + 0.5) / (He * sub)
    uu = (torch.arange(We * sub, dtype=torch.float64, device=dev) + 0.5) / (We * sub)
    U, Vv = torch.meshgrid(uu, vv, indexing="xy")
    w = (uv_to_dir(U.reshape(-1), Vv.reshape(-1)) @ env.R.T)
    dom = (2 * math.pi ** 2 / (He * We * sub * sub)) * torch.sin(math.pi * Vv.reshape(-1))
    rows = torch.arange(He * sub, device=dev) // sub
    cols = torch.arange(We * sub, device=dev) // sub
    L = env.image[rows[:, None], cols[None, :]].reshape(-1, 3)
    m = w.shape[0]
    e = lambda a: a.double()[None].expand(m, -1)  # noqa: E731
    vis, _, _ = visibility(e(x), e(n), e(ng), e(v), w, torch.full((m,), int(face), device=dev), V, F, eps_d)
    fd, fs = roughplastic_point(e(n), e(v), w, e(kd), e(ks), torch.full((m,), float(rough), dtype=torch.float64, device=dev), tables)
    k = (dom * vis.double())[:, None] * L
    return (k * fd).sum(0), (k * fs).sum(0)


# ---- Radiance RGBE, the encoder the reader is tested against ----
def encode_rgbe(img):
    """float [H, W, 3] -> uint8 [H, W, 4], mantissas rounded to nearest: channel = mantissa 2^(e - 136)"""
    img = np.asarray(img, dtype=np.float64)
    mx = img.max(-1)
    e = np.where(mx > 1e-38, np.floor(np.log2(np.maximum(mx, 1e-300))) + 1, 0)  # mx in [2^(e-1), 2^e)
    man = np.rint(img / np.exp2(e - 8)[..., None])
    bump = man.max(-1) >= 256
    e = np.where(bump, e + 1, e)
    man = np.where(bump[..., None], np.rint(img / np.exp2(e - 8)[..., None]), man)
    out = np.zeros(img.shape[:2] + (4,), dtype=np.uint8)
    ok = mx > 1e-38
    out[..., :3] = np.where(ok[..., None], man, 0).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    return out


def write_hdr(path, rgbe, rle):
    """rgbe uint8 [H, W, 4] as a Radiance picture, flat scanlines or new-style run-length encoded ones"""
    H, W = rgbe.shape[:2]
    out = bytearray(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W))
    for y in range(H):
        if not rle:
            out += rgbe[y].tobytes()
            continue
        out += bytes([2, 2, W >> 8, W & 255])
        for ch in range(4):
            row = rgbe[y, :, ch]
            x = 0
            while x < W:
                run = 1
                while x + run < W and run < 127 and row[x + run] == row[x]:
                    run += 1
                if run >= 4:
                    out += bytes([128 + run, int(row[x])])
                    x += run
                    continue
                lit = x  # literals up to the next run of >= 4, at most 128
                while lit < W and lit - x < 128:
                    r2 = 1
                    while lit + r2 < W and r2 < 4 and row[lit + r2] == row[lit]:
                        r2 += 1
                    if r2 >= 4:
                        break
                    lit += 1
                out += bytes([lit - x]) + row[x:lit].tobytes()
                x = lit
    with open(path, "wb") as fp:
        fp.write(bytes(out))


# ---- the scenes, maps and inputs of the tests (CPU checks of their stability and the GPU tests share them) ----
VIS_MARGIN = 1e-4   # a visibility mismatch is allowed only below this brute-force margin ...
VIS_SHARE = 1e-3    # ... and on at most this share of the shadow rays
FLIP_SHARE = 1e-3   # share of u within 4 fp32 ulps of a CDF boundary (expected ~2.4e-4 with 512 boundaries)
HOT = (3, 9)        # the texel at 1e4 of the integrator's map


def ulps(u, k):
    """k fp32 ulps at u (fp64 tensor of positive values)"""
    return k * torch.exp2(torch.floor(torch.log2(u.double())) - 23)


def f32(x):
    return x.float().double()


def env_maps():
    g = torch.Generator().manual_seed(31)
    holes = torch.rand((8, 16, 3), generator=g, dtype=torch.float64)
    holes[0] = 0.0
    holes[5] = 0.0
    holes[7] = 0.0
    holes[2, 4] = 0.0
    holes[3, 0] = 0.0
    holes[6, 15] = 0.0
    return {"1x1": f32(torch.full((1, 1, 3), 0.4, dtype=torch.float64)),
            "2x3": f32(torch.rand((2, 3, 3), generator=g, dtype=torch.float64)),
            "16x32": f32(torch.rand((16, 32, 3), generator=g, dtype=torch.float64) * 2),
            "holes": f32(holes)}


def hot_map():
    g = torch.Generator().manual_seed(32)
    img = 0.05 + 0.1 * torch.rand((16, 32, 3), generator=g, dtype=torch.float64)
    img[HOT[0], HOT[1]] = 1e4
    return f32(img)


def sample_inputs(n=100000):
    u = torch.rand((n, 2), generator=torch.Generator().manual_seed(33), dtype=torch.float32).clamp(2.0 ** -24, 1 - 2.0 ** -24)
    return u.double()


def scene(name):
    """{V, F (fp32-exact), uvs, face_uvs, material [h, w, 7], normals, cam, target, eps_d}: `floor`, a two-triangle floor y = 0 with
    a one-quad occluder at y = 1/2 above it, and `cube`, the unit cube with smooth vertex normals (shading and geometric normals
    differ: both side tests matter)."""
    import _meshdist_oracle as MO
    g = torch.Generator().manual_seed(34)
    if name == "floor":
        V = torch.tensor([[-1.0, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1], [-0.3, 0.5, -0.3], [0.3, 0.5, -0.3], [0.3, 0.5, 0.3], [-0.3, 0.5, 0.3]],
                         dtype=torch.float64)
        F = torch.tensor([[0, 2, 1], [0, 3, 2], [4, 6, 5], [4, 7, 6]])
        uvs = torch.stack([(V[:, 0] + 1) / 2, (V[:, 2] + 1) / 2], -1)
        cam, target, normals = (0.4, 1.5, 2.2), (0.0, 0.0, 0.0), "face"
    else:
        V, F = MO.unit_cube()
        V, F = V.double(), F[:, [0, 2, 1]]  # that cube is wound inwards; outward normals here, or every view would be back-facing
        uvs = torch.stack([0.5 * V[:, 0] + 0.25 * V[:, 2] + 0.1, 0.5 * V[:, 1] + 0.25 * V[:, 2] + 0.1], -1)
        cam, target, normals = (1.9, 1.6, 2.4), (0.5, 0.5, 0.5), "vertex"
    mat = torch.rand((4, 4, 7), generator=g, dtype=torch.float64) * 0.6 + 0.2
    mat[..., 6] = 0.2 + 0.4 * torch.rand((4, 4), generator=g, dtype=torch.float64)
    V = f32(V)
    return {"V": V, "F": F, "uvs": f32(uvs), "face_uvs": F, "material": f32(mat), "normals": normals, "cam": cam, "target": target,
            "eps_d": 1e-4 * float((V.max(0).values - V.min(0).values).norm())}


def scene_rays(sc, W=33, H=31):
    import _meshrender_oracle as O
    o, d = O.pinhole_rays(sc["cam"], W, H, 0.9 * W, target=sc["target"])
    return f32(o), f32(d)


def oracle_probe_rays(sc, seed):
    """The primary hits of the scene's camera (fp64) with 24 random directions each about the geometric normal: the population the
    stability of the fp32 visibility is measured on.  -> x, n (= n_g), n_g, v, face, w, one row per shadow ray."""
    import _meshrender_oracle as O
    o, d = scene_rays(sc)
    t, f, _, _ = O.closest_hit(o, d, sc["V"], sc["F"])
    hit = f >= 0
    x = (o + t[:, None] * d)[hit]
    ng = geometric_normals(sc["V"], sc["F"])[f[hit]]
    v = -d[hit]
    k = 24
    g = torch.Generator().manual_seed(seed)
    w = _unit(torch.randn((x.shape[0], k, 3), generator=g, dtype=torch.float64))
    w = torch.where((_dot(w, ng[:, None, :]) * _dot(v, ng)[:, None] > 0)[..., None], w, -w)  # on the viewer's side
    e = lambda a: a[:, None].expand(a.shape[0], k, *a.shape[1:]).reshape(-1, *a.shape[1:])  # noqa: E731
    return f32(e(x)), e(ng), e(ng), e(v), e(f[hit]), f32(w.reshape(-1, 3))
