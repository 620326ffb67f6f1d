"""Multiresolution hash-grid encoding on gfx950: the tcnn.Encoding of models/tcnn_fields.py (tiny-cuda-nn's published HashGrid with
Linear interpolation, fp32 table), csrc/hashgrid.hip and csrc/hashgrid_train.hip; the definition is DESIGN.md "Hash-grid encoding".

    enc = HashEncoding(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.3819).cuda()
    y = enc(x)                                   # x [..., 3] in [0, 1] (clamped), y [..., 32]
    n = torch.autograd.grad(y.sum(), x, create_graph=True)[0]; ((n.norm(dim=-1) - 1) ** 2).mean().backward()

Two autograd functions: the encoding, and its input gradient d_x = sum dy J as a differentiable function of (dy, table), so that an
eikonal term reaches the table (a third node carries the table gradient, so that torch.autograd.grad(y, x) does not compute it).  The second derivative with respect to x is not built: a LEAF x with requires_grad receives the
first-order term only (like fields.SDFNetwork.get_all), an x that is itself the result of a differentiable computation is
refused under create_graph, where that term would silently be missing."""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib

ENCODING_KEYS = ("n_levels", "n_features_per_level", "log2_hashmap_size", "base_resolution", "per_level_scale")


def make_desc(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale) -> _lib.iron_hashgrid_desc:
    """The descriptor of the C ABI; a value outside the definition's range raises an IronError that names the key."""
    vals = dict(n_levels=n_levels, n_features_per_level=n_features_per_level, log2_hashmap_size=log2_hashmap_size,
                base_resolution=base_resolution, per_level_scale=per_level_scale)
    for k in ENCODING_KEYS[:4]:
        v = vals[k]
        if isinstance(v, bool) or not isinstance(v, int):
            if not (isinstance(v, float) and v == int(v)):
                raise _lib.IronError("hash-grid encoding: %s must be an integer, got %r" % (k, v))
            vals[k] = int(v)
    if not 1 <= vals["n_levels"] <= _lib.IRON_HASHGRID_MAX_LEVELS:
        raise _lib.IronError("hash-grid encoding: n_levels must be 1 .. 32, got %r" % (n_levels,))
    if vals["n_features_per_level"] not in (1, 2, 4, 8):
        raise _lib.IronError("hash-grid encoding: n_features_per_level must be 1, 2, 4 or 8, got %r" % (n_features_per_level,))
    if not 1 <= vals["log2_hashmap_size"] <= 24:
        raise _lib.IronError("hash-grid encoding: log2_hashmap_size must be 1 .. 24, got %r" % (log2_hashmap_size,))
    if vals["base_resolution"] < 1:
        raise _lib.IronError("hash-grid encoding: base_resolution must be at least 1, got %r" % (base_resolution,))
    b = float(per_level_scale)
    if not (b >= 1.0 and math.isfinite(b)):
        raise _lib.IronError("hash-grid encoding: per_level_scale must be at least 1, got %r" % (per_level_scale,))
    d = _lib.iron_hashgrid_desc()
    d.n_levels, d.n_features_per_level = vals["n_levels"], vals["n_features_per_level"]
    d.log2_hashmap_size, d.base_resolution, d.per_level_scale = vals["log2_hashmap_size"], vals["base_resolution"], b
    return d


def layout(desc: _lib.iron_hashgrid_desc):
    """(levels, n_params) from iron_hashgrid_layout (host only): levels is a list of dicts scale / res / size / offset / dense."""
    lv = (_lib.iron_hashgrid_level * _lib.IRON_HASHGRID_MAX_LEVELS)()
    n = C.c_int64(0)
    rc = _lib.load().iron_hashgrid_layout(C.byref(desc), lv, C.byref(n))
    if rc == _lib.IRON_ERR_RANGE:
        raise _lib.IronError("hash-grid encoding: per_level_scale ** (n_levels - 1) * base_resolution reaches 2^22, past what the "
                             "fp32 cell arithmetic resolves")
    _lib.check(rc)
    levels = [dict(scale=float(lv[l].scale), res=int(lv[l].res), size=int(lv[l].size), offset=int(lv[l].offset),
                   dense=bool(lv[l].dense)) for l in range(desc.n_levels)]
    return levels, int(n.value)


def parse_encoding_config(cfg: dict) -> dict:
    """The `encoding` block of a tiny-cuda-nn style JSON -> HashEncoding's keyword arguments.  Whatever the kernels are not built for
    (another grid type or interpolation, fp16 tables, an unknown key) raises an IronError that names the key."""
    if not isinstance(cfg, dict):
        raise _lib.IronError("encoding: expected a JSON object, got %s" % type(cfg).__name__)
    fixed = {"otype": ("HashGrid",), "type": ("Hash",), "interpolation": ("Linear",), "n_dims_to_encode": (3,),
             "table_dtype": ("float32", "fp32"), "dtype": ("float32", "fp32")}
    out = {}
    for k, v in cfg.items():
        if k in ENCODING_KEYS:
            out[k] = v
        elif k in fixed:
            if v not in fixed[k]:
                raise _lib.IronError("encoding: %s = %r is not built (only %s)" % (k, v, " / ".join(map(str, fixed[k]))))
        else:
            raise _lib.IronError("encoding: unknown key %r" % (k,))
    if cfg.get("otype") != "HashGrid":
        raise _lib.IronError("encoding: otype must be \"HashGrid\", got %r" % (cfg.get("otype"),))
    for k in ENCODING_KEYS:
        if k not in out:
            raise _lib.IronError("encoding: missing key %r" % (k,))
    return out


def grad_unit(bound: float, n: int) -> float:
    """The fixed-point unit of a table gradient whose contributions are bounded by `bound` (fp32) over n points."""
    return math.ldexp(1.0, _lib.load_train().iron_hashgrid_grad_unit_exp(float(bound), int(n)))


def _check_inputs(x, table, desc, n_params):
    x = _lib.require_cuda_f32(x, "x")
    table = _lib.require_cuda_f32(table, "params")
    if x.dim() != 2 or x.shape[1] != 3:
        raise _lib.IronError("hash-grid encoding: x must be [n, 3], got %s" % (tuple(x.shape),))
    if table.numel() != n_params * desc.n_features_per_level:
        raise _lib.IronError("hash-grid encoding: params holds %d values, the layout needs %d" % (table.numel(), n_params * desc.n_features_per_level))
    if table.device != x.device:
        raise _lib.IronError("hash-grid encoding: x and params live on different devices")
    return x, table


def encode(desc, n_params, x, table, jacobian=False):
    """y [n, L F] (and J [n, L F, 3] when asked) of iron_hashgrid_encode."""
    x, table = _check_inputs(x, table, desc, n_params)
    n, width = x.shape[0], desc.n_levels * desc.n_features_per_level
    y = torch.empty((n, width), dtype=torch.float32, device=x.device)
    jac = torch.empty((n, width, 3), dtype=torch.float32, device=x.device) if jacobian else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().iron_hashgrid_encode(C.byref(desc), x.data_ptr(), n, table.data_ptr(), y.data_ptr(), _lib.ptr(jac),
                                                    _lib.stream_ptr(x.device)))
    return (y, jac) if jacobian else y


def _table_out(out, n_params, F, device):
    if out is None:
        return torch.empty((n_params, F), dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or out.device != device or not out.is_contiguous() or out.numel() != n_params * F:
        raise _lib.IronError("hash-grid encoding: d_table_out must be a contiguous float32 tensor of %d values on x's device" % (n_params * F))
    return out


def backward(desc, n_params, x, table, dy, want_table=True, want_x=True, d_table_out=None):
    """(d_table [n_params, F] or None, d_x [n, 3] or None) of iron_hashgrid_backward; d_table_out: a buffer to write d_table into
    (every entry is written)."""
    x, table = _check_inputs(x, table, desc, n_params)
    dy = _lib.require_cuda_f32(dy, "dy")
    n, F = x.shape[0], desc.n_features_per_level
    if dy.numel() != n * desc.n_levels * F:
        raise _lib.IronError("hash-grid encoding: dy must be [n, %d]" % (desc.n_levels * F))
    lib = _lib.load_train()
    d_table = _table_out(d_table_out, n_params, F, x.device) if want_table else None
    d_x = torch.empty((n, 3), dtype=torch.float32, device=x.device) if want_x else None
    ws, nbytes = None, 0
    with torch.cuda.device(x.device):
        if want_table:
            nbytes = lib.iron_hashgrid_backward_workspace_bytes(C.byref(desc), n)
            ws = _lib.workspace(nbytes, x.device, "hashgrid")
        _lib.check_train(lib.iron_hashgrid_backward(C.byref(desc), x.data_ptr(), n, table.data_ptr(), dy.data_ptr(), _lib.ptr(d_table),
                                                    _lib.ptr(d_x), _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)))
    return d_table, d_x


def backward_backward(desc, n_params, x, table, dy, g, want_dy=True, want_table=True, d_table_out=None):
    """(d_dy [n, L F] or None, d_table [n_params, F] or None) of iron_hashgrid_backward_backward."""
    x, table = _check_inputs(x, table, desc, n_params)
    dy = _lib.require_cuda_f32(dy, "dy")
    g = _lib.require_cuda_f32(g, "g")
    n, F = x.shape[0], desc.n_features_per_level
    if dy.numel() != n * desc.n_levels * F or g.numel() != n * 3:
        raise _lib.IronError("hash-grid encoding: dy must be [n, %d] and g [n, 3]" % (desc.n_levels * F))
    lib = _lib.load_train()
    d_dy = torch.empty((n, desc.n_levels * F), dtype=torch.float32, device=x.device) if want_dy else None
    d_table = _table_out(d_table_out, n_params, F, x.device) if want_table else None
    ws, nbytes = None, 0
    with torch.cuda.device(x.device):
        if want_table:
            nbytes = lib.iron_hashgrid_backward_backward_workspace_bytes(C.byref(desc), n)
            ws = _lib.workspace(nbytes, x.device, "hashgrid")
        _lib.check_train(lib.iron_hashgrid_backward_backward(C.byref(desc), x.data_ptr(), n, table.data_ptr(), dy.data_ptr(), g.data_ptr(),
                                                             _lib.ptr(d_dy), _lib.ptr(d_table), _lib.ptr(ws), nbytes,
                                                             _lib.stream_ptr(x.device)))
    return d_dy, d_table


def backward_pair(desc, n_params, x, table, dy1, dy2, g, d_table_out=None):
    """d_table [n_params, F] of iron_hashgrid_backward_pair: backward(dy1)'s table term plus backward_backward(dy2, g)'s, each
    (corner, feature) rounded and added once."""
    x, table = _check_inputs(x, table, desc, n_params)
    dy1, dy2, g = _lib.require_cuda_f32(dy1, "dy1"), _lib.require_cuda_f32(dy2, "dy2"), _lib.require_cuda_f32(g, "g")
    n, F = x.shape[0], desc.n_features_per_level
    if dy1.numel() != n * desc.n_levels * F or dy2.numel() != n * desc.n_levels * F or g.numel() != n * 3:
        raise _lib.IronError("hash-grid encoding: dy1 and dy2 must be [n, %d] and g [n, 3]" % (desc.n_levels * F))
    lib = _lib.load_train()
    d_table = _table_out(d_table_out, n_params, F, x.device)
    with torch.cuda.device(x.device):
        nbytes = lib.iron_hashgrid_backward_pair_workspace_bytes(C.byref(desc), n)
        ws = _lib.workspace(nbytes, x.device, "hashgrid")
        _lib.check_train(lib.iron_hashgrid_backward_pair(C.byref(desc), x.data_ptr(), n, table.data_ptr(), dy1.data_ptr(), dy2.data_ptr(),
                                                         g.data_ptr(), d_table.data_ptr(), _lib.ptr(ws), nbytes,
                                                         _lib.stream_ptr(x.device)))
    return d_table


class _InputGradFn(torch.autograd.Function):
    """d_x = sum_{l,f} dy[l,f] J[l,f,:] as a function of (dy, table); x is a constant here (its second derivative is not built)."""

    @staticmethod
    def forward(ctx, dy, table, x, enc):
        ctx.enc = enc
        dy = dy.contiguous()
        ctx.save_for_backward(dy, table, x)
        return backward(enc.desc, enc.n_params, x, table, dy, want_table=False, want_x=True)[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dy, table, x = ctx.saved_tensors
        enc = ctx.enc
        d_dy, d_table = backward_backward(enc.desc, enc.n_params, x, table, dy, g.contiguous(), want_dy=ctx.needs_input_grad[0],
                                          want_table=ctx.needs_input_grad[1])
        return d_dy, (d_table.view_as(table) if d_table is not None else None), None, None


class _EncodeFn(torch.autograd.Function):
    """y(x, table), differentiated with respect to x here; the table's gradient belongs to _TableGradFn (see HashEncoding.forward)."""

    @staticmethod
    def forward(ctx, x, table, enc, x_is_leaf):
        ctx.enc, ctx.x_is_leaf = enc, x_is_leaf
        ctx.save_for_backward(x, table)
        return encode(enc.desc, enc.n_params, x, table)

    @staticmethod
    def backward(ctx, dy):
        x, table = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if torch.is_grad_enabled() and not ctx.x_is_leaf:
            raise NotImplementedError(
                "HashEncoding under create_graph: x is the result of a differentiable computation, and the second derivative of "
                "the encoding with respect to x is not built, so the term through x would silently be missing; evaluate at a "
                "leaf (x.detach().requires_grad_(True)) as the reference's gradient() / get_all() do")
        return _InputGradFn.apply(dy.contiguous(), table, x.detach(), ctx.enc), None, None, None


class _TableGradFn(torch.autograd.Function):
    """A zero of y's shape whose backward is the table gradient.  It is a separate node so that the autograd engine can leave it
    out: torch.autograd.grad(y, x) reaches x through _EncodeFn alone and never runs the scatter, whose result it would discard
    (a Function's needs_input_grad is fixed at forward time and cannot tell)."""

    @staticmethod
    def forward(ctx, table, x, enc):
        ctx.enc = enc
        ctx.save_for_backward(x, table)
        return torch.zeros((1, 1), dtype=torch.float32, device=x.device).expand(x.shape[0], enc.n_output_dims)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, table = ctx.saved_tensors
        enc = ctx.enc
        d_table = backward(enc.desc, enc.n_params, x, table, dy.contiguous(), want_table=True, want_x=False)[0]
        return d_table.view_as(table), None, None


class HashEncoding(nn.Module):
    """tcnn.Encoding(3, {"otype": "HashGrid", ...}) with an fp32 table: `params` [n_params * F], uniform in +-1e-4."""

    def __init__(self, n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0):
        super().__init__()
        self.desc = make_desc(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale)
        self.levels, self.n_params = layout(self.desc)
        self.n_levels, self.n_features_per_level = self.desc.n_levels, self.desc.n_features_per_level
        self.n_input_dims = 3
        self.n_output_dims = self.n_levels * self.n_features_per_level
        self.params = nn.Parameter(torch.empty(self.n_params * self.n_features_per_level, dtype=torch.float32).uniform_(-1e-4, 1e-4))

    @classmethod
    def from_config(cls, cfg: dict) -> "HashEncoding":
        return cls(**parse_encoding_config(cfg))

    def extra_repr(self):
        d = self.desc
        return "n_levels=%d, n_features_per_level=%d, log2_hashmap_size=%d, base_resolution=%d, per_level_scale=%g" % (
            d.n_levels, d.n_features_per_level, d.log2_hashmap_size, d.base_resolution, d.per_level_scale)

    def _flat(self, x):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise _lib.IronError("HashEncoding: x must be a CUDA (ROCm) tensor: iron_amd has no CPU path")
        if not self.params.is_cuda:
            raise _lib.IronError("HashEncoding: params must live on a CUDA (ROCm) device; call .cuda() first")
        if x.dtype != torch.float32:
            raise _lib.IronError("HashEncoding: x must be float32, got %s" % (x.dtype,))
        if x.shape[-1] != 3:
            raise _lib.IronError("HashEncoding: x must end in 3 coordinates, got %s" % (tuple(x.shape),))
        return x.reshape(-1, 3)

    def forward(self, x):
        flat = self._flat(x)
        y = _EncodeFn.apply(flat, self.params, self, x.grad_fn is None)
        if torch.is_grad_enabled() and self.params.requires_grad:
            y = y + _TableGradFn.apply(self.params, flat.detach(), self)
        return y.reshape(*x.shape[:-1], self.n_output_dims)

    def jacobian(self, x):
        """(y, J [..., L F, 3]) without autograd: what iron_hashgrid_encode returns."""
        flat = self._flat(x)
        with torch.no_grad():
            y, jac = encode(self.desc, self.n_params, flat.contiguous(), self.params, jacobian=True)
        return y.reshape(*x.shape[:-1], self.n_output_dims), jac.reshape(*x.shape[:-1], self.n_output_dims, 3)
