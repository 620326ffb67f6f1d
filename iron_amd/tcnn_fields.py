"""models/tcnn_fields.py on gfx950: the hash-grid SDF field `TCNNSDF`, without tiny-cuda-nn.

The reference builds `tcnn.Encoding(3, config["encoding"])` and `tcnn.Network(n_enc, n_out, config["network"])` from one JSON file.
Here the encoding is iron_amd.hashgrid.HashEncoding (HIP, fp32 table) and the network is its plain-torch equivalent: bias-free
nn.Linear layers (tiny-cuda-nn's MLPs carry no biases) with the configured activation.  forward / sdf / sdf_hidden_appearance /
gradient / get_all keep the reference's shapes and detach rules (tcnn_fields.py:26-66).  Points are taken in the unit cube, as the
reference hands them to tcnn (the encoding clamps to [0, 1]).

Inference has a fused form beside it: `eval_fused` / `as_callable` evaluate the encoding and the head, and on request d sdf / dx, in
one launch of csrc/hashgrid_field.hip (exact-fp32 MFMA head, no autograd).  Training keeps the plain head by default;
with `field.fused_training = True` forward / sdf / sdf_hidden_appearance / gradient / get_all run through one autograd function whose
forward is that launch and whose backward is csrc/hashgrid_field_train.hip: first- and second-order (eikonal)
gradients of the table and the head in closed form, no autograd graph through the head and no gradient with respect to x.

`TCNNRendering` and `TCNNNeRF` are not built: the reference's forwards are empty or mis-shaped (tcnn_fields.py:201-249)."""
from __future__ import annotations

import ctypes as C
import json

import torch
import torch.nn as nn

from . import _lib
from .hashgrid import HashEncoding, parse_encoding_config

NETWORK_KEYS = ("otype", "activation", "output_activation", "n_neurons", "n_hidden_layers")
_ACTIVATIONS = {"ReLU": nn.ReLU, "Softplus": nn.Softplus, "None": nn.Identity}


def parse_network_config(cfg: dict) -> dict:
    """The `network` block -> dict(n_neurons, n_hidden_layers, activation); anything the plain head does not cover raises an
    IronError that names the key."""
    if not isinstance(cfg, dict):
        raise _lib.IronError("network: expected a JSON object, got %s" % type(cfg).__name__)
    for k in cfg:
        if k not in NETWORK_KEYS:
            raise _lib.IronError("network: unknown key %r" % (k,))
    if cfg.get("otype", "FullyFusedMLP") not in ("FullyFusedMLP", "CutlassMLP"):
        raise _lib.IronError("network: otype = %r is not built (FullyFusedMLP / CutlassMLP)" % (cfg.get("otype"),))
    act = cfg.get("activation", "ReLU")
    if act not in _ACTIVATIONS:
        raise _lib.IronError("network: activation = %r is not built (ReLU / Softplus / None)" % (act,))
    if cfg.get("output_activation", "None") != "None":
        raise _lib.IronError("network: output_activation = %r is not built (None)" % (cfg.get("output_activation"),))
    out = {"activation": act}
    for k in ("n_neurons", "n_hidden_layers"):
        v = cfg.get(k)
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise _lib.IronError("network: %s must be a positive integer, got %r" % (k, v))
        out[k] = v
    return out


def read_config(conf_path) -> dict:
    """{"encoding": HashEncoding keyword arguments, "network": parse_network_config's dict} of a tiny-cuda-nn style JSON file."""
    with open(conf_path) as f:
        config = json.load(f)
    for k in ("encoding", "network"):
        if k not in config:
            raise _lib.IronError("%s: missing block %r" % (conf_path, k))
    return {"encoding": parse_encoding_config(config["encoding"]), "network": parse_network_config(config["network"])}


def field_backward(desc, p, table, packed, train_packed, d_out, d_g, scale=None, offset=None, want_table=True, want_rows=False):
    """iron_hashgrid_field_backward (csrc/hashgrid_field_train.hip) for the adjoints d_out [n, n_out] and d_g [n, 3] of
    the fused evaluation's two results (either may be None: zero) -> (d_weights [n_weights], flat in the pack's weight order,
    d_table [n_params, F] or None, ybar [n, L F] or None, e [n, L F] or None)."""
    lib, libt = _lib.load(), _lib.load_train()
    p, table = _lib.require_cuda_f32(p, "x"), _lib.require_cuda_f32(table, "params")
    n, lf = p.shape[0], desc.encoding.n_levels * desc.encoding.n_features_per_level
    if d_out is not None:
        d_out = _lib.require_cuda_f32(d_out, "d_out")
        if d_out.numel() != n * desc.n_out:
            raise _lib.IronError("TCNNSDF: d_out must be [n, %d]" % desc.n_out)
    if d_g is not None:
        d_g = _lib.require_cuda_f32(d_g, "d_g")
        if d_g.numel() != n * 3:
            raise _lib.IronError("TCNNSDF: d_g must be [n, 3]")
    n_weights = C.c_int64(0)
    _lib.check(lib.iron_hashgrid_field_check(C.byref(desc), C.byref(n_weights)))
    d_weights = torch.empty(n_weights.value, dtype=torch.float32, device=p.device)
    d_table = torch.empty_like(table) if want_table else None
    ybar = torch.empty((n, lf), dtype=torch.float32, device=p.device) if want_rows else None
    e = torch.empty((n, lf), dtype=torch.float32, device=p.device) if want_rows else None
    with torch.cuda.device(p.device):
        nbytes = libt.iron_hashgrid_field_backward_workspace_bytes(C.byref(desc), n)
        ws = _lib.workspace(nbytes, p.device, "hashfield_train")
        _lib.check_train(libt.iron_hashgrid_field_backward(
            C.byref(desc), p.data_ptr(), n, _map3(scale, "scale"), _map3(offset, "offset"), table.data_ptr(), packed.data_ptr(),
            train_packed.data_ptr(), _lib.ptr(d_out), _lib.ptr(d_g), d_weights.data_ptr(), _lib.ptr(d_table), _lib.ptr(ybar), _lib.ptr(e),
            ws.data_ptr(), nbytes, _lib.stream_ptr(p.device)))
    return d_weights, d_table, ybar, e


class _FieldFn(torch.autograd.Function):
    """(out, d out[:, 0] / dx) of the fused evaluation as a function of (table, the head's weights); x is a constant: no gradient
    reaches it (the second derivative of the trilinear form is not built).  The forward keeps nothing but x and the
    two packed blobs; the backward recomputes it (csrc/hashgrid_field_train.hip)."""

    @staticmethod
    def forward(ctx, x, table, field, want_grad, *weights):
        desc = field._fused_desc()
        packed, train_packed = field._fused_packed(desc, x.device), field._train_packed(desc, x.device)
        n = x.shape[0]
        out = torch.empty((n, desc.n_out), dtype=torch.float32, device=x.device)
        grad = torch.empty((n, 3), dtype=torch.float32, device=x.device) if want_grad else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().iron_hashgrid_field_eval(C.byref(desc), x.data_ptr(), n, None, None, table.data_ptr(), packed.data_ptr(),
                                                            out.data_ptr(), _lib.ptr(grad), _lib.stream_ptr(x.device)))
        ctx.desc, ctx.packed, ctx.train_packed, ctx.shapes = desc, packed, train_packed, [w.shape for w in weights]
        ctx.save_for_backward(x, table)
        ctx.set_materialize_grads(False)
        return (out, grad) if want_grad else out

    @staticmethod
    def backward(ctx, d_out, d_g=None):
        if torch.is_grad_enabled():
            raise _lib.IronError("TCNNSDF.fused_training: a second backward through the fused gradient (create_graph=True) is not "
                                 "built; the plain path (fused_training = False) differentiates twice")
        x, table = ctx.saved_tensors
        d_weights, d_table, _, _ = field_backward(ctx.desc, x, table, ctx.packed, ctx.train_packed, d_out, d_g,
                                                  want_table=ctx.needs_input_grad[1])
        parts = torch.split(d_weights, [s.numel() for s in ctx.shapes])
        grads = [g.view(s) if need else None for g, s, need in zip(parts, ctx.shapes, ctx.needs_input_grad[4:])]
        return (None, d_table.view_as(table) if d_table is not None else None, None, None, *grads)


class TCNNSDF(nn.Module):
    def __init__(self, conf_path, n_inputs_dims=3, n_outputs_dims=1, geometric_init=True, weight_norm=True, inside_outside=False):
        super().__init__()
        if n_inputs_dims != 3:
            raise _lib.IronError("TCNNSDF: n_inputs_dims = %r is not built (the hash grid is 3-D)" % (n_inputs_dims,))
        config = read_config(conf_path)
        self.sdf_encoding = HashEncoding(**config["encoding"])
        net = config["network"]
        dims = [self.sdf_encoding.n_output_dims] + [net["n_neurons"]] * net["n_hidden_layers"] + [n_outputs_dims]
        layers = []
        for i in range(len(dims) - 1):
            layers.append(nn.Linear(dims[i], dims[i + 1], bias=False))
            if i < len(dims) - 2:
                layers.append(_ACTIVATIONS[net["activation"]]())
        self.sdf_network = nn.Sequential(*layers)
        self.model = nn.Sequential(self.sdf_encoding, self.sdf_network)
        self._network_config = dict(net, n_out=n_outputs_dims)    # plain attributes: the fused evaluation's shape and its
        self._fused_cache = None                                  # packed weights (key, blob); neither is part of state_dict()
        self._train_cache = None                                  # the training blob, keyed the same way
        self.fused_training = False                               # True: training runs through _FieldFn

    def forward(self, inputs):
        if self.fused_training:
            return self._fused_apply(inputs, False)
        return self.model(inputs)

    def sdf(self, x):
        return self.forward(x)[..., :1]

    def sdf_hidden_appearance(self, x):
        return self.forward(x)

    def _forward_and_gradient(self, x, attached):
        """(forward(x), d sdf / dx); x becomes a leaf that requires grad, in place, as in the reference.  `attached` keeps the
        gradient differentiable with respect to the table and the head (the reference's create_graph)."""
        x.requires_grad_(True)
        if self.fused_training:
            out, grad = self._fused_apply(x, True)
            return out, (grad if attached else grad.detach())
        out = self.forward(x)
        (grad,) = torch.autograd.grad(out[..., :1].sum(), x, create_graph=attached)
        return out, grad

    def gradient(self, x):
        return self._forward_and_gradient(x, True)[1]

    def get_all(self, x, is_training=True):
        with torch.enable_grad():
            out, grad = self._forward_and_gradient(x, is_training)
        if not is_training:
            out, grad = out.detach(), grad.detach()
        return out[..., :1], out[..., 1:], grad

    # ---- fused inference (csrc/hashgrid_field.hip): encoding and head in one launch, no autograd ----
    def _fused_desc(self):
        """The C descriptor of the fused evaluation; a shape the kernel is not built for raises an IronError that names the key."""
        net, enc = self._network_config, self.sdf_encoding
        if net["n_neurons"] not in (16, 32, 64, 128):
            raise _lib.IronError("TCNNSDF.eval_fused: n_neurons = %r is not built (16 / 32 / 64 / 128)" % (net["n_neurons"],))
        if not 1 <= net["n_hidden_layers"] <= 4:
            raise _lib.IronError("TCNNSDF.eval_fused: n_hidden_layers = %r is not built (1 .. 4)" % (net["n_hidden_layers"],))
        if not 1 <= net["n_out"] <= 16:
            raise _lib.IronError("TCNNSDF.eval_fused: n_outputs_dims = %r is not built (1 .. 16)" % (net["n_out"],))
        if enc.n_output_dims > 128:
            raise _lib.IronError("TCNNSDF.eval_fused: n_levels * n_features_per_level = %d is not built (at most 128)" % enc.n_output_dims)
        d = _lib.iron_hashgrid_field_desc()
        d.encoding = enc.desc
        d.n_neurons, d.n_hidden_layers, d.n_out = net["n_neurons"], net["n_hidden_layers"], net["n_out"]
        d.activation = _lib.IRON_FIELD_ACT[net["activation"]]
        return d

    def fused_supported(self) -> bool:
        try:
            self._fused_desc()
        except _lib.IronError:
            return False
        return True

    def fused_training_supported(self) -> bool:
        """Whether fused_training = True can run this shape (iron_hashgrid_field_train_check; host only)."""
        try:
            self._train_desc()
        except _lib.IronError:
            return False
        return True

    def _train_desc(self):
        desc = self._fused_desc()
        rc = _lib.load_train().iron_hashgrid_field_train_check(C.byref(desc))
        if rc == _lib.IRON_ERR_RANGE:
            raise _lib.IronError("TCNNSDF.fused_training: n_neurons = %r with %d hidden layers on %d features is not built (16 / 32 / 64, "
                                 "and the stages of 32 points must fit the 160 KiB of LDS)"
                                 % (self._network_config["n_neurons"], self._network_config["n_hidden_layers"], self.sdf_encoding.n_output_dims))
        _lib.check_train(rc)
        return desc

    def _fused_apply(self, x, want_grad):
        """forward (and d sdf / dx) through _FieldFn: differentiable with respect to the table and the head, not to x"""
        if not torch.is_tensor(x) or not x.is_cuda:
            raise _lib.IronError("TCNNSDF.fused_training: x must be a CUDA (ROCm) tensor: iron_amd has no CPU path")
        if x.dtype != torch.float32:
            raise _lib.IronError("TCNNSDF.fused_training: x must be float32, got %s" % (x.dtype,))
        if x.dim() < 1 or x.shape[-1] != 3:
            raise _lib.IronError("TCNNSDF.fused_training: x must end in 3 coordinates, got %s" % (tuple(x.shape),))
        if x.grad_fn is not None and torch.is_grad_enabled():
            raise _lib.IronError("TCNNSDF.fused_training: x is the result of a differentiable computation, and no gradient reaches x "
                                 "here, so its term would silently be missing; evaluate at a leaf (x.detach())")
        self._train_desc()
        table = self.sdf_encoding.params
        if table.device != x.device or table.dtype != torch.float32:
            raise _lib.IronError("TCNNSDF.fused_training: the table must be float32 on x's device; call .cuda() first")
        lin = [m.weight for m in self.sdf_network if isinstance(m, nn.Linear)]
        res = _FieldFn.apply(x.detach().reshape(-1, 3).contiguous(), table, self, want_grad, *lin)
        n_out = self._network_config["n_out"]
        if want_grad:
            return res[0].reshape(*x.shape[:-1], n_out), res[1].reshape(x.shape)
        return res.reshape(*x.shape[:-1], n_out)

    def _train_packed(self, desc, device):
        """The transposed fragments of the output layer (the adjoint chain's), repacked with the inference blob's key."""
        lin = [m.weight for m in self.sdf_network if isinstance(m, nn.Linear)]
        key = (device,) + tuple((w.data_ptr(), w._version) for w in lin)
        if self._train_cache is not None and self._train_cache[0] == key:
            return self._train_cache[1]
        lib = _lib.load_train()
        flat = torch.cat([w.detach().reshape(-1) for w in lin])
        blob = torch.empty(lib.iron_hashgrid_field_train_pack_bytes(C.byref(desc)), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            _lib.check_train(lib.iron_hashgrid_field_train_pack(C.byref(desc), flat.data_ptr(), blob.data_ptr(), _lib.stream_ptr(device)))
        self._train_cache = (key, blob)
        return blob

    def _fused_packed(self, desc, device):
        """The head's weights in MFMA fragment order, repacked when a parameter was replaced or written in place."""
        lin = [m.weight for m in self.sdf_network if isinstance(m, nn.Linear)]
        key = (device,) + tuple((w.data_ptr(), w._version) for w in lin)
        if self._fused_cache is not None and self._fused_cache[0] == key:
            return self._fused_cache[1]
        lib = _lib.load()
        n_weights = C.c_int64(0)
        _lib.check(lib.iron_hashgrid_field_check(C.byref(desc), C.byref(n_weights)))
        for w in lin:
            if w.device != device or w.dtype != torch.float32:
                raise _lib.IronError("TCNNSDF.eval_fused: the head's weights must be float32 on x's device")
        flat = torch.cat([w.detach().reshape(-1) for w in lin])
        if flat.numel() != n_weights.value:
            raise _lib.IronError("TCNNSDF.eval_fused: the head holds %d weights, the descriptor needs %d" % (flat.numel(), n_weights.value))
        packed = torch.empty(lib.iron_hashgrid_field_pack_bytes(C.byref(desc)), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            _lib.check(lib.iron_hashgrid_field_pack(C.byref(desc), flat.data_ptr(), packed.data_ptr(), _lib.stream_ptr(device)))
        self._fused_cache = (key, packed)
        return packed

    def eval_fused(self, x, gradient=False, scale=None, offset=None):
        """out [..., n_out], or (out, d out[..., 0] / dx [..., 3]) with gradient=True, at scale * x + offset (per axis; None: x itself),
        in one launch.  Inference only: runs under no_grad, the results carry no graph."""
        if not torch.is_tensor(x) or not x.is_cuda:
            raise _lib.IronError("TCNNSDF.eval_fused: x must be a CUDA (ROCm) tensor: iron_amd has no CPU path")
        if x.dtype != torch.float32:
            raise _lib.IronError("TCNNSDF.eval_fused: x must be float32, got %s" % (x.dtype,))
        if x.dim() < 1 or x.shape[-1] != 3:
            raise _lib.IronError("TCNNSDF.eval_fused: x must end in 3 coordinates, got %s" % (tuple(x.shape),))
        desc = self._fused_desc()
        table = self.sdf_encoding.params
        if table.device != x.device or table.dtype != torch.float32:
            raise _lib.IronError("TCNNSDF.eval_fused: the table must be float32 on x's device; call .cuda() first")
        a, b = _map3(scale, "scale"), _map3(offset, "offset")
        with torch.no_grad():
            flat = x.detach().reshape(-1, 3).contiguous()
            n, n_out = flat.shape[0], desc.n_out
            packed = self._fused_packed(desc, x.device)
            out = torch.empty((n, n_out), dtype=torch.float32, device=x.device)
            grad = torch.empty((n, 3), dtype=torch.float32, device=x.device) if gradient else None
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().iron_hashgrid_field_eval(C.byref(desc), flat.data_ptr(), n, a, b, table.detach().contiguous().data_ptr(),
                                                                packed.data_ptr(), out.data_ptr(), _lib.ptr(grad), _lib.stream_ptr(x.device)))
        out = out.reshape(*x.shape[:-1], n_out)
        return (out, grad.reshape(x.shape)) if gradient else out

    def as_callable(self, scale=None, offset=None):
        """The signed distance (column 0 of eval_fused) at scale * x + offset as an SDFCallable: the form to hand to RayTracer.forward
        and extract_fields_gpu, which work in the unit sphere while the field lives in the unit cube (scale = offset = 0.5)."""
        from .raytracer import SDFCallable
        self._fused_desc()
        return SDFCallable(lambda x: self.eval_fused(x, scale=scale, offset=offset)[..., 0])

    def as_traced(self, scale=None, offset=None):
        """The same signed distance as a HashFieldSDF handle: RayTracer.forward / occluded / the stage methods and raytrace_pixels
        trace it with the field evaluated inside the tracer's own kernels (csrc/hashgrid_trace.hip), bit for bit the
        results of as_callable(scale, offset) without its host round trips.  The handle holds this field, not a copy: an optimiser
        step is seen by the next trace."""
        from .raytracer import HashFieldSDF
        return HashFieldSDF(self, scale, offset)


def _map3(v, name):
    """None, a number or three numbers -> None or a float[3] for the C ABI"""
    if v is None:
        return None
    if torch.is_tensor(v):
        v = v.detach().cpu().tolist()
    vals = [float(v)] * 3 if isinstance(v, (int, float)) else [float(c) for c in v]
    if len(vals) != 3:
        raise _lib.IronError("TCNNSDF.eval_fused: %s must be a number or three numbers, got %r" % (name, v))
    return (C.c_float * 3)(*vals)
