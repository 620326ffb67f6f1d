"""models/tcnn_fields.py on gfx950: the hash-grid SDF field `TCNNSDF`, without tiny-cuda-nn.

The reference builds `tcnn.Encoding(3, config["encoding"])` and `tcnn.Network(n_enc, n_out, config["network"])` from one JSON file.
Here the encoding is iron_amd.hashgrid.HashEncoding (HIP, fp32 table) and the network is its plain-torch equivalent: bias-free
nn.Linear layers (tiny-cuda-nn's MLPs carry no biases) with the configured activation.  forward / sdf / sdf_hidden_appearance /
gradient / get_all keep the reference's shapes and detach rules (tcnn_fields.py:26-66).  Points are taken in the unit cube, as the
reference hands them to tcnn (the encoding clamps to [0, 1]).

`TCNNRendering` and `TCNNNeRF` are not built: the reference's forwards are empty or mis-shaped (tcnn_fields.py:201-249)."""
from __future__ import annotations

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

    def forward(self, inputs):
        return self.model(inputs)

    def sdf(self, x):
        return self.forward(x)[..., :1]

    def sdf_hidden_appearance(self, x):
        return self.forward(x)

    def _forward_and_gradient(self, x, attached):
        """(forward(x), d sdf / dx); x becomes a leaf that requires grad, in place, as in the reference.  `attached` keeps the
        gradient differentiable with respect to the table and the head (the reference's create_graph)."""
        x.requires_grad_(True)
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
