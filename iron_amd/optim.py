"""FusedAdam: torch.optim.Adam's update (no weight decay, no amsgrad) for every parameter in one HIP launch per 80 tensors
(csrc/optim.hip: iron_adam_multi, include/iron_train.h).

It is a torch.optim.Optimizer: `param_groups` with a per-group `lr`, `step()`, `zero_grad()`, `state_dict()` and
`load_state_dict()` are the base class's, and the per-parameter state is torch.optim.Adam's own -- `step` (a float32 CPU scalar),
`exp_avg`, `exp_avg_sq` -- created the first time a parameter has a gradient, so a state saved by either optimiser loads into the
other.  A step fills a host table kept from construction and hands it to the library: nothing is uploaded, allocated (once the
moments exist) or waited for.

The kernel writes parameters behind autograd's back, so step() bumps the version counter of every parameter it wrote
(torch.autograd.graph.increment_version): SDFNetwork.hip_net()'s packed copies, PointLightNetwork.host_light() and the
"parameters changed between forward and backward" check of the HIP autograd functions all key on it.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def _adam_defaults() -> dict:
    # torch.optim.Adam's own group keys, so that a saved group loads into either optimiser
    return dict(torch.optim.Adam([torch.zeros(1)]).defaults)


class FusedAdam(torch.optim.Optimizer):
    """params_or_groups: an iterable of parameters or of {"params": [...], "lr": ...} groups, as torch.optim.Adam takes them.
    zero_grads=True: step() leaves every gradient it read exactly zero (in the same pass), for loops that keep their gradient
    buffers; a later step then sees a zero gradient, not None, so the parameter is updated and its step count advances."""

    def __init__(self, params_or_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, zero_grads=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid betas: %r" % (betas,))
        defaults = _adam_defaults()
        defaults.update(lr=lr, betas=tuple(betas), eps=eps)
        super().__init__(params_or_groups, defaults)
        self.zero_grads = bool(zero_grads)
        n = sum(len(g["params"]) for g in self.param_groups)
        self._table = (_lib.iron_adam_tensor * max(n, 1))()   # parameters are checked when they are stepped, as torch does

    @staticmethod
    def _check_param(p) -> None:
        if not p.is_cuda:
            raise _lib.IronError("FusedAdam: parameters must be CUDA (ROCm) tensors: iron_amd has no CPU path")
        if p.dtype != torch.float32:
            raise _lib.IronError("FusedAdam: parameters must be float32, got %s" % p.dtype)
        if not p.is_contiguous():
            raise _lib.IronError("FusedAdam: parameters must be contiguous, got shape %s with strides %s" % (tuple(p.shape), p.stride()))

    @staticmethod
    def _check_grad(p, g) -> None:
        if g.shape != p.shape or g.dtype != p.dtype or g.device != p.device:
            raise _lib.IronError("FusedAdam: gradient %s %s on %s does not match its parameter %s %s on %s"
                                 % (tuple(g.shape), g.dtype, g.device, tuple(p.shape), p.dtype, p.device))
        if g.is_sparse or not g.is_contiguous():
            raise _lib.IronError("FusedAdam: gradients must be dense and contiguous, got shape %s with strides %s"
                                 % (tuple(g.shape), g.stride() if not g.is_sparse else "sparse"))

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        n = sum(len(g["params"]) for g in self.param_groups)
        if hasattr(self, "_table") and n > len(self._table):
            self._table = (_lib.iron_adam_tensor * n)()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load_train()
        # one library call per (device, betas, eps); the reference's three groups share all of them
        calls = {}
        for group in self.param_groups:
            for k in ("weight_decay", "amsgrad", "maximize"):
                if group.get(k):
                    raise _lib.IronError("FusedAdam: %s is not built (the reference trains with torch.optim.Adam's defaults)" % k)
            lr = float(group["lr"])
            for p in group["params"]:
                if p.grad is None:
                    continue   # as torch: untouched, its step count does not advance
                self._check_param(p)
                self._check_grad(p, p.grad)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if m.shape != p.shape or v.shape != p.shape or not (m.is_contiguous() and v.is_contiguous()) or m.device != p.device \
                        or v.device != p.device or m.dtype != torch.float32 or v.dtype != torch.float32:
                    raise _lib.IronError("FusedAdam: the loaded exp_avg / exp_avg_sq do not match their parameter %s" % (tuple(p.shape),))
                st["step"] += 1
                key = (p.device, float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
                calls.setdefault(key, []).append((p, m, v, int(st["step"]), lr))
        for (dev, b1, b2, eps), items in calls.items():
            for i, (p, m, v, t, lr) in enumerate(items):
                e = self._table[i]
                e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr()
                e.numel, e.step, e.lr = p.numel(), t, lr
            with torch.cuda.device(dev):
                _lib.check_train(lib.iron_adam_multi(self._table, len(items), b1, b2, eps, 1 if self.zero_grads else 0,
                                                     _lib.stream_ptr(dev)))
            torch.autograd.graph.increment_version([p for p, *_ in items])
            if self.zero_grads:
                torch.autograd.graph.increment_version([p.grad for p, *_ in items])
        return loss
