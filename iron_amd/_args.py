"""Argument handling shared by the mesh chain's modules (mesh, mesh_distance, mesh_render, uv_unwrap, texture_bake; image_metrics
takes the workspace helper): choosing the device, numpy / tensor in -> checked contiguous device tensor out, and the sized
workspace of the C entries.  `what` is the calling module's name as its messages begin with it.  strict=True refuses CPU tensors
(iron_amd has no CPU path); strict=False uploads them, which is texture_bake's contract.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def refuse_cpu(what, *xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and not x.is_cuda:
            raise _lib.IronError("%s: CPU tensors are not accepted (iron_amd has no CPU path); pass CUDA tensors or numpy" % what)


def pick_device(what, *xs, strict=True) -> torch.device:
    """The device of the first CUDA tensor among xs, else the current GPU."""
    if strict:
        refuse_cpu(what, *xs)
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if strict and not torch.cuda.is_available():
        raise _lib.IronError("%s needs a GPU (iron_amd has no CPU path)" % what)
    return torch.device("cuda", torch.cuda.current_device())


def as_tensor(x, what="mesh", strict=True) -> torch.Tensor:
    """numpy (or a nested sequence) or tensor -> detached tensor, where it is."""
    if strict:
        refuse_cpu(what, x)
        return x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
    return torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x).detach()


def device_array(x, dtype, dev, name, shape_tail, strict=True, what="mesh") -> torch.Tensor:
    """x -> contiguous `dtype` tensor [n, *shape_tail] on dev; the shape is checked before the upload."""
    t = as_tensor(x, what, strict)
    if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail):
        raise _lib.IronError("%s must be [n, %s], got %s" % (name, ", ".join(str(k) for k in shape_tail), tuple(t.shape)))
    return t.to(device=dev, dtype=dtype).contiguous()


def face_array(faces, dev, what="mesh") -> torch.Tensor:
    """Integer faces [n, 3] -> contiguous int32 on dev."""
    f = as_tensor(faces, what)
    if f.dim() != 2 or f.shape[1] != 3:
        raise _lib.IronError("faces must be [n, 3], got %s" % (tuple(f.shape),))
    if f.is_floating_point() or f.dtype == torch.bool:
        raise _lib.IronError("faces must hold integer vertex indices, got %s" % f.dtype)
    f = f.to(device=dev)
    if f.dtype == torch.int64:  # an index beyond int32 must stay out of range (the build flags it), not wrap
        f = f.clamp(-1, (1 << 31) - 1)
    return f.to(torch.int32).contiguous()


def sized_workspace(fn, *size_args, device, tag=None) -> torch.Tensor:
    """The uint8 workspace of a C entry whose size `fn(*size_args, &bytes)` reports: fresh and call-scoped, or with `tag` the
    stream's growing buffer of _lib.workspace."""
    nb = C.c_size_t(0)
    _lib.check(fn(*size_args, C.byref(nb)))
    if tag is not None:
        return _lib.workspace(nb.value, device, tag)
    return torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=device)
