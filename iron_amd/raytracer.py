"""Stage-2 forward render operators with the reference's surface (models/raytracer.py), backed by
the gfx950 HIP kernels in iron_amd/csrc (trace.hip, shade.hip, pointwise.hip).

Same names, arguments, result-dict keys / shapes / dtypes as the reference:
    RayTracer (:27-220), intersect_sphere (:223-237), Camera (:240-364), raytrace_pixels (:367-409),
    raytrace_camera (:542-590), render_normal_and_color (:593-662), render_camera (:778-814).
What differs is only HOW: one persistent kernel pipeline per call instead of a Python loop of
masked torch ops (no host sync inside the tracer), and a fused shading kernel when the render_fn
is the GGX one from iron_amd.rendering_func.

Built: the forward path including hole filling and silhouette edge sampling (locate_edge_points :421-506,
render_edge_pixels :665-729), and is_training=True (reparam_points :17-24, shading and edge blending
attached to the parameters through the differentiable HIP operators of iron_amd.autograd).
An SDF the library cannot evaluate itself is traced through SDFCallable(fn): the reference's evaluation schedule with fn supplying
the values, the per-ray bookkeeping between two calls in csrc/trace_any.hip.
A hash-grid field (TCNNSDF.as_traced() -> HashFieldSDF) is traced with the field evaluated inside the tracer's kernels
(csrc/hashgrid_trace.hip): the callable path's bits without its host round trips.
There is no CPU path: tensors must be CUDA (ROCm) fp32.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib

VERBOSE_MODE = False
RESULT_KEYS = ("convergent_mask", "points", "sdf", "distance")   # of RayTracer.forward's dictionary, in the order of the outputs


class SDFHandle:
    """The `sdf` callable raytrace_pixels hands to RayTracer.forward (reference: a lambda,
    raytracer.py:375).  Calling it evaluates the network; RayTracer recognises it and runs the fused
    HIP tracer on the wrapped SDFNetwork instead of calling it point batch by point batch."""

    def __init__(self, sdf_network):
        self.sdf_network = sdf_network

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.sdf_network.sdf(x)[..., 0]


class SDFCallable:
    """Marks `fn: Tensor[m,3] (CUDA, fp32, contiguous) -> Tensor[m]` as an SDF to be traced AS GIVEN: an analytic distance, a network
    of a shape the fused tracer refuses, a hash-grid field, a post-processed distance.  RayTracer.forward / sphere_tracing /
    ray_sampler / rootfind then make every evaluation the reference makes (raytracer.py:45-220), on the same points, by calling
    `fn` under torch.no_grad() on the current stream; the per-ray state machine between two evaluations runs in the HIP kernels of
    csrc/trace_any.hip.  The multi-rank form (phase_begin / forward_phased) does not take one."""

    def __init__(self, fn):
        if not callable(fn):
            raise _lib.IronError("SDFCallable needs a callable, got %s" % type(fn).__name__)
        self.fn = fn

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.fn(x)


class HashFieldSDF:
    """The hash-grid field `TCNNSDF` at scale * x + offset as an SDF the tracer evaluates INSIDE its own kernels
    (csrc/hashgrid_trace.hip); made by TCNNSDF.as_traced().  RayTracer.forward / occluded / sphere_tracing /
    ray_sampler / rootfind enqueue a fixed launch sequence for it and read nothing back (unless collect_stats=True); the results are,
    bit for bit, those of the same call on field.as_callable(scale, offset).  Holds the field itself, not a copy: the table is read
    in place and the head is repacked when a weight changed.  Calling the handle evaluates the field (column 0 of eval_fused).  The
    multi-rank form (phase_begin / forward_phased) does not take one."""

    def __init__(self, field, scale=None, offset=None):
        from .tcnn_fields import TCNNSDF, _map3
        if not isinstance(field, TCNNSDF):
            raise _lib.IronError("HashFieldSDF needs a TCNNSDF, got %s" % type(field).__name__)
        field._fused_desc()   # an unsupported head shape is refused here, by name
        self.field = field
        self.scale, self.offset = scale, offset
        self._a, self._b = _map3(scale, "scale"), _map3(offset, "offset")

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.field.eval_fused(x, scale=self.scale, offset=self.offset)[..., 0]

    def field_args(self, device):
        """(desc, map a, map b, table, packed) for the iron_hashgrid_trace* entries; the tensors must be kept alive over the call."""
        desc = self.field._fused_desc()
        table = self.field.sdf_encoding.params
        if table.device != device or table.dtype != torch.float32:
            raise _lib.IronError("HashFieldSDF: the table must be float32 on the rays' device; call .cuda() first")
        return desc, self._a, self._b, table.detach().contiguous(), self.field._fused_packed(desc, device)


def as_traceable(sdf):
    """What RayTracer takes for `sdf`: a HashFieldSDF, an SDFHandle or an SDFCallable passes, an iron_amd SDFNetwork (anything with
    `hip_net`) is wrapped in its handle.  None for anything else: the caller decides what a foreign object becomes."""
    if isinstance(sdf, (HashFieldSDF, SDFHandle, SDFCallable)):
        return sdf
    return SDFHandle(sdf) if hasattr(sdf, "hip_net") else None


_lin_cache = {}


def _linspace_steps(n_steps: int, device) -> torch.Tensor:
    # torch.linspace(0, 1, n_steps).float() exactly as raytracer.py:144-146 builds it; a fresh upload (tests restate the sampler with it)
    return torch.linspace(0, 1, steps=n_steps).float().to(device)


def _linspace_steps_cached(n_steps: int, device) -> torch.Tensor:
    """_linspace_steps, uploaded once per (n_steps, device): the one source of the sample steps for every arm, so that no tracer
    call copies anything from the host"""
    key = (int(n_steps), device)
    if key not in _lin_cache:
        _lin_cache[key] = _linspace_steps(n_steps, device)
    return _lin_cache[key]


def _per_ray(t, name, dtype, like):
    """work_mask (bool) / ray_index (int64) -> [n], contiguous, beside the rays `like`"""
    if t.dtype != dtype or not t.is_cuda:
        raise _lib.IronError("%s must be a CUDA %s tensor" % (name, "bool" if dtype == torch.bool else "int64"))
    t = t.reshape(-1).contiguous()
    if t.shape[0] != like.shape[0] or t.device != like.device:
        raise _lib.IronError("%s must have one entry per ray" % name)
    return t


def _ray_call(ray_o, ray_d, scalars, work_mask=None, ray_index=None):
    """The arguments of one tracer call, normalised for every public entry -> (o, d, scalars, work, index): ray_o and ray_d [n, 3],
    every per-ray scalar [n], all CUDA fp32; work_mask bool [n] and ray_index int64 [n], CUDA (None stays None: what that means is
    the entry's); everything contiguous, one entry per ray, on one device.  [n, 1] scalars, masks of any shape with n elements and
    non-contiguous tensors are taken.  The C entries read n entries from every array and can check none of this."""
    o = _lib.require_cuda_f32(ray_o, "ray_o").reshape(-1, 3)
    d = _lib.require_cuda_f32(ray_d, "ray_d").reshape(-1, 3)
    rest = [_lib.require_cuda_f32(t, "argument").reshape(-1) for t in scalars]
    for t in [d] + rest:
        if t.shape[0] != o.shape[0] or t.device != o.device:
            raise _lib.IronError("the ray arguments must have one entry per ray, on one device")
    work = None if work_mask is None else _per_ray(work_mask, "work_mask", torch.bool, o)
    index = None if ray_index is None else _per_ray(ray_index, "ray_index", torch.int64, o)
    return o, d, rest, work, index


def _outputs(alloc, n, dev, mask_only=False):
    """(mask, points, sdf, distance) of a call on n rays from torch.empty or torch.zeros; mask_only: the three behind it are None"""
    mask = alloc(n, dtype=torch.bool, device=dev)
    if mask_only:
        return mask, None, None, None
    return (mask, alloc((n, 3), dtype=torch.float32, device=dev), alloc(n, dtype=torch.float32, device=dev),
            alloc(n, dtype=torch.float32, device=dev))


def _ray_workspace(ws_bytes, n, dev, tag):
    """the call-scoped workspace of a tracer whose *_workspace_bytes answers 0 for a ray count it does not take"""
    if n > 0 and ws_bytes == 0:
        raise _lib.IronError("the tracer takes fewer than 2^31 - 1 rays per call; pass fewer rays (the callable tracer: chunk=)")
    return _lib.workspace(ws_bytes, dev, tag)


class _AnyTrace:
    """One reference call on an SDFCallable: the workspace, the evaluation buffer and the argument plumbing of iron_trace_any_*."""

    def __init__(self, tracer, sdf, o, d, stats):
        self.fn = sdf.fn
        self.o, self.d = o, d
        self.n, self.dev = o.shape[0], o.device
        self.thr = float(tracer.sdf_threshold)
        self.iters = int(tracer.sphere_tracing_iters)
        self.n_steps = int(tracer.n_steps)
        self.max_num_pts = int(tracer.max_num_pts)
        self.rays_per_call = self.max_num_pts // self.n_steps
        self.stats = stats
        self.lib = _lib.load()
        self.st = _lib.stream_ptr(self.dev)
        self.ws_bytes = self.lib.iron_trace_any_workspace_bytes(self.n)
        self.ws = _ray_workspace(self.ws_bytes, self.n, self.dev, "trace_any")
        self.wsp = self.ws.data_ptr()
        self.buf = torch.empty((max(self.n, 1), 3), dtype=torch.float32, device=self.dev)   # the next batch of the list stages
        self.words = (C.c_int64 * 2)()

    def evaluate(self, x, m):
        """fn on the first m points of x; its result is checked here, on the host, before any kernel reads it."""
        x = x[:m]
        with torch.no_grad():
            v = self.fn(x)
        if not torch.is_tensor(v) or not v.is_cuda or v.device != x.device:
            raise _lib.IronError("the sdf callable must return a CUDA tensor on the device of its argument")
        if v.dtype != torch.float32:
            raise _lib.IronError("the sdf callable must return float32, got %s" % (v.dtype,))
        if v.numel() != m:
            raise _lib.IronError("the sdf callable returned %d values for %d points" % (v.numel(), m))
        if self.stats is not None:
            self.stats["n_evals"] += m
            self.stats["n_calls"] += 1
        return v.reshape(-1).contiguous()

    def read(self):
        _lib.check(self.lib.iron_trace_any_read(self.wsp, self.ws_bytes, self.n, self.words, self.st))
        return int(self.words[0]), int(self.words[1])

    def sphere(self, near, far, work, points, sdf_out, dist):
        """raytracer.py:105-130 -> (list holding the unfinished rays, their count)."""
        lib, n = self.lib, self.n
        _lib.check(lib.iron_trace_any_start(self.o.data_ptr(), self.d.data_ptr(), near.data_ptr(), n, points.data_ptr(), dist.data_ptr(), self.st))
        values, m, cur, it = self.evaluate(points, n), n, -1, 0
        while True:
            advance = it < self.iters
            _lib.check(lib.iron_trace_any_sphere_step(values.data_ptr(), m, cur, int(advance), self.thr, self.d.data_ptr(), far.data_ptr(),
                                                      work.data_ptr(), n, points.data_ptr(), sdf_out.data_ptr(), dist.data_ptr(),
                                                      self.buf.data_ptr(), self.buf.shape[0], self.wsp, self.ws_bytes, self.st))
            cur = 0 if cur < 0 else 1 - cur
            m, _ = self.read()
            if not advance or m == 0:
                return cur, m
            it += 1
            values = self.evaluate(self.buf, m)

    def sphere_finish(self, far, work, sdf_out, dist, conv, unfinished=None):
        _lib.check(self.lib.iron_trace_any_sphere_finish(work.data_ptr(), far.data_ptr(), self.thr, self.n, sdf_out.data_ptr(), dist.data_ptr(),
                                                         conv.data_ptr(), _lib.ptr(unfinished), self.wsp, self.ws_bytes, self.st))

    def sampler(self, sel, m, a, b, lin, conv, points, sdf_out, dist):
        """raytracer.py:142-197 on the m rays of list `sel` (-1: rays 0..m-1 on [a, b] as given) -> (sampled rays, bisected rays,
        bisection iterations)."""
        lib, n, ns = self.lib, self.n, self.n_steps
        if self.rays_per_call < 1:
            raise _lib.IronError("the callable tracer samples whole rays per call: max_num_pts (%d) must be at least n_steps (%d)"
                                 % (self.max_num_pts, ns))
        _lib.check(lib.iron_trace_any_sampler_interval(sel, m, a.data_ptr(), b.data_ptr(), sdf_out.data_ptr(), dist.data_ptr(), n,
                                                       self.wsp, self.ws_bytes, self.st))
        block = min(m, self.rays_per_call)
        pts = torch.empty((block * ns, 3), dtype=torch.float32, device=self.dev)
        for k0 in range(0, m, block):
            nk = min(block, m - k0)
            _lib.check(lib.iron_trace_any_sampler_points(sel, m, k0, nk, ns, lin.data_ptr(), self.o.data_ptr(), self.d.data_ptr(), n,
                                                         pts.data_ptr(), pts.shape[0], self.wsp, self.ws_bytes, self.st))
            values = self.evaluate(pts, nk * ns)
            _lib.check(lib.iron_trace_any_sampler_reduce(m, k0, nk, ns, lin.data_ptr(), values.data_ptr(), n, self.wsp, self.ws_bytes, self.st))
        _lib.check(lib.iron_trace_any_sampler_gather(sel, m, self.o.data_ptr(), self.d.data_ptr(), n, conv.data_ptr(), points.data_ptr(),
                                                     sdf_out.data_ptr(), dist.data_ptr(), self.buf.data_ptr(), self.buf.shape[0], self.wsp,
                                                     self.ws_bytes, self.st))
        nb, wide = self.read()
        return m, nb, (self.bisect(nb, wide, conv, points, sdf_out, dist) if nb > 0 else 0)

    def bisect(self, nb, wide, conv, points, sdf_out, dist):
        """raytracer.py:204-220 on the nb slots the gather (or bisect_load) opened -> iterations."""
        lib, n = self.lib, self.n
        it = 0
        while wide:
            if it >= 256:   # fp32 brackets halve to nothing long before; the reference's loop would never end here
                raise _lib.IronError("the bisection does not close: the sdf callable returns NaN inside an open bracket, or a bracket is not finite")
            values = self.evaluate(self.buf, nb)
            _lib.check(lib.iron_trace_any_bisect_step(values.data_ptr(), nb, self.thr, self.o.data_ptr(), self.d.data_ptr(), n,
                                                      self.buf.data_ptr(), self.buf.shape[0], self.wsp, self.ws_bytes, self.st))
            _, wide = self.read()
            it += 1
        values = self.evaluate(self.buf, nb)
        _lib.check(lib.iron_trace_any_finish(values.data_ptr(), nb, self.o.data_ptr(), self.d.data_ptr(), n, _lib.ptr(conv), points.data_ptr(),
                                             sdf_out.data_ptr(), dist.data_ptr(), self.wsp, self.ws_bytes, self.st))
        return it


def _resolve_sdf_network(sdf, device):
    """The SDFNetwork behind the `sdf` callable of RayTracer.forward.  The reference hands over a lambda
    (`lambda x: sdf_network(x)[..., 0]`, raytracer.py:375); the HIP tracer needs the network itself, so:
      * an SDFHandle (what raytrace_pixels makes) or anything with an `.sdf_network` attribute is taken as is;
      * a bound method of a network, or a function whose closure / defaults hold exactly one network, is accepted
        only after a probe: the callable and the network must agree on 64 random points (a lambda that post-processes
        the distance would otherwise be traced wrongly without notice).
    Anything else is refused."""
    net = getattr(sdf, "sdf_network", None)
    if net is not None and hasattr(net, "hip_net"):
        return net
    cands = []
    owner = getattr(sdf, "__self__", None)
    if owner is not None and hasattr(owner, "hip_net"):
        cands.append(owner)
    for cell in (getattr(sdf, "__closure__", None) or ()):
        try:
            v = cell.cell_contents
        except ValueError:
            continue
        if hasattr(v, "hip_net") and hasattr(v, "sdf"):
            cands.append(v)
    for v in (getattr(sdf, "__defaults__", None) or ()):
        if hasattr(v, "hip_net") and hasattr(v, "sdf"):
            cands.append(v)
    cands = list({id(c): c for c in cands}.values())
    if len(cands) != 1:
        raise _lib.IronError("RayTracer.forward needs the sdf handle made by raytrace_pixels / SDFHandle(sdf_network), or a "
                             "callable that wraps exactly one iron_amd SDFNetwork; opaque sdf callables cannot run on the fused HIP tracer. "
                             "Wrap any other callable in SDFCallable(fn) to trace it as given.")
    net = cands[0]
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(64, 3, generator=g) * 1.6 - 0.8).to(device)
    got = torch.as_tensor(sdf(x)).reshape(-1)
    want = net.sdf(x)[..., 0].reshape(-1)
    if got.shape != want.shape or not torch.allclose(got, want, rtol=1e-5, atol=1e-6):
        raise _lib.IronError("the sdf callable does not return sdf_network.sdf(x)[..., 0] of the network it wraps; "
                             "pass SDFHandle(sdf_network)")
    return net


class _Arm:
    """One kind of SDF behind RayTracer.  RayTracer normalises the arguments (_ray_call), allocates the outputs (_outputs) and turns
    the stats words into last_stats; an arm makes its tracer's launches between the two, and its callers do not know which it is:
        trace(tr, o, d, near, far, work, chunk, out, collect_stats)   forward() / occluded() into out = (mask, points, sdf, distance);
                                                                      points None: the mask alone (an arm with mask_only)
        stage(tr, stage, o, d, ins, work, out, unfinished)            sphere_tracing / ray_sampler / rootfind = stage 0 / 1 / 2
        phase_begin(tr, ...) -> state, phase_finish(state)            the multi-rank pair, where the arm has it
    trace and stage return the call's stats words (a device tensor, or host counters) or None.  stats_fields names the words (None:
    not reported) and check(stats) raises on words that void the result."""
    stats_fields = ()
    mask_only = True    # occluded() has a shortened form that writes the mask alone
    phased = None       # what phase_begin calls the arm when it refuses it

    @staticmethod
    def check(stats) -> None:
        pass

    def phase_begin(self, *args):
        raise _lib.IronError("the multi-rank form (phase_begin / forward_phased) does not take %s: call forward() per rank" % self.phased)


class _NetworkArm(_Arm):
    """An SDFNetwork on the fused kernels of csrc/trace.hip: one iron_trace* call per operation."""
    stats_fields = _lib.TRACE_STATS_FIELDS

    def __init__(self, net):
        self.net = net

    @staticmethod
    def check(stats) -> None:
        """`reserved` counts k_sampler workgroups that gave up polling their work queue (csrc/trace.hip): never, unless the queue
        protocol is broken -- then the trace is incomplete and must not pass as a result."""
        if stats.get("reserved", 0):
            raise _lib.IronError("k_sampler left its work queue by the poll bound (%d workgroups): the trace is incomplete" % stats["reserved"])

    def trace(self, tr, o, d, near, far, work, chunk, out, collect_stats):
        conv, points, sdf_out, dist = out
        n, dev = o.shape[0], o.device
        if points is None and n == 0:
            return None
        lib = _lib.load()
        prm = tr._params(chunk)
        ws_bytes = (lib.iron_trace_workspace_bytes if points is not None else lib.iron_trace_occluded_workspace_bytes)(n, C.byref(prm))
        ws = _lib.workspace(ws_bytes, dev, "trace")
        stats = torch.zeros(8, dtype=torch.int64, device=dev) if collect_stats else None
        lin = _linspace_steps_cached(tr.n_steps, dev)
        head = (self.net.hip_net().handle, C.byref(prm), lin.data_ptr(), o.data_ptr(), d.data_ptr(), near.data_ptr(), far.data_ptr(),
                work.data_ptr(), n, conv.data_ptr())
        tail = (_lib.ptr(stats), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev))
        with torch.cuda.device(dev):
            if points is None:
                _lib.check(lib.iron_trace_occluded(*head, *tail))
            else:
                _lib.check(lib.iron_trace(*head, points.data_ptr(), sdf_out.data_ptr(), dist.data_ptr(), *tail))
        return stats

    def stage(self, tr, stage, o, d, ins, work, out, unfinished):
        """one iron_trace_stage call, i.e. the same persistent kernels forward() chains"""
        mask, points, sdf_out, dist = out
        n, dev = o.shape[0], o.device
        if n > 0:
            lib = _lib.load()
            prm = tr._params(0)
            ws_bytes = lib.iron_trace_workspace_bytes(n, C.byref(prm))
            ws = _lib.workspace(ws_bytes, dev, "trace")
            lin = _linspace_steps_cached(tr.n_steps, dev)
            with torch.cuda.device(dev):
                _lib.check(lib.iron_trace_stage(stage, self.net.hip_net().handle, C.byref(prm), lin.data_ptr(), o.data_ptr(), d.data_ptr(),
                                                _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), _lib.ptr(ins[3]), _lib.ptr(work), n,
                                                mask.data_ptr(), unfinished.data_ptr(), points.data_ptr(), sdf_out.data_ptr(),
                                                dist.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)))
        return None

    def phase_begin(self, tr, o, d, near, far, work, idx, n_chunks, chunk, collect_stats):
        n, dev = o.shape[0], o.device
        out = _outputs(torch.empty, n, dev)
        chunk_iters = torch.zeros(int(n_chunks), dtype=torch.int32, device=dev)
        lib = _lib.load()
        prm = tr._params(chunk)
        ws_bytes = lib.iron_trace_workspace_bytes(n, C.byref(prm))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)   # the state outlives the call: not the call-scoped workspace
        stats = torch.zeros(8, dtype=torch.int64, device=dev) if collect_stats else None
        lin = _linspace_steps_cached(tr.n_steps, dev)
        args = (self.net.hip_net().handle, C.byref(prm), lin.data_ptr(), o.data_ptr(), d.data_ptr(), near.data_ptr(),
                far.data_ptr(), work.data_ptr(), idx.data_ptr(), n, chunk_iters.data_ptr(), int(n_chunks),
                *[t.data_ptr() for t in out], _lib.ptr(stats), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev))
        state = {"args": args, "keep": (prm, lin, o, d, near, far, work, idx, ws), "n": n, "device": dev, "arm": self,
                 "out": dict(zip(RESULT_KEYS, out)), "chunk_iters": chunk_iters, "stats": stats}
        if n > 0:
            with torch.cuda.device(dev):
                _lib.check(lib.iron_trace_phase(0, *args))
        return state

    def phase_finish(self, state):
        if state["n"] > 0:
            with torch.cuda.device(state["device"]):
                _lib.check(_lib.load().iron_trace_phase(1, *state["args"]))


class _CallableArm(_Arm):
    """An opaque callable (SDFCallable): the same reference call, its evaluations made by the caller's function and everything between
    them by the kernels of csrc/trace_any.hip (_AnyTrace)."""
    stats_fields = ("n_evals", "n_calls", "n_sampler", "n_bisect", "n_bisect_iters")   # counted on the host
    mask_only = False   # occluded() is forward()'s mask: that form is not shortened
    phased = "an SDFCallable"

    def __init__(self, sdf):
        self.sdf = sdf

    def trace(self, tr, o, d, near, far, work, chunk, out, collect_stats):
        conv, points, sdf_out, dist = out
        n, dev = o.shape[0], o.device
        stats = dict.fromkeys(self.stats_fields, 0) if collect_stats else None
        lin = _linspace_steps_cached(tr.n_steps, dev)
        step = n if chunk is None or int(chunk) <= 0 else int(chunk)
        with torch.cuda.device(dev):
            for a in range(0, n, max(step, 1)):   # each chunk is a reference call of its own; slices of dim 0 stay contiguous
                b = min(n, a + step)
                run = _AnyTrace(tr, self.sdf, o[a:b], d[a:b], stats)
                c_near, c_far, c_work = near[a:b], far[a:b], work[a:b]
                c_conv, c_points, c_sdf, c_dist = conv[a:b], points[a:b], sdf_out[a:b], dist[a:b]
                sel, m = run.sphere(c_near, c_far, c_work, c_points, c_sdf, c_dist)
                run.sphere_finish(c_far, c_work, c_sdf, c_dist, c_conv)
                if m > 0:
                    _, nb, it = run.sampler(sel, m, c_near, c_far, lin, c_conv, c_points, c_sdf, c_dist)
                    if stats is not None:
                        stats["n_sampler"] += m
                        stats["n_bisect"] += nb
                        stats["n_bisect_iters"] += it
        return list(stats.values()) if collect_stats else None

    def stage(self, tr, stage, o, d, ins, work, out, unfinished):
        mask, points, sdf_out, dist = out
        n, dev = o.shape[0], o.device
        if n > 0:
            with torch.cuda.device(dev):
                run = _AnyTrace(tr, self.sdf, o, d, None)
                if stage == 0:
                    run.sphere(ins[0], ins[1], work, points, sdf_out, dist)
                    run.sphere_finish(ins[1], work, sdf_out, dist, mask, unfinished)
                elif stage == 1:
                    run.sampler(-1, n, ins[0], ins[1], _linspace_steps_cached(tr.n_steps, dev), mask, points, sdf_out, dist)
                    # the gather clears the rootless rays and the finish raises the bracketed ones: `mask` started as zeros
                else:
                    _lib.check(run.lib.iron_trace_any_bisect_load(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(),
                                                                  o.data_ptr(), d.data_ptr(), n, run.buf.data_ptr(), run.buf.shape[0],
                                                                  run.wsp, run.ws_bytes, run.st))
                    _, wide = run.read()
                    run.bisect(n, wide, None, points, sdf_out, dist)
        return None


class _HashFieldArm(_Arm):
    """A hash-grid field (HashFieldSDF): the same reference call with the field evaluated inside the kernels of
    csrc/hashgrid_trace.hip; a fixed launch sequence, nothing read back unless the stats are asked for."""
    stats_fields = tuple(None if k.startswith("reserved") else k for k in _lib.HASHGRID_TRACE_STATS_FIELDS)
    phased = "a HashFieldSDF"

    def __init__(self, sdf):
        self.sdf = sdf

    @staticmethod
    def check(stats) -> None:
        if stats.get("incomplete", 0):   # the callable tracer's own error, for the same cause
            raise _lib.IronError("the bisection does not close: the sdf callable returns NaN inside an open bracket, or a bracket is not finite")

    @staticmethod
    def _params(tr, chunk):
        if not 2 <= int(tr.n_steps) <= 4096:
            raise _lib.IronError("the hash-grid tracer takes n_steps in 2 .. 4096, got %r" % (tr.n_steps,))
        if int(tr.sphere_tracing_iters) < 0:
            raise _lib.IronError("sphere_tracing_iters must not be negative, got %r" % (tr.sphere_tracing_iters,))
        return tr._params(0 if chunk is None else max(int(chunk), 0))

    def _bind(self, lib, tr, prm, n, dev):
        """-> (the field and parameter arguments every iron_hashgrid_trace* entry begins with, the workspace and stream ones it ends
        with, what must stay alive over the call)"""
        desc, map_a, map_b, table, packed = self.sdf.field_args(dev)
        ws_bytes = lib.iron_hashgrid_trace_workspace_bytes(n, C.byref(prm))
        ws = _ray_workspace(ws_bytes, n, dev, "hashfield_trace")
        lin = _linspace_steps_cached(tr.n_steps, dev)
        return ((C.byref(desc), C.byref(prm), map_a, map_b, table.data_ptr(), packed.data_ptr(), lin.data_ptr()),
                (ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)), (desc, table, packed))

    def trace(self, tr, o, d, near, far, work, chunk, out, collect_stats):
        conv, points, sdf_out, dist = out
        n, dev = o.shape[0], o.device
        prm = self._params(tr, chunk)
        stats = torch.zeros(8, dtype=torch.int64, device=dev) if collect_stats else None
        if n > 0:
            lib = _lib.load()
            with torch.cuda.device(dev):
                field, tail, keep = self._bind(lib, tr, prm, n, dev)
                rays = (o.data_ptr(), d.data_ptr(), near.data_ptr(), far.data_ptr(), work.data_ptr(), n, conv.data_ptr())
                if points is None:
                    _lib.check(lib.iron_hashgrid_trace_occluded(*field, *rays, _lib.ptr(stats), *tail))
                else:
                    _lib.check(lib.iron_hashgrid_trace(*field, *rays, points.data_ptr(), sdf_out.data_ptr(), dist.data_ptr(),
                                                       _lib.ptr(stats), *tail))
        return stats

    def stage(self, tr, stage, o, d, ins, work, out, unfinished):
        """The stage methods are the debugging surface, not the frame's path: each reads the stats words back once, so that a
        bisection that does not close raises here as it does on the callable."""
        mask, points, sdf_out, dist = out
        n, dev = o.shape[0], o.device
        prm = self._params(tr, 0)
        if n == 0:
            return None
        lib = _lib.load()
        stats = torch.zeros(8, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            field, tail, keep = self._bind(lib, tr, prm, n, dev)
            _lib.check(lib.iron_hashgrid_trace_stage(stage, *field, o.data_ptr(), d.data_ptr(), _lib.ptr(ins[0]), _lib.ptr(ins[1]),
                                                     _lib.ptr(ins[2]), _lib.ptr(ins[3]), _lib.ptr(work), n, mask.data_ptr(),
                                                     unfinished.data_ptr(), points.data_ptr(), sdf_out.data_ptr(), dist.data_ptr(),
                                                     stats.data_ptr(), *tail))
        return stats


def _arm_of(sdf, device) -> _Arm:
    """The arm that serves `sdf`: the one place that asks what kind of SDF it is.  Anything but the two marked kinds must resolve to
    an SDFNetwork (_resolve_sdf_network and its probe) or is refused there."""
    if isinstance(sdf, SDFCallable):
        return _CallableArm(sdf)
    if isinstance(sdf, HashFieldSDF):
        return _HashFieldArm(sdf)
    return _NetworkArm(_resolve_sdf_network(sdf, device))


class RayTracer(nn.Module):
    def __init__(self, sdf_threshold=5.0e-5, sphere_tracing_iters=16, n_steps=128, max_num_pts=200000):
        super().__init__()
        self.sdf_threshold = sdf_threshold
        self.sphere_tracing_iters = sphere_tracing_iters
        self.n_steps = n_steps
        self.max_num_pts = max_num_pts
        self.last_stats: Optional[Dict[str, int]] = None

    def _params(self, chunk: int) -> _lib.iron_trace_params:
        p = _lib.iron_trace_params()
        p.sdf_threshold = float(self.sdf_threshold)
        p.sphere_tracing_iters = int(self.sphere_tracing_iters)
        p.n_steps = int(self.n_steps)
        p.chunk = int(chunk)
        return p

    def _stats_out(self, words, fields, check) -> None:
        """a call's stats words (None: it collected none) under the arm's field names -> last_stats (for a device tensor the one
        read-back), then the arm's check of them"""
        if words is None:
            return
        values = words.cpu().tolist() if torch.is_tensor(words) else words
        self.last_stats = {k: v for k, v in zip(fields, values) if k is not None}
        check(self.last_stats)

    def _trace(self, sdf, ray_o, ray_d, min_dis, max_dis, work_mask, chunk, collect_stats, mask_only):
        o, d, (near, far), work, _ = _ray_call(ray_o, ray_d, (min_dis, max_dis), work_mask)
        n, dev = o.shape[0], o.device
        if work is None:
            if not mask_only:
                raise _lib.IronError("work_mask must be a CUDA bool tensor")
            work = torch.ones(n, dtype=torch.bool, device=dev)
        arm = _arm_of(sdf, dev)
        out = _outputs(torch.empty, n, dev, mask_only and arm.mask_only)
        self._stats_out(arm.trace(self, o, d, near, far, work, chunk, out, collect_stats), arm.stats_fields, arm.check)
        return out[0] if mask_only else dict(zip(RESULT_KEYS, out))

    @torch.no_grad()
    def forward(self, sdf, ray_o, ray_d, min_dis, max_dis, work_mask, chunk: int = 0, collect_stats: bool = False):
        """One reference call = sphere_tracing + ray_sampler + rootfind on n rays (raytracer.py:45-103).

        `chunk` (extension): rays [k*chunk,(k+1)*chunk) are treated as separate reference calls
        (they share the bisection iteration count, raytracer.py:204-217); 0 = the whole batch."""
        return self._trace(sdf, ray_o, ray_d, min_dis, max_dis, work_mask, chunk, collect_stats, False)

    @torch.no_grad()
    def occluded(self, sdf, ray_o, ray_d, min_dis, max_dis, work_mask=None, collect_stats: bool = False):
        """Does each ray meet the surface in [min_dis, max_dis)?  bool [n], bit for bit forward(...)["convergent_mask"] for the same
        arguments: the reference tracer's own answer.  For an SDFNetwork (SDFHandle, or a callable forward() accepts) it is computed
        by the sphere and sampler kernels alone (iron_trace_occluded): the mask is final once the dense sampler has found, or not
        found, a first negative sample (raytracer.py:162-167), so no ray is bisected and no point, sdf or distance is returned.
        An SDFCallable is traced by forward() itself and its mask returned: that form is not shortened.  work_mask None: every ray.
        Bare callables and CPU tensors are refused as forward() refuses them."""
        return self._trace(sdf, ray_o, ray_d, min_dis, max_dis, work_mask, 0, collect_stats, True)

    # ---- the three stages as the reference exposes them (raytracer.py:105-220; tests/test_raytracer.py drives forward(), the
    # methods are public API of the class)
    def _stage(self, stage, sdf, ray_o, ray_d, in0, in1, in2=None, in3=None, work_mask=None):
        o, d, ins, work, _ = _ray_call(ray_o, ray_d, [t for t in (in0, in1, in2, in3) if t is not None], work_mask)
        n, dev = o.shape[0], o.device
        arm = _arm_of(sdf, dev)
        out = _outputs(torch.zeros, n, dev)   # zeros: what a stage leaves unwritten, and the callable arm's sampler relies on `mask` starting so
        unfinished = torch.zeros(n, dtype=torch.bool, device=dev)
        self._stats_out(arm.stage(self, stage, o, d, ins + [None] * (4 - len(ins)), work, out, unfinished), arm.stats_fields, arm.check)
        return (out[0], unfinished) + out[1:]

    @torch.no_grad()
    def sphere_tracing(self, sdf, ray_o, ray_d, min_dis, max_dis, work_mask):
        """raytracer.py:105-140 -> (convergent_mask, unfinished_mask_start, curr_start_points, curr_sdf_start, acc_start_dis)."""
        conv, unfinished, points, s, t = self._stage(0, sdf, ray_o, ray_d, min_dis, max_dis, work_mask=work_mask)
        return conv, unfinished, points, s, t

    @torch.no_grad()
    def ray_sampler(self, sdf, ray_o, ray_d, min_dis, max_dis):
        """raytracer.py:142-197: n_steps samples on [min_dis, max_dis] of every ray, first sign change, rootfind ->
        (rootfind_work_mask, sampler_pts, sampler_sdf, sampler_dis); rays without a bracketed root hold zeros."""
        mask, _, points, s, t = self._stage(1, sdf, ray_o, ray_d, min_dis, max_dis)
        return mask, points, s, t

    @torch.no_grad()
    def rootfind(self, sdf, f_low, f_high, d_low, d_high, ray_o, ray_d):
        """raytracer.py:199-220: bisection of every bracket while ANY of the call's brackets is wider than 2 x sdf_threshold ->
        (p_mid, d_mid, f_mid).  (The reference also narrows d_low / d_high / f_low / f_high in place; callers of this class do not
        read them afterwards and this method leaves them alone.)"""
        _, _, points, s, t = self._stage(2, sdf, ray_o, ray_d, f_low, f_high, d_low, d_high)
        return points, t, s

    @torch.no_grad()
    def phase_begin(self, sdf, ray_o, ray_d, min_dis, max_dis, work_mask, ray_index, n_chunks, chunk, collect_stats: bool = False):
        """First half of the multi-rank form of forward(): sphere tracing, dense sampling and each ray's own bisection
        (iron_trace_phase 0).  The rays of one reference chunk may live on several ranks, so the chunk-global bisection count
        (raytracer.py:204-217) has to be MAX-reduced over the ranks before the second half runs.  `ray_index` [n] int64 =
        position of each ray in the whole job (chunk id = ray_index // chunk).  Returns the state phase_finish() takes;
        state["chunk_iters"] (int32 [n_chunks], device) is the table to reduce in place."""
        o, d, (near, far), work, idx = _ray_call(ray_o, ray_d, (min_dis, max_dis), work_mask, ray_index)
        return _arm_of(sdf, o.device).phase_begin(self, o, d, near, far, work, idx, n_chunks, chunk, collect_stats)

    @torch.no_grad()
    def phase_finish(self, state):
        """Second half: every bracketed ray runs up to its chunk's (reduced) iteration count, then the final mid-point
        evaluation (iron_trace_phase 1).  Returns the result dict of forward()."""
        arm = state["arm"]
        arm.phase_finish(state)
        self._stats_out(state["stats"], arm.stats_fields, arm.check)
        return state["out"]

    @torch.no_grad()
    def forward_phased(self, sdf, ray_o, ray_d, min_dis, max_dis, work_mask, ray_index, n_chunks, chunk, reduce_fn,
                       collect_stats: bool = False):
        """phase_begin -> reduce_fn(int32[n_chunks]) (MAX over the ranks, in place: iron_amd.sharding.reduce_chunk_iters)
        -> phase_finish."""
        state = self.phase_begin(sdf, ray_o, ray_d, min_dis, max_dis, work_mask, ray_index, n_chunks, chunk, collect_stats)
        reduce_fn(state["chunk_iters"])
        return self.phase_finish(state)


@torch.no_grad()
def intersect_sphere(ray_o, ray_d, r):
    """raytracer.py:223-237 -> (mask bool[...], near[...], far[...])."""
    o = _lib.require_cuda_f32(ray_o, "ray_o")
    sh = list(o.shape[:-1])
    o = o.reshape(-1, 3)
    d = _lib.require_cuda_f32(ray_d, "ray_d").reshape(-1, 3)
    n = o.shape[0]
    mask = torch.empty(n, dtype=torch.bool, device=o.device)
    near = torch.empty(n, dtype=torch.float32, device=o.device)
    far = torch.empty(n, dtype=torch.float32, device=o.device)
    with torch.cuda.device(o.device):
        _lib.check(_lib.load().iron_intersect_sphere(o.data_ptr(), d.data_ptr(), n, float(r), mask.data_ptr(),
                                                     near.data_ptr(), far.data_ptr(), _lib.stream_ptr(o.device)))
    return mask.reshape(sh), near.reshape(sh), far.reshape(sh)


class Camera(object):
    def __init__(self, W, H, K, W2C):
        """W, H: int; K, W2C: 4x4 tensor (raytracer.py:240-252)."""
        self.W = W
        self.H = H
        self.K = K
        self.W2C = W2C
        self.device = self.K.device
        # 4x4 inverses on the host in fp32 (same LAPACK path as the reference's CPU run), kept on K's device
        self.K_inv = torch.inverse(K.detach().float().cpu()).to(self.device)
        self.C2W = torch.inverse(W2C.detach().float().cpu()).to(self.device)
        self._kinv_host = (C.c_float * 9)(*self.K_inv[:3, :3].cpu().reshape(-1).tolist())
        self._c2w_host = (C.c_float * 12)(*self.C2W[:3, :4].cpu().reshape(-1).tolist())
        self._w2c_rot_host = (C.c_float * 9)(*W2C.detach().float()[:3, :3].cpu().reshape(-1).tolist())
        self._w2c_host16 = (C.c_float * 16)(*W2C.detach().float().cpu().reshape(-1).tolist())
        self._k_host16 = (C.c_float * 16)(*K.detach().float().cpu().reshape(-1).tolist())

    def get_rays(self, uv):
        """uv [..., 2] -> ray_o [...,3], ray_d [...,3] (unit), ray_d_norm [...] (raytracer.py:254-286)."""
        uvc = _lib.require_cuda_f32(uv, "uv")
        sh = list(uvc.shape[:-1])
        uvc = uvc.reshape(-1, 2)
        n = uvc.shape[0]
        dev = uvc.device
        ray_o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ray_d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        nrm = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().iron_camera_rays(self._kinv_host, self._c2w_host, uvc.data_ptr(), n, ray_o.data_ptr(),
                                                    ray_d.data_ptr(), nrm.data_ptr(), _lib.stream_ptr(dev)))
        return ray_o.reshape(sh + [3]), ray_d.reshape(sh + [3]), nrm.reshape(sh)

    def get_camera_origin(self, prefix_shape=None):
        ray_o = self.C2W[:3, 3]
        if prefix_shape is not None:
            prefix_shape = list(prefix_shape)
            ray_o = ray_o.view([1] * len(prefix_shape) + [3]).expand(prefix_shape + [3])
        return ray_o

    def get_uv(self):
        """Pixel centres [H,W,2] (raytracer.py:300-303)."""
        # built on the device (a fresh tensor per call, as in the reference: callers write into it): the reference's numpy meshgrid
        # + .to(device) is a synchronous 5 MB host copy per 800x800 frame that also drains the stream -- the next frame's trace could
        # not be queued behind the current frame's shading (1.9 ms of idle GPU per frame, tools/host_timeline.py)
        if self.device.type != "cuda":
            u, v = np.meshgrid(np.arange(self.W), np.arange(self.H))
            return torch.from_numpy(np.stack((u, v), axis=-1).astype(np.float32)).to(self.device) + 0.5
        u = torch.arange(self.W, dtype=torch.float32, device=self.device) + 0.5
        v = torch.arange(self.H, dtype=torch.float32, device=self.device) + 0.5
        return torch.stack((u.unsqueeze(0).expand(self.H, self.W), v.unsqueeze(1).expand(self.H, self.W)), dim=-1)

    def project(self, points):
        """points [...,3] -> uv [...,2] (raytracer.py:305-325): homogeneous point through W2C and K, perspective division.  Written
        as broadcast products and sums (4-term dot products; differentiable): a [n,4] x [4,4] torch.matmul would go to a BLAS
        library for 16 multiply-adds per point."""
        sh = list(points.shape[:-1])
        p = points.reshape(-1, 3)
        ph = torch.cat([p, torch.ones_like(p[:, :1])], dim=1)
        cam = (ph.unsqueeze(1) * self.W2C.unsqueeze(0)).sum(dim=-1)
        img = (cam.unsqueeze(1) * self.K.unsqueeze(0)).sum(dim=-1)
        return (img[:, :2] / img[:, 2:3]).view(sh + [2])

    def _crop_origin(self, trgt_W, trgt_H, center_crop, ul_corner):
        """(column, row) of the crop window's upper-left pixel.  The random draws consume numpy's global generator exactly
        like raytracer.py:331-338: column first, then row."""
        if ul_corner is not None:
            return int(ul_corner[0]), int(ul_corner[1])
        if center_crop:  # a window around the centre, pushed up / left by less than 256 pixels
            jitter = [int(np.random.randint(0, 256)) for _ in range(2)]
            return self.W // 2 - trgt_W // 2 - jitter[0], self.H // 2 - trgt_H // 2 - jitter[1]
        return int(np.random.randint(0, self.W - trgt_W)), int(np.random.randint(0, self.H - trgt_H))

    def crop_region(self, trgt_W, trgt_H, center_crop=False, ul_corner=None, image=None, mask=None):
        """raytracer.py:327-351 -> (camera, image, mask): the sub-window's camera is this one with the principal point moved
        by the window origin; `image` / `mask` ([H,W,...]) are cut to the same window."""
        col0, row0 = self._crop_origin(trgt_W, trgt_H, center_crop, ul_corner)
        principal_shift = torch.zeros_like(self.K)
        principal_shift[0, 2] = col0
        principal_shift[1, 2] = row0
        sub = Camera(trgt_W, trgt_H, self.K - principal_shift, self.W2C.clone())
        window = (slice(row0, row0 + trgt_H), slice(col0, col0 + trgt_W))
        cut = []
        for label, img in (("image", image), ("mask", mask)):
            if img is not None:
                if img.shape[0] != self.H or img.shape[1] != self.W:
                    raise AssertionError("%s size does not match specified size" % label)
                img = img[window]
            cut.append(img)
        return sub, cut[0], cut[1]

    def resize(self, factor, image=None):
        """raytracer.py:353-364 -> (camera, image): intrinsics rows 0 / 1 scaled by the (integer-truncated) size ratio; `image`
        ([H,W] or [H,W,C]; tensor or numpy array) resampled to the new size the way cv2.INTER_AREA does when shrinking: every
        output pixel is the coverage-weighted mean of the input pixels its footprint overlaps (exact box average for integer
        ratios).  cv2 is not installed in the build container, so this resampling is parity-unpinned against OpenCV itself
        (tests hold it to the closed form).  Enlarging (factor > 1), where INTER_AREA degenerates to an interpolation, uses
        bilinear interpolation."""
        new_H, new_W = int(self.H * factor), int(self.W * factor)
        K = self.K.clone()
        for row, ratio in ((0, new_W / self.W), (1, new_H / self.H)):
            K[row, :3] = K[row, :3] * ratio
        cam = Camera(new_W, new_H, K, self.W2C.clone())
        if image is None:
            return cam, None
        as_numpy = isinstance(image, np.ndarray)
        img = torch.as_tensor(image)
        orig_dtype = img.dtype
        x = img.to(torch.float64 if img.dtype == torch.float64 else torch.float32)
        squeeze = x.dim() == 2
        if squeeze:
            x = x.unsqueeze(-1)
        if x.shape[0] != self.H or x.shape[1] != self.W:
            raise AssertionError("image size does not match specified size")
        if new_H <= self.H and new_W <= self.W:
            x = torch.einsum("ih,hwc->iwc", _area_weights(self.H, new_H, x), x)
            x = torch.einsum("jw,iwc->ijc", _area_weights(self.W, new_W, x), x)
        else:
            x = torch.nn.functional.interpolate(x.permute(2, 0, 1).unsqueeze(0), size=(new_H, new_W), mode="bilinear",
                                                align_corners=False)[0].permute(1, 2, 0)
        if squeeze:
            x = x[..., 0]
        if not orig_dtype.is_floating_point:
            x = x.round().clamp(torch.iinfo(orig_dtype).min, torch.iinfo(orig_dtype).max)
        x = x.to(orig_dtype)
        return cam, (x.cpu().numpy() if as_numpy else x)


def _area_weights(n_in: int, n_out: int, like: torch.Tensor) -> torch.Tensor:
    """[n_out, n_in] coverage weights of the shrinking box filter: output cell i covers [i s, (i+1) s) of the input, s = n_in / n_out."""
    s = n_in / n_out
    lo = torch.arange(n_out, dtype=torch.float64).unsqueeze(1) * s
    hi = lo + s
    j = torch.arange(n_in, dtype=torch.float64).unsqueeze(0)
    w = (torch.minimum(hi, j + 1.0) - torch.maximum(lo, j)).clamp_min(0.0) / s
    return w.to(dtype=like.dtype, device=like.device)


@torch.no_grad()
def raytrace_pixels(sdf_network, raytracer, uv, camera, mask=None, max_num_rays=200000):
    """raytracer.py:367-409.  All rays go through ONE tracer launch sequence; `max_num_rays` only keeps
    its reference meaning as the bisection-count chunk."""
    if mask is None:
        mask = torch.ones_like(uv[..., 0]).bool()
    dots_sh = list(uv.shape[:-1])
    ray_o, ray_d, ray_d_norm = camera.get_rays(uv)
    sdf = as_traceable(sdf_network)   # TCNNSDF.as_traced() and the other handles pass through
    if sdf is None:  # a foreign network: traced through its own forward, as the reference does (raytracer.py:375)
        sdf = SDFCallable(lambda x: sdf_network(x)[..., 0])
    o, d = ray_o.reshape(-1, 3), ray_d.reshape(-1, 3)
    hit, near, far = intersect_sphere(o, d, r=1.0)
    results = raytracer(sdf, o, d, near, far, hit & mask.reshape(-1), chunk=max_num_rays,
                        collect_stats=VERBOSE_MODE)
    results["depth"] = results["distance"] / ray_d_norm.reshape(-1)
    merged = {}
    for k, v in results.items():
        v = v.reshape(dots_sh + [-1])
        merged[k] = v[..., 0] if v.shape[-1] == 1 else v
    merged.update({"uv": uv, "ray_o": ray_o, "ray_d": ray_d, "ray_d_norm": ray_d_norm})
    return merged


def _require_iron_network(sdf_network, what, attr=None):
    """Tracing takes any network (raytrace_pixels falls back to SDFCallable); the edge walk and the shading need the gradient and
    feature kernels of an iron_amd SDFNetwork."""
    if not hasattr(sdf_network, "hip_net" if attr is None else attr):
        raise _lib.IronError("%s needs an iron_amd SDFNetwork, got %s: a foreign network can be traced "
                             "(raytrace_pixels, raytrace_camera(detect_edges=False)) but not walked or shaded" % (what, type(sdf_network).__name__))


def unique(x, dim=-1):
    """raytracer.py:412-419: the unique elements of x along `dim` and, for each, the index of its FIRST occurrence in x
    (a min-reduction over the positions that map to each unique element: deterministic on the GPU)."""
    values, group = torch.unique(x, return_inverse=True, dim=dim)
    n = x.size(dim)
    position = torch.arange(n, dtype=group.dtype, device=group.device)
    first = torch.full((values.size(dim),), n, dtype=group.dtype, device=group.device)
    return values, first.scatter_reduce_(0, group.reshape(-1), position, reduce="amin", include_self=True)


def morph_closing3x3(depth):
    """kornia.morphology.closing(depth[None,None], ones(3,3))[0,0] (raytracer.py:554-557) on an [H,W] image."""
    x = _lib.require_cuda_f32(depth, "depth")
    H, W = x.shape
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().iron_morph_closing3x3(x.data_ptr(), H, W, tmp.data_ptr(), out.data_ptr(),
                                                     _lib.stream_ptr(x.device)))
    return out


def sobel_magnitude(depth):
    """kornia.filters.sobel(depth[None,None])[0,0] (raytracer.py:569) on an [H,W] image."""
    x = _lib.require_cuda_f32(depth, "depth")
    H, W = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().iron_sobel_magnitude(x.data_ptr(), H, W, out.data_ptr(), _lib.stream_ptr(x.device)))
    return out


def _edge_walk_fused(sdf_network, start, cam_o, max_step, step_size, dot_threshold):
    """The whole walk in one kernel (iron_edge_walk); None when the network cannot run on the h2 core."""
    n = start.shape[0]
    dev = start.device
    points = torch.empty_like(start)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    cam = (C.c_float * 3)(*cam_o.reshape(-1).tolist())
    with torch.cuda.device(dev):
        rc = _lib.load().iron_edge_walk(sdf_network.hip_net().handle, start.data_ptr(), n, cam, int(max_step), float(step_size),
                                        float(dot_threshold), points.data_ptr(), found.data_ptr(), _lib.stream_ptr(dev))
    if rc == _lib.IRON_ERR_UNSUPPORTED:
        return None
    _lib.check(rc)
    return points, found.bool()


@torch.no_grad()
def locate_edge_points(camera, walk_start_points, sdf_network, max_step, step_size, dot_threshold, max_num_rays=200000,
                       mask=None):
    """raytracer.py:421-506: walk the masked surface points along the surface towards the silhouette
    (|n.v| <= dot_threshold), then keep one edge point per pixel.

    Every point is an independent state machine (a found point is never moved again), so all candidates
    advance together through <= max_step+1 get_all launches; `max_num_rays` has no effect on the result
    (the reference only uses it to bound memory) and is accepted for signature parity."""
    _require_iron_network(sdf_network, "locate_edge_points (detect_edges=True)")
    if mask is None:
        mask = torch.ones_like(walk_start_points[..., 0]).bool()
    dev = walk_start_points.device
    cur = _lib.require_cuda_f32(walk_start_points[mask], "walk_start_points").reshape(-1, 3).clone()
    found = torch.zeros(cur.shape[0], dtype=torch.bool, device=dev)
    if cur.shape[0] > 0:
        cam_o = camera.get_camera_origin().reshape(1, 3)
        fused = _edge_walk_fused(sdf_network, cur, cam_o, max_step, step_size, dot_threshold)
        if fused is not None:
            cur, found = fused
        else:  # network not on the h2 core: the same walk, one get_all launch per step
            for i in range(max_step + 1):
                sdf, grad = sdf_network.get_sdf_and_gradient(cur)
                view = cam_o - cur
                view = view / (view.norm(dim=-1, keepdim=True) + 1e-10)
                nrm = grad / (grad.norm(dim=-1, keepdim=True) + 1e-10)
                dot = (nrm * view).sum(dim=-1)
                # a found point keeps its position, hence its dot: OR-ing equals the reference's masked update
                found |= ~(dot.abs() > dot_threshold)
                if i >= max_step or (i % 4 == 3 and bool(found.all())):
                    break
                walk = nrm - view / dot.unsqueeze(-1)
                walk = walk / (walk.norm(dim=-1, keepdim=True) + 1e-10)
                walk = walk - sdf * nrm
                cur = torch.where(found.unsqueeze(-1), cur, cur + step_size * walk)
    # one edge point per pixel: the first found candidate that projects into it (raytracer.py:481-500), iron_edge_pixels
    n_cand = cur.shape[0]
    n_pix = camera.H * camera.W
    first = torch.full((n_pix,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    if n_cand > 0:
        cur = cur.contiguous()
        uv_all = torch.empty((n_cand, 2), dtype=torch.float32, device=dev)
        flags = found.contiguous().view(torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().iron_edge_pixels(cur.data_ptr(), flags.data_ptr(), n_cand, camera._w2c_host16, camera._k_host16, camera.H,
                                                    camera.W, uv_all.data_ptr(), first.data_ptr(), _lib.stream_ptr(dev)))
    edge_mask = (first != 2 ** 31 - 1).reshape(camera.H, camera.W)
    update_pixels = edge_mask.reshape(-1).nonzero().reshape(-1)          # ascending: the order torch.unique returns
    if update_pixels.shape[0] > 0:
        winner = first[update_pixels].long()
        edge_points, edge_uv = cur[winner], uv_all[winner]
    else:
        edge_points = torch.zeros((0, 3), dtype=torch.float32, device=dev)
        edge_uv = torch.zeros((0, 2), dtype=torch.float32, device=dev)
    out = {"edge_mask": edge_mask, "edge_points": edge_points, "edge_uv": edge_uv, "edge_pixel_idx": update_pixels}
    if VERBOSE_MODE:  # the reference's debug maps (raytracer.py:515-537)
        walk_edge_found_mask = torch.zeros_like(mask)
        walk_edge_found_mask[mask] = found
        edge_angles = torch.zeros(camera.H, camera.W, dtype=torch.float32, device=dev)
        edge_sdf = torch.zeros(camera.H, camera.W, 1, dtype=torch.float32, device=dev)
        if update_pixels.shape[0] > 0:
            view = camera.get_camera_origin().reshape(1, 3) - edge_points
            view = view / (view.norm(dim=-1, keepdim=True) + 1e-10)
            sdf_vals, grads = sdf_network.get_sdf_and_gradient(edge_points)
            nrm = grads / (grads.norm(dim=-1, keepdim=True) + 1e-10)
            edge_angles.view(-1)[update_pixels] = torch.rad2deg(torch.acos((view * nrm).sum(dim=-1)))
            edge_sdf.view(-1)[update_pixels] = sdf_vals.squeeze(-1)
        out.update({"walk_edge_found_mask": walk_edge_found_mask, "edge_angles": edge_angles, "edge_sdf": edge_sdf})
    return out


def fill_depth_holes(results):
    """The fill_holes branch of raytrace_camera (raytracer.py:554-564), in place and without a host round trip:
    morphological closing of the depth image, then -- only if that turns some non-convergent pixel into a hit -- depth at
    the new hits, mask = closed depth > 1e-2, and distance / points recomputed from the depth for every pixel
    (iron_morph_closing3x3 + iron_fill_holes)."""
    depth = results["depth"]
    closed = morph_closing3x3(depth)
    dev = depth.device
    n = depth.numel()
    conv = results["convergent_mask"]
    if not conv.is_contiguous():
        conv = results["convergent_mask"] = conv.contiguous()
    for k in ("depth", "distance", "points"):
        if not results[k].is_contiguous():
            results[k] = results[k].contiguous()
    ray_o = _lib.require_cuda_f32(results["ray_o"], "ray_o")
    ray_d = _lib.require_cuda_f32(results["ray_d"], "ray_d")
    nrm = _lib.require_cuda_f32(results["ray_d_norm"], "ray_d_norm")
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().iron_fill_holes(closed.data_ptr(), ray_o.data_ptr(), ray_d.data_ptr(), nrm.data_ptr(), n,
                                               results["depth"].data_ptr(), conv.data_ptr(), results["distance"].data_ptr(),
                                               results["points"].data_ptr(), flag.data_ptr(), _lib.stream_ptr(dev)))


def silhouette_candidates(results):
    """raytracer.py:566-570: hit pixels whose depth changes by more than 1e-2 per pixel (normalised sobel magnitude)."""
    magnitude = sobel_magnitude(results["depth"])
    return magnitude, (magnitude > 1e-2) & results["convergent_mask"]


@torch.no_grad()
def raytrace_camera(camera, sdf_network, raytracer, max_num_rays=200000, fill_holes=False, detect_edges=False,
                    depth_edge_mask=None):
    """raytracer.py:542-590.  `depth_edge_mask` (extension, tests only) replaces the sobel-derived candidate mask."""
    results = raytrace_pixels(sdf_network, raytracer, camera.get_uv(), camera, max_num_rays=max_num_rays)
    results["depth"] *= results["convergent_mask"].float()
    if fill_holes:
        fill_depth_holes(results)
    if detect_edges:
        locate_silhouette(results, camera, sdf_network, max_num_rays, depth_edge_mask)
    return results


def locate_silhouette(results, camera, sdf_network, max_num_rays=200000, depth_edge_mask=None):
    """The detect_edges branch (raytracer.py:566-588): candidates -> surface walk -> one edge point per pixel; edge pixels
    leave the convergent mask.  Shared by raytrace_camera and the sharded renderer's post-pass."""
    magnitude = None
    if depth_edge_mask is None:
        magnitude, depth_edge_mask = silhouette_candidates(results)
    results.update(locate_edge_points(camera, results["points"], sdf_network, max_step=16, step_size=1e-3,
                                      dot_threshold=5e-2, max_num_rays=max_num_rays, mask=depth_edge_mask))
    results["convergent_mask"] &= ~results["edge_mask"]
    if VERBOSE_MODE and magnitude is not None:
        results["depth_grad_norm"], results["depth_edge_mask"] = magnitude, depth_edge_mask


def reparam_points(nondiff_points, nondiff_grads, nondiff_trgt_dirs, diff_sdf_vals):
    """raytracer.py:17-24: re-attach a traced (non-differentiable) surface point to the SDF parameters.  Moving the
    parameters moves the zero level set along `nondiff_trgt_dirs` by -d(sdf) / (grad . dir); the residual below is zero in
    value and carries exactly that derivative.  The slope is clamped at 1e-4 (rays grazing the surface)."""
    slope = (nondiff_grads * nondiff_trgt_dirs).sum(dim=-1, keepdim=True).clamp(min=1e-4)
    residual = diff_sdf_vals - diff_sdf_vals.detach()
    return nondiff_points - (nondiff_trgt_dirs / slope) * residual


def render_normal_and_color(results, sdf_network, color_network_dict, render_fn, is_training=False, max_num_pts=320000):
    """raytracer.py:593-662; mutates `results`.  With the GGX render_fn of iron_amd.rendering_func the whole
    body (get_all -> normalise -> materials -> GGX -> scatter) is one fused kernel launch; any other callable
    gets the reference's generic gather / get_all / render_fn / reshape flow (chunked by max_num_pts).
    is_training=True takes the generic flow under grad mode: get_all attached to the SDF parameters,
    reparam_points, render_fn over the differentiable HIP operators (iron_amd.autograd)."""
    _require_iron_network(sdf_network, "render_normal_and_color", "get_all")
    dots_sh = list(results["convergent_mask"].shape)
    fused = getattr(render_fn, "iron_fused_ggx", None)
    if fused is not None and not is_training:
        out = fused(results, sdf_network, color_network_dict)
        for k, v in out.items():
            v = v.reshape(dots_sh + [-1])
            results[k] = v.squeeze(-1) if v.shape[-1] == 1 else v
        return

    merge = None
    for points_split, ray_d_split, ray_o_split, mask_split in zip(
            torch.split(results["points"].reshape(-1, 3), max_num_pts, dim=0),
            torch.split(results["ray_d"].reshape(-1, 3), max_num_pts, dim=0),
            torch.split(results["ray_o"].reshape(-1, 3), max_num_pts, dim=0),
            torch.split(results["convergent_mask"].reshape(-1), max_num_pts, dim=0)):
        # the hits listed ONCE (x[mask] lists them again at every use: a nonzero and a host sync each)
        hit_index = mask_split.nonzero(as_tuple=True)[0]
        if hit_index.numel() > 0:
            points_split, ray_d_split, ray_o_split = (x.index_select(0, hit_index) for x in (points_split, ray_d_split, ray_o_split))
            sdf_split, feature_split, normal_split = sdf_network.get_all(points_split, is_training=is_training)
            if is_training:
                points_split = reparam_points(points_split, normal_split.detach(), -ray_d_split.detach(), sdf_split)
        else:
            e = torch.zeros(0, dtype=torch.float32, device=points_split.device)
            points_split = ray_d_split = ray_o_split = normal_split = feature_split = e
        with torch.set_grad_enabled(is_training):
            if getattr(render_fn, "iron_takes_hit_index", False):
                r = render_fn(mask_split, color_network_dict, ray_o_split, ray_d_split, points_split, normal_split, feature_split,
                              hit_index=hit_index)
            else:
                r = render_fn(mask_split, color_network_dict, ray_o_split, ray_d_split, points_split, normal_split,
                              feature_split)
        if merge is None:
            merge = {k: [v] for k, v in r.items()} if r is not None else {}
        else:
            for k, v in r.items():
                merge[k].append(v)
    for k, parts in merge.items():
        v = torch.cat(parts, dim=0).reshape(dots_sh + [-1])
        results[k] = v.squeeze(-1) if v.shape[-1] == 1 else v


PIXEL_RADIUS = 0.707  # a pixel taken as a disc of radius sqrt(2)/2 (raytracer.py:691-693)


def _side_rays(results_of, n_edge, sdf_network, raytracer, camera, side_uv, color_network_dict, render_fn, is_training):
    """Trace + shade the 2n side samples ([2n,2] uv: positive side first).  One launch sequence for both sides: with
    chunk = n the tracer keeps rays [0,n) and [n,2n) apart as two reference calls (own bisection counts,
    raytracer.py:204-217) and shading is per point, so this equals the reference's two raytrace_pixels + two
    render_normal_and_color calls."""
    if n_edge <= 200000:
        both = raytrace_pixels(sdf_network, raytracer, side_uv, camera, max_num_rays=n_edge)
        render_normal_and_color(both, sdf_network, color_network_dict, render_fn, is_training=is_training)
        return both
    halves = []
    for part in (side_uv[:n_edge], side_uv[n_edge:]):
        r = raytrace_pixels(sdf_network, raytracer, part, camera)
        render_normal_and_color(r, sdf_network, color_network_dict, render_fn, is_training=is_training)
        halves.append(r)
    return {k: torch.cat([halves[0][k], halves[1][k]], dim=0) for k in halves[0]}


def render_edge_pixels(results, camera, sdf_network, raytracer, color_network_dict, render_fn, is_training=False):
    """raytracer.py:665-729: one ray on each side of every edge pixel, blended by the area the silhouette cuts off the pixel
    disc; mutates `results` (color, normal, uv, points at the edge pixels; edge_pos_neg_normal).
    Inference: iron_edge_sides -> side-ray trace + shade -> iron_edge_blend, no elementwise torch chain.
    is_training=True (row f-2): the same geometry as torch expressions, because the blend weight and both side colours
    carry gradients to the SDF parameters (the edge point is re-attached with reparam_points)."""
    n_edge = int(results["edge_uv"].shape[0])
    if n_edge == 0:
        results["edge_pos_neg_normal"] = results["normal"].new_zeros((0, 3))
        return
    if is_training:
        return _render_edge_pixels_training(results, camera, sdf_network, raytracer, color_network_dict, render_fn)
    _edge_blend(results, _edge_side_colours(results, camera, sdf_network, raytracer, color_network_dict, render_fn))


def _edge_side_colours(results, camera, sdf_network, raytracer, color_network_dict, render_fn):
    """First half of the inference edge pass: edge gradients -> the two side samples of every edge pixel (iron_edge_sides) -> traced
    and shaded.  Reads the edge_* keys only; returns what the blend needs."""
    n_edge = int(results["edge_uv"].shape[0])
    dev = results["edge_uv"].device
    edge_points = _lib.require_cuda_f32(results["edge_points"], "edge_points")
    edge_uv = _lib.require_cuda_f32(results["edge_uv"], "edge_uv")
    pixel = results["edge_pixel_idx"].contiguous()
    _, edge_grads = sdf_network.get_sdf_and_gradient(edge_points)
    edge_grads = edge_grads.contiguous()
    side_uv = torch.empty((2 * n_edge, 2), dtype=torch.float32, device=dev)
    weight = torch.empty(n_edge, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.iron_edge_sides(edge_uv.data_ptr(), edge_grads.data_ptr(), camera._w2c_rot_host, n_edge, side_uv.data_ptr(),
                                       weight.data_ptr(), _lib.stream_ptr(dev)))
    both = _side_rays(results, n_edge, sdf_network, raytracer, camera, side_uv, color_network_dict, render_fn, False)
    side_color = _lib.require_cuda_f32(both["color"], "color").reshape(2 * n_edge, 3)
    ctx = {"n_edge": n_edge, "edge_points": edge_points, "edge_uv": edge_uv, "pixel": pixel, "edge_grads": edge_grads, "weight": weight,
           "side_color": side_color, "pos_neg_normal": both["normal"][both["convergent_mask"]]}
    if VERBOSE_MODE:
        ctx["verbose"] = {"side_uv": side_uv, "side_depth": both["depth"].reshape(-1)}
    return ctx


def _edge_blend(results, ctx):
    """Second half: iron_edge_blend writes colour, normal, uv and point of the edge pixels into `results`."""
    dev = ctx["edge_uv"].device
    n_edge = ctx["n_edge"]
    for k in ("color", "normal", "uv", "points"):
        if not results[k].is_contiguous():
            results[k] = results[k].contiguous()
    n_pixels = results["color"].numel() // 3
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.iron_edge_blend(ctx["side_color"].data_ptr(), ctx["weight"].data_ptr(), ctx["edge_grads"].data_ptr(),
                                       ctx["edge_uv"].data_ptr(), ctx["edge_points"].data_ptr(), ctx["pixel"].data_ptr(), n_edge, n_pixels,
                                       results["color"].data_ptr(), results["normal"].data_ptr(), results["uv"].data_ptr(),
                                       results["points"].data_ptr(), _lib.stream_ptr(dev)))
    results["edge_pos_neg_normal"] = ctx["pos_neg_normal"]
    if VERBOSE_MODE and "verbose" in ctx:  # the reference's debug maps (raytracer.py:731-775)
        v, pixel = ctx["verbose"], ctx["pixel"]
        shape = list(results["edge_mask"].shape)
        maps = {}
        for key, vals, ch in (("edge_pos_side_weight", ctx["weight"], None), ("edge_pos_side_depth", v["side_depth"][:n_edge], None),
                              ("edge_neg_side_depth", v["side_depth"][n_edge:], None),
                              ("edge_pos_side_color", ctx["side_color"][:n_edge], 3), ("edge_neg_side_color", ctx["side_color"][n_edge:], 3)):
            img = torch.zeros(shape + ([ch] if ch else []), dtype=torch.float32, device=dev)
            if ch:
                img.view(-1, ch)[pixel] = vals
            else:
                img.view(-1)[pixel] = vals
            maps[key] = img
        maps["pos_side_uv"], maps["neg_side_uv"] = v["side_uv"][:n_edge], v["side_uv"][n_edge:]
        half = 0.5 * (maps["neg_side_uv"] - maps["pos_side_uv"])          # = PIXEL_RADIUS * edge_normals2d (raytracer.py:693-694)
        maps["edge_normals2d"] = half / (half.norm(dim=-1, keepdim=True) + 1e-10)
        results.update(maps)


def _render_edge_pixels_training(results, camera, sdf_network, raytracer, color_network_dict, render_fn):
    prep = _edge_training_prepare(results, camera, sdf_network)
    both = _side_rays(results, prep["n_edge"], sdf_network, raytracer, camera, prep["side_uv"], color_network_dict, render_fn, True)
    _edge_training_finish(results, prep, both)


def _edge_training_prepare(results, camera, sdf_network):
    """Edge points re-attached to the SDF parameters, their projection, and the (non-differentiable) side samples."""
    anchor = results["edge_points"]
    centre = results["edge_uv"].floor() + 0.5
    sdf_at_edge, _, grads = sdf_network.get_all(anchor, is_training=True)
    g = grads.detach()
    unit = g / (g.norm(dim=-1, keepdim=True) + 1e-10)
    # the edge point slides along its normal with the parameters, and so does its projection
    moving = reparam_points(anchor, g, unit, sdf_at_edge)
    moving_uv = camera.project(moving)
    in_plane = (unit.unsqueeze(1) * camera.W2C[:2, :3].unsqueeze(0)).sum(dim=-1)   # first two rows of the camera-space normal
    in_plane = in_plane / (in_plane.norm(dim=-1, keepdim=True) + 1e-10)
    offset = PIXEL_RADIUS * in_plane
    return {"n_edge": int(anchor.shape[0]), "centre": centre, "grads": grads, "moving": moving, "moving_uv": moving_uv,
            "in_plane": in_plane, "side_uv": torch.cat([centre - offset, centre + offset], dim=0)}


def _edge_training_finish(results, prep, both):
    pixel = results["edge_pixel_idx"]
    n_edge, centre, in_plane = prep["n_edge"], prep["centre"], prep["in_plane"]
    # circular-segment area on the positive side of a chord at signed distance h from the centre, as a fraction of the disc
    h = ((prep["moving_uv"] - centre) * in_plane).sum(dim=-1)
    angle = 2 * torch.arccos((h / PIXEL_RADIUS).clamp(min=0.0, max=1.0))
    w = (1.0 - (angle - torch.sin(angle)) / (2.0 * np.pi)).unsqueeze(-1)
    results["color"].view(-1, 3)[pixel] = both["color"][:n_edge] * w + both["color"][n_edge:] * (1.0 - w)
    results["normal"].view(-1, 3)[pixel] = prep["grads"]
    results["edge_pos_neg_normal"] = both["normal"][both["convergent_mask"]]
    results["uv"].view(-1, 2)[pixel] = prep["moving_uv"].detach()
    results["points"].view(-1, 3)[pixel] = prep["moving"].detach()


def render_camera(camera, sdf_network, raytracer, color_network_dict, render_fn, fill_holes=False, handle_edges=True,
                  is_training=False, depth_edge_mask=None):
    """raytracer.py:778-814 (`depth_edge_mask`: see raytrace_camera).
    Inference with handle_edges and the fused GGX render_fn runs the hit shading and the silhouette pass side by side on two streams
    (_render_camera_overlapped); IRON_EDGE_OVERLAP=0 keeps them in sequence."""
    if (handle_edges and not is_training and EDGE_OVERLAP and getattr(render_fn, "iron_fused_ggx", None) is not None
            and camera.K.is_cuda and not _has_stream_bound_scratch(color_network_dict)):
        return _render_camera_overlapped(camera, sdf_network, raytracer, color_network_dict, render_fn, fill_holes, depth_edge_mask)
    results = raytrace_camera(camera, sdf_network, raytracer, max_num_rays=50000, fill_holes=fill_holes,
                              detect_edges=handle_edges, depth_edge_mask=depth_edge_mask)
    render_normal_and_color(results, sdf_network, color_network_dict, render_fn, is_training=is_training,
                            max_num_pts=320000)
    if handle_edges and results["edge_mask"].sum() > 0:
        render_edge_pixels(results, camera, sdf_network, raytracer, color_network_dict, render_fn, is_training=is_training)
    return results


# ---- hit shading beside the side rays of the silhouette pass -----------------------------------------------------------------------
# The second half of an inference frame's silhouette pass (two side rays per edge pixel: generated, traced through <= 17 + 16 + ~10
# dependent SDF evaluations, shaded) is a latency chain on a few thousand rays -- ~6 ms per 800x800 frame during which some 30
# workgroups are busy and the rest of the chip idles.  It reads the edge_* maps only; the shading of the hits reads the traced maps
# only.  They run on two streams, each on its share of the CUs (iron_set_cu_limit: the persistent kernels fill one CU per workgroup,
# a full-width shading launch would leave the side stream nothing; measured with tools/cu_share.py).  The surface walk that finds the
# edge points stays in front of both, at full width: it is ~250 workgroup-tiles of work on the depth-edge candidates, and the hits
# are shaded with the edge pixels already out of the convergent mask, exactly the reference's order (raytracer.py:586-588, 800-812).
EDGE_OVERLAP = os.environ.get("IRON_EDGE_OVERLAP", "1") != "0"
# CUs of the side-ray stream (one workgroup traces 128 rays).  Round 3: the hits' shading got twice as fast (reverse-mode get_all), so the
# side chain -- its sampler is throughput-bound on few CUs -- is the longer branch now: 800x800 frame 63.6 / 62.9 / 61.9-62.8 / 62.5 / 63.2 ms
# with 48 / 64 / 80 / 96 / 128 side CUs on one box (the plain frame: 53.9)
EDGE_SIDE_CUS = int(os.environ.get("IRON_EDGE_SIDE_CUS", "96"))
_side_streams = {}


def _has_stream_bound_scratch(color_network_dict) -> bool:
    """A material net with a skip layer parks partial sums in a per-handle scratch indexed by workgroup (k_material_h2_skip):
    launches on such a handle must be ordered on ONE stream (include/iron_hip.h).  The overlapped frame shades the hits and the
    side rays with the same handles on two streams, so it is only taken when no net of the dict has a skip layer."""
    for net in color_network_dict.values():
        if len(getattr(net, "skip_in", ()) or ()) > 0 and not hasattr(net, "sdf"):
            return True
    return False


def _side_stream(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=dev)
    return _side_streams[key]


def _render_camera_overlapped(camera, sdf_network, raytracer, color_network_dict, render_fn, fill_holes, depth_edge_mask):
    results = raytrace_camera(camera, sdf_network, raytracer, max_num_rays=50000, fill_holes=fill_holes, detect_edges=True,
                              depth_edge_mask=depth_edge_mask)
    if int(results["edge_uv"].shape[0]) == 0:
        render_normal_and_color(results, sdf_network, color_network_dict, render_fn, is_training=False, max_num_pts=320000)
        return results
    dev = results["points"].device
    lib = _lib.load()
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    located = torch.cuda.Event()
    located.record(main)
    n_cu = int(lib.iron_set_cu_limit(0))
    side_cus = max(1, min(EDGE_SIDE_CUS, n_cu // 2))
    try:
        lib.iron_set_cu_limit(n_cu - side_cus)
        render_normal_and_color(results, sdf_network, color_network_dict, render_fn, is_training=False, max_num_pts=320000)
        lib.iron_set_cu_limit(side_cus)
        with torch.cuda.stream(side):
            side.wait_event(located)
            ctx = _edge_side_colours(results, camera, sdf_network, raytracer, color_network_dict, render_fn)
            done = torch.cuda.Event()
            done.record(side)
    finally:
        lib.iron_set_cu_limit(0)
    main.wait_event(done)
    for v in ctx.values():   # produced on the side stream, consumed (and possibly released) on the caller's
        if torch.is_tensor(v) and v.is_cuda:
            v.record_stream(main)
    _edge_blend(results, ctx)
    return results
