"""torch.autograd.Function wrappers that make the HIP operators trainable (BASELINE config C3).

The reference trains by running its ordinary torch modules under autograd (render_surface.py:533-653).  Here each
operator's forward is the inference HIP kernel (libiron_hip.so) and its backward is the closed-form HIP pass (hand-written split-fp16 MFMA GEMMs, no BLAS) of
libiron_train.so (include/iron_train.h):

    SDFGetAllFn      SDFNetwork.get_all(is_training=True) / .gradient       models/fields.py:106-137 (second order)
    RenderNetFn      RenderingNetwork.forward                               models/fields.py:203-239
    GGXColocatedFn   GGXColocatedRenderer.forward                           models/renderer_ggx.py:82-146
    PyramidL2Fn      PyramidL2Loss.forward                                  models/image_losses.py:29-48
    SSIMFn           ssim_loss_fn                                           models/image_losses.py:97-158

so `render_camera(..., is_training=True)`, the reference's `reparam_points`, its `render_fn` closure and its loss code
run unchanged on top and `loss.backward()` fills `.grad` of weight_g / weight_v / bias / light exactly as there.  There is
no fallback: a missing library or a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _layer_params(net) -> List[torch.Tensor]:
    """Flat parameter list in the order the Functions take / return them: per layer (weight_g, weight_v, bias) or
    (weight, bias)."""
    out = []
    for lin in net._layers():
        if getattr(lin, "has_weight_norm", False):
            out += [lin.weight_g, lin.weight_v, lin.bias]
        else:
            out += [lin.weight, lin.bias]
    return out


def _train_layers(net, device):
    """iron_train_layer array over the module's current parameters + freshly allocated gradient buffers (returned in
    _layer_params order)."""
    layers = net._layers()
    arr = (_lib.iron_train_layer * len(layers))()
    keep, grads = [], []
    for i, lin in enumerate(layers):
        wn = getattr(lin, "has_weight_norm", False)
        v = (lin.weight_v if wn else lin.weight).detach()
        b = lin.bias.detach()
        v = _lib.require_cuda_f32(v, "weight")
        b = _lib.require_cuda_f32(b, "bias")
        dv, db = torch.empty_like(v), torch.empty_like(b)
        arr[i].weight_v, arr[i].bias, arr[i].d_weight_v, arr[i].d_bias = v.data_ptr(), b.data_ptr(), dv.data_ptr(), db.data_ptr()
        arr[i].out_dim, arr[i].in_dim = v.shape[0], v.shape[1]
        keep += [v, b]
        if wn:
            g = _lib.require_cuda_f32(lin.weight_g.detach(), "weight_g")
            dg = torch.empty_like(g)
            arr[i].weight_g, arr[i].d_weight_g = g.data_ptr(), dg.data_ptr()
            keep.append(g)
            grads += [dg, dv, db]
        else:
            arr[i].weight_g, arr[i].d_weight_g = None, None
            grads += [dv, db]
    return arr, keep, grads


def _opt(t: Optional[torch.Tensor], shape=None) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = _lib.require_cuda_f32(t, "upstream gradient")
    return t.reshape(shape) if shape is not None else t


def _flat3(t: torch.Tensor, lead, name: str) -> torch.Tensor:
    """A [..., 3] input, or a [..., 1] one broadcast over the channels, as a contiguous [n, 3] CUDA float32 tensor."""
    return _lib.require_cuda_f32(t.expand(lead + [3]), name).reshape(-1, 3)


def _unflat3(g: torch.Tensor, lead, shape) -> torch.Tensor:
    """The [n, 3] gradient of a _flat3 input in that input's shape (summed over the channels of a broadcast [..., 1])."""
    g = g.reshape(lead + [3])
    return (g.sum(dim=-1, keepdim=True) if shape[-1] == 1 else g).reshape(shape)


class SDFGetAllFn(torch.autograd.Function):
    """(sdf [n,1], feature [n,d_out-1], gradient [n,3]) = get_all(x); differentiable w.r.t. the network parameters, to
    second order through `gradient` (the tangent sweep of iron_sdf_backward).  x itself gets no gradient: the reference
    evaluates get_all on the tracer's detached hit points (raytracer.py:622) and on sampled eikonal points."""

    @staticmethod
    def forward(ctx, net, x, *params):
        ctx.set_materialize_grads(False)
        ctx.net = net
        ctx.param_versions = tuple(p._version for p in params)  # backward re-reads the module's parameters: they must not have moved
        with torch.no_grad():
            sdf, feat, grad = net.get_all(x, is_training=False)
        ctx.save_for_backward(x.detach())
        return sdf, feat, grad

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, d_sdf, d_feat, d_grad):
        net = ctx.net
        (x,) = ctx.saved_tensors
        x = _lib.require_cuda_f32(x, "x").reshape(-1, 3)
        n = x.shape[0]
        dev = x.device
        if ctx.param_versions != tuple(p._version for p in _layer_params(net)):
            raise RuntimeError("a parameter of the SDFNetwork was modified in place between get_all(is_training=True) and backward(); "
                               "the closed-form backward re-evaluates the forward from the CURRENT parameters (as autograd's own version "
                               "check would, this refuses instead of returning a gradient of a different function)")
        if net.scale != 1 or len(net.skip_in) > 1:
            raise _lib.IronError("SDF backward supports scale = 1 and at most one skip layer")
        lib = _lib.load_train()
        with torch.cuda.device(dev):
            arr, keep, grads = _train_layers(net, dev)
            desc = _lib.iron_sdf_train_desc()
            desc.n_linear, desc.multires = net.num_layers - 1, net.multires
            desc.skip_layer = net.skip_in[0] if net.skip_in else -1
            desc.layers = arr
            d_sdf, d_feat, d_grad = _opt(d_sdf, (-1,)), _opt(d_feat, (n, -1)), _opt(d_grad, (-1, 3))
            nbytes = lib.iron_sdf_backward_workspace_bytes(C.byref(desc), n)
            if nbytes == 0:
                raise _lib.IronError("unsupported SDFNetwork shape for the backward pass")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check_train(lib.iron_sdf_backward(C.byref(desc), x.data_ptr(), n, _lib.ptr(d_sdf), _lib.ptr(d_feat), _lib.ptr(d_grad),
                                                   ws.data_ptr(), nbytes, _lib.stream_ptr(dev)))
        del keep
        return (None, None) + tuple(grads)


class RenderNetFn(torch.autograd.Function):
    """out = RenderingNetwork(points, normals, view_dirs, features); differentiable w.r.t. all four inputs and the
    parameters."""

    @staticmethod
    def forward(ctx, net, points, normals, view_dirs, feats, *params):
        ctx.net = net
        with torch.no_grad():
            out = net._forward_values(points, normals, view_dirs, feats)
        ctx.has = (normals is not None, view_dirs is not None)
        ctx.shapes = (points.shape, None if normals is None else normals.shape, None if view_dirs is None else view_dirs.shape, feats.shape)
        ctx.save_for_backward(points.detach(), feats.detach(), *([normals.detach()] if normals is not None else []),
                              *([view_dirs.detach()] if view_dirs is not None else []))
        return out

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, d_out):
        net = ctx.net
        saved = list(ctx.saved_tensors)
        pts, feats = saved[0], saved[1]
        k = 2
        nrm = vd = None
        if ctx.has[0]:
            nrm = saved[k]; k += 1
        if ctx.has[1]:
            vd = saved[k]
        pts = _lib.require_cuda_f32(pts, "points").reshape(-1, 3)
        n = pts.shape[0]
        dev = pts.device
        feats = _lib.require_cuda_f32(feats, "features").reshape(n, -1)
        nrm = _lib.require_cuda_f32(nrm, "normals").reshape(-1, 3) if nrm is not None else None
        vd = _lib.require_cuda_f32(vd, "view_dirs").reshape(-1, 3) if vd is not None else None
        lib = _lib.load_train()
        with torch.cuda.device(dev):
            arr, keep, grads = _train_layers(net, dev)
            desc = _lib.iron_render_train_desc()
            desc.n_linear, desc.mode = net.num_layers - 1, _lib.MODES[net.mode]
            desc.multires, desc.multires_view = net.multires, net.multires_view
            desc.d_feature, desc.d_out = net.d_feature, net.d_out
            if len(net.skip_in) > 1:
                raise _lib.IronError("RenderingNetwork backward supports at most one skip layer")
            desc.skip_layer = net.skip_in[0] if net.skip_in else -1
            desc.squeeze_out = 1 if net.squeeze_out else 0
            desc.output_bias, desc.output_scale, desc.squeeze_out_scale = float(net.output_bias), float(net.output_scale), float(net.squeeze_out_scale)
            desc.layers = arr
            g = _lib.require_cuda_f32(d_out, "d_out").reshape(n, net.d_out)
            need = ctx.needs_input_grad  # (net, points, normals, view_dirs, feats, *params)
            d_pts = torch.empty_like(pts) if need[1] else None
            d_nrm = torch.empty_like(nrm) if (nrm is not None and need[2]) else None
            d_vd = torch.empty_like(vd) if (vd is not None and need[3]) else None
            d_ft = torch.empty_like(feats) if need[4] else None
            nbytes = lib.iron_render_backward_workspace_bytes(C.byref(desc), n)
            if nbytes == 0:
                raise _lib.IronError("unsupported RenderingNetwork shape for the backward pass")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check_train(lib.iron_render_backward(C.byref(desc), pts.data_ptr(), _lib.ptr(nrm), _lib.ptr(vd), feats.data_ptr(), n, g.data_ptr(),
                                                      _lib.ptr(d_pts), _lib.ptr(d_nrm), _lib.ptr(d_vd), _lib.ptr(d_ft), ws.data_ptr(), nbytes,
                                                      _lib.stream_ptr(dev)))
        del keep
        sp, sn, sv, sf = ctx.shapes
        return (None,
                d_pts.reshape(sp) if d_pts is not None else None,
                d_nrm.reshape(sn) if d_nrm is not None else None,
                d_vd.reshape(sv) if d_vd is not None else None,
                d_ft.reshape(sf) if d_ft is not None else None) + tuple(grads)


class GGXColocatedFn(torch.autograd.Function):
    """(diffuse_rgb, specular_rgb, rgb) = GGXColocatedRenderer(light, distance, normal, viewdir, kd, ks, roughness)."""

    @staticmethod
    def forward(ctx, renderer, light, distance, normal, viewdir, kd, ks, rough):
        ctx.set_materialize_grads(False)
        ctx.renderer = renderer
        light_t = light if torch.is_tensor(light) else None
        ctx.light_shape = None if light_t is None else light_t.shape
        ctx.light_value = float(light)
        with torch.no_grad():
            out = renderer._forward_values(ctx.light_value, distance, normal, viewdir, kd, ks, rough)
        ctx.shapes = (distance.shape, normal.shape, viewdir.shape, kd.shape, ks.shape, rough.shape)
        ctx.save_for_backward(distance.detach(), normal.detach(), viewdir.detach(), kd.detach(), ks.detach(), rough.detach())
        return out["diffuse_rgb"], out["specular_rgb"], out["rgb"]

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, g_diff, g_spec, g_rgb):
        dist, nrm, vd, kd, ks, rough = ctx.saved_tensors
        nrm = _lib.require_cuda_f32(nrm, "normal").reshape(-1, 3)
        n = nrm.shape[0]
        dev = nrm.device
        sh = list(ctx.shapes[1][:-1])
        dist = _lib.require_cuda_f32(dist, "distance").reshape(-1)
        vd, kd, ks = _flat3(vd, sh, "viewdir"), _flat3(kd, sh, "diffuse_albedo"), _flat3(ks, sh, "specular_albedo")
        rough = _lib.require_cuda_f32(rough, "specular_roughness").reshape(-1)
        t1, t2 = ctx.renderer._tables_on(dev)
        g_diff, g_spec, g_rgb = _opt(g_diff, (-1, 3)), _opt(g_spec, (-1, 3)), _opt(g_rgb, (-1, 3))
        lib = _lib.load_train()
        with torch.cuda.device(dev):
            d_light = torch.zeros(1, dtype=torch.float32, device=dev)
            d_dist, d_rough = torch.empty_like(dist), torch.empty_like(rough)
            d_nrm, d_vd, d_kd, d_ks = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(4))
            _lib.check_train(lib.iron_ggx_colocated_backward(ctx.light_value, dist.data_ptr(), nrm.data_ptr(), vd.data_ptr(), kd.data_ptr(),
                                                             ks.data_ptr(), rough.data_ptr(), t1.data_ptr(), t2.data_ptr(), n, _lib.ptr(g_diff),
                                                             _lib.ptr(g_spec), _lib.ptr(g_rgb), d_light.data_ptr(), d_dist.data_ptr(),
                                                             d_nrm.data_ptr(), d_vd.data_ptr(), d_kd.data_ptr(), d_ks.data_ptr(),
                                                             d_rough.data_ptr(), _lib.stream_ptr(dev)))
        s_dist, s_nrm, s_vd, s_kd, s_ks, s_rough = ctx.shapes
        return (None, d_light.reshape(ctx.light_shape) if ctx.light_shape is not None else None, d_dist.reshape(s_dist), d_nrm.reshape(s_nrm),
                d_vd.reshape(s_vd), _unflat3(d_kd, sh, s_kd), _unflat3(d_ks, sh, s_ks), d_rough.reshape(s_rough))


class CompositeFn(torch.autograd.Function):
    """(rgb, specular_rgb, metallic_rgb, dielectric_rgb, env_light) = CompositeRenderer(light, distance, normal, viewdir, kd, ks,
    roughness, metallic_eta, metallic_k, dielectric_eta, env_light) (models/renderer_ggx.py:781-858).  env_light None = the
    point-light branch (the last output is then an empty placeholder).  "diffuse_rgb" is the same tensor as "rgb" in the
    reference, so the caller maps both keys to the first output."""

    NAMES = ("diffuse_albedo", "specular_albedo", "specular_roughness", "metallic_eta", "metallic_k", "dielectric_eta")

    @staticmethod
    def forward(ctx, renderer, light, distance, normal, viewdir, kd, ks, rough, m_eta, m_k, d_eta, env_light):
        ctx.set_materialize_grads(False)
        ctx.renderer = renderer
        ctx.light_shape = light.shape if torch.is_tensor(light) else None
        ctx.light_value = float(light)
        ctx.use_env = env_light is not None
        params = dict(zip(CompositeFn.NAMES, (kd, ks, rough, m_eta, m_k, d_eta)))
        params["metallic"] = params["dielectric"] = rough  # read and ignored by the reference (:829-831)
        if ctx.use_env:
            params["env_light"] = env_light
        with torch.no_grad():
            out = renderer._forward_values(ctx.light_value, distance, normal, viewdir, params, ctx.use_env)
        tensors = [normal, viewdir, kd, ks, rough, m_eta, m_k, d_eta, env_light if ctx.use_env else distance]
        ctx.shapes = tuple(t.shape for t in tensors)
        ctx.dist_shape = distance.shape if torch.is_tensor(distance) else None
        ctx.save_for_backward(*(t.detach() for t in tensors))
        env_out = out["env_light"] if ctx.use_env else normal.new_zeros(0)
        return out["rgb"], out["specular_rgb"], out["metallic_rgb"], out["dielectric_rgb"], env_out

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, g_rgb, g_spec, g_met, g_die, g_env):
        nrm, vd, kd, ks, rough, m_eta, m_k, d_eta, last = ctx.saved_tensors
        nrm = _lib.require_cuda_f32(nrm, "normal").reshape(-1, 3)
        n = nrm.shape[0]
        dev = nrm.device
        sh = list(ctx.shapes[0][:-1])

        def sca(t, name):
            return _lib.require_cuda_f32(t, name).reshape(-1)

        vd = _flat3(vd, sh, "viewdir")
        kd_f, ks_f = _flat3(kd, sh, "diffuse_albedo"), _flat3(ks, sh, "specular_albedo")
        maps = [sca(t, k) for t, k in zip((rough, m_eta, m_k, d_eta), CompositeFn.NAMES[2:])]
        last = sca(last, "env_light" if ctx.use_env else "distance")
        t1, t2 = ctx.renderer._tables_on(dev)
        ups = [_opt(g, (-1, 3)) for g in (g_rgb, g_spec, g_met, g_die)]
        g_env = _opt(g_env, (-1,)) if ctx.use_env else None
        lib = _lib.load_train()
        with torch.cuda.device(dev):
            p = _lib.iron_composite_params()
            p.diffuse_albedo, p.specular_albedo, p.specular_roughness = kd_f.data_ptr(), ks_f.data_ptr(), maps[0].data_ptr()
            p.metallic_eta, p.metallic_k, p.dielectric_eta = maps[1].data_ptr(), maps[2].data_ptr(), maps[3].data_ptr()
            p.env_light = last.data_ptr() if ctx.use_env else None
            gi = _lib.iron_composite_grads_in()
            gi.d_rgb, gi.d_specular_rgb, gi.d_metallic_rgb, gi.d_dielectric_rgb = (_lib.ptr(u) for u in ups)
            gi.d_env_light_out = _lib.ptr(g_env)
            d_light = torch.zeros(1, dtype=torch.float32, device=dev)
            d_last = torch.empty_like(last)
            d_nrm, d_vd, d_kd, d_ks = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(4))
            d_maps = [torch.empty_like(m) for m in maps]
            go = _lib.iron_composite_grads_out()
            go.d_light, go.d_normal, go.d_viewdir = d_light.data_ptr(), d_nrm.data_ptr(), d_vd.data_ptr()
            go.d_distance = None if ctx.use_env else d_last.data_ptr()
            go.d_env_light = d_last.data_ptr() if ctx.use_env else None
            go.d_diffuse_albedo, go.d_specular_albedo = d_kd.data_ptr(), d_ks.data_ptr()
            go.d_specular_roughness, go.d_metallic_eta, go.d_metallic_k, go.d_dielectric_eta = (m.data_ptr() for m in d_maps)
            _lib.check_train(lib.iron_composite_colocated_backward(ctx.light_value, None if ctx.use_env else last.data_ptr(), nrm.data_ptr(),
                                                                   vd.data_ptr(), C.byref(p), t1.data_ptr(), t2.data_ptr(), n, C.byref(gi), C.byref(go),
                                                                   _lib.stream_ptr(dev)))
        s_nrm, s_vd, s_kd, s_ks = ctx.shapes[:4]
        d_light_out = d_light.reshape(ctx.light_shape) if (ctx.light_shape is not None and not ctx.use_env) else None
        d_dist = None
        if not ctx.use_env:
            d_dist = d_last.reshape(ctx.shapes[8])
        elif ctx.dist_shape is not None:
            d_dist = torch.zeros(ctx.dist_shape, dtype=torch.float32, device=dev)
        d_env = d_last.reshape(ctx.shapes[8]) if ctx.use_env else None
        return (None, d_light_out, d_dist, d_nrm.reshape(s_nrm), d_vd.reshape(s_vd), _unflat3(d_kd, sh, s_kd), _unflat3(d_ks, sh, s_ks)) + tuple(
            m.reshape(s) for m, s in zip(d_maps, ctx.shapes[4:8])) + (d_env,)


class ColocHeadFn(torch.autograd.Function):
    """(diffuse_rgb, specular_rgb, rgb) of the four simple co-located heads (models/renderer_ggx.py:149-395)."""

    @staticmethod
    def forward(ctx, head, light, distance, normal, viewdir, kd, ks, alpha):
        ctx.set_materialize_grads(False)
        ctx.head = head
        ctx.light_shape = light.shape if torch.is_tensor(light) else None
        ctx.light_value = float(light)
        with torch.no_grad():
            out = head._forward_values(ctx.light_value, distance, normal, viewdir, kd, ks, alpha)
        ctx.has_alpha = alpha is not None
        ctx.shapes = (distance.shape, normal.shape, viewdir.shape, kd.shape, ks.shape, None if alpha is None else alpha.shape)
        ctx.save_for_backward(distance.detach(), normal.detach(), viewdir.detach(), kd.detach(), ks.detach(),
                              *([alpha.detach()] if alpha is not None else []))
        return out["diffuse_rgb"], out["specular_rgb"], out["rgb"]

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, g_diff, g_spec, g_rgb):
        saved = list(ctx.saved_tensors)
        dist, nrm, vd, kd, ks = saved[:5]
        alpha = saved[5] if ctx.has_alpha else None
        head = ctx.head
        nrm = _lib.require_cuda_f32(nrm, "normal").reshape(-1, 3)
        n = nrm.shape[0]
        dev = nrm.device
        sh = list(ctx.shapes[1][:-1])
        dist = _lib.require_cuda_f32(dist, "distance").reshape(-1)
        vd, kd_f, ks_f = _flat3(vd, sh, "viewdir"), _flat3(kd, sh, "diffuse_albedo"), _flat3(ks, sh, "specular_albedo")
        al = _lib.require_cuda_f32(alpha, "alpha").reshape(-1) if (alpha is not None and head.KIND == 3) else None
        ups = [_opt(g, (-1, 3)) for g in (g_diff, g_spec, g_rgb)]
        with torch.cuda.device(dev):
            d_light = torch.zeros(1, dtype=torch.float32, device=dev)
            d_dist = torch.empty_like(dist)
            d_nrm, d_vd, d_kd, d_ks = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(4))
            d_al = torch.empty_like(al) if al is not None else None
            _lib.check_train(_lib.load_train().iron_coloc_head_backward(
                head.KIND, ctx.light_value, float(head.eta), float(head.k), dist.data_ptr(), nrm.data_ptr(), vd.data_ptr(), kd_f.data_ptr(),
                ks_f.data_ptr(), _lib.ptr(al), n, _lib.ptr(ups[0]), _lib.ptr(ups[1]), _lib.ptr(ups[2]), d_light.data_ptr(), d_dist.data_ptr(),
                d_nrm.data_ptr(), d_vd.data_ptr(), d_kd.data_ptr(), d_ks.data_ptr(), _lib.ptr(d_al), _lib.stream_ptr(dev)))
        s_dist, s_nrm, s_vd, s_kd, s_ks, s_al = ctx.shapes
        d_alpha = None
        if ctx.has_alpha:
            d_alpha = d_al.reshape(s_al) if d_al is not None else torch.zeros(s_al, dtype=torch.float32, device=dev)
        return (None, d_light.reshape(ctx.light_shape) if ctx.light_shape is not None else None, d_dist.reshape(s_dist), d_nrm.reshape(s_nrm),
                d_vd.reshape(s_vd), _unflat3(d_kd, sh, s_kd), _unflat3(d_ks, sh, s_ks), d_alpha)


class NeRFFn(torch.autograd.Function):
    """(alpha [n,1], rgb [n,3]) = NeRF(input_pts [n,4], input_views [n,3]); differentiable w.r.t. the parameters (the reference
    feeds sample positions computed without grad, renderer.py:163-172, so the inputs get none)."""

    @staticmethod
    def forward(ctx, net, pts, views, *params):
        ctx.set_materialize_grads(False)
        ctx.net = net
        with torch.no_grad():
            alpha, rgb = net._forward_values(pts, views)
        ctx.save_for_backward(pts.detach(), views.detach())
        return alpha, rgb

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, d_alpha, d_rgb):
        net = ctx.net
        pts, views = ctx.saved_tensors
        pts = _lib.require_cuda_f32(pts, "input_pts").reshape(-1, net.d_in)
        views = _lib.require_cuda_f32(views, "input_views").reshape(-1, net.d_in_view)
        n = pts.shape[0]
        dev = pts.device
        lib = _lib.load_train()
        with torch.cuda.device(dev):
            arr, keep, grads = _train_layers(net, dev)
            desc = _lib.iron_nerf_train_desc()
            desc.D, desc.W, desc.d_in, desc.d_in_view = net.D, net.W, net.d_in, net.d_in_view
            desc.multires, desc.multires_view = net.multires, net.multires_view
            if len(net.skips) > 1:
                raise _lib.IronError("NeRF backward supports at most one skip layer")
            desc.skip = net.skips[0] if net.skips else -1
            desc.layers = arr
            nbytes = lib.iron_nerf_backward_workspace_bytes(C.byref(desc), n)
            if nbytes == 0:
                raise _lib.IronError("unsupported NeRF shape for the backward pass")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            d_alpha, d_rgb = _opt(d_alpha, (-1,)), _opt(d_rgb, (-1, 3))
            _lib.check_train(lib.iron_nerf_backward(C.byref(desc), pts.data_ptr(), views.data_ptr(), n, _lib.ptr(d_alpha), _lib.ptr(d_rgb),
                                                    ws.data_ptr(), nbytes, _lib.stream_ptr(dev)))
        del keep
        return (None, None, None) + tuple(grads)


class NeusCompositeFn(torch.autograd.Function):
    """The compositing of NeuSRenderer.render_core (models/renderer.py:279-344, background blend :174-178) from the network
    outputs at the section mid points: (sdf [n*m,1], grad [n*m,3], colour [n*m,3], 1/s, background density / colour) ->
    (color [n,3], weights, weight_sum, gradient_error, cdf, inside_sphere, weight_max).  The last three carry no gradient."""

    @staticmethod
    def forward(ctx, sdf, grad, color, inv_s, bg_density, bg_color, dists, pts, dirs, bg_dists, background_rgb, cos_anneal_ratio):
        ctx.set_materialize_grads(False)
        n, m = dists.shape
        dev = dists.device
        f32 = lambda t, name: _lib.require_cuda_f32(t.detach(), name)
        sdf_c, grad_c, color_c = f32(sdf, "sdf").reshape(-1), f32(grad, "gradients").reshape(-1, 3), f32(color, "sampled_color").reshape(-1, 3)
        dists_c, pts_c, dirs_c = f32(dists, "dists"), f32(pts, "pts").reshape(-1, 3), f32(dirs, "dirs").reshape(-1, 3)
        bg = bg_density is not None
        mo = bg_dists.shape[1] if bg else m
        keep = [sdf_c, grad_c, color_c, dists_c, pts_c, dirs_c]
        a = _lib.iron_neus_composite_args()
        a.dists, a.pts, a.dirs, a.sdf, a.grad, a.color = (t.data_ptr() for t in (dists_c, pts_c, dirs_c, sdf_c, grad_c, color_c))
        if bg:
            bgd, bgc, bgdist = f32(bg_density, "density").reshape(-1), f32(bg_color, "background colour").reshape(-1, 3), f32(bg_dists, "bg_dists")
            keep += [bgd, bgc, bgdist]
            a.bg_dists, a.bg_density, a.bg_color = bgdist.data_ptr(), bgd.data_ptr(), bgc.data_ptr()
        bgrgb = f32(background_rgb, "background_rgb").reshape(3) if background_rgb is not None else None
        a.background_rgb = _lib.ptr(bgrgb)
        a.n, a.m, a.mo = n, m, mo
        inv_s_value = float(inv_s)
        a.inv_s, a.cos_anneal_ratio = inv_s_value, float(cos_anneal_ratio)
        out_color = torch.empty((n, 3), dtype=torch.float32, device=dev)
        weights = torch.empty((n, mo), dtype=torch.float32, device=dev)
        cdf = torch.empty((n, m), dtype=torch.float32, device=dev)
        inside = torch.empty((n, m), dtype=torch.float32, device=dev)
        wsum = torch.empty((n, 1), dtype=torch.float32, device=dev)
        wmax = torch.empty((n, 1), dtype=torch.float32, device=dev)
        gacc = torch.zeros(2, dtype=torch.float32, device=dev)
        a.out_color, a.weights, a.cdf, a.inside_sphere = out_color.data_ptr(), weights.data_ptr(), cdf.data_ptr(), inside.data_ptr()
        a.weight_sum, a.weight_max, a.gradient_error_acc = wsum.data_ptr(), wmax.data_ptr(), gacc.data_ptr()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().iron_neus_composite(C.byref(a), _lib.stream_ptr(dev)))
        gerr = gacc[0] / (gacc[1] + 1e-5)
        ctx.meta = (n, m, mo, bg, inv_s_value, float(cos_anneal_ratio), torch.is_tensor(inv_s), tuple(sdf.shape), tuple(grad.shape), tuple(color.shape),
                    None if not bg else tuple(bg_density.shape), None if not bg else tuple(bg_color.shape))
        ctx.save_for_backward(gacc, *(keep + ([bgrgb] if bgrgb is not None else [])))
        ctx.has_bgrgb = bgrgb is not None
        ctx.mark_non_differentiable(cdf, inside, wmax)
        return out_color, weights, wsum, gerr, cdf, inside, wmax

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, d_color, d_weights, d_wsum, d_gerr, _dc, _di, _dm):
        n, m, mo, bg, inv_s_value, ca, inv_s_is_tensor, s_sdf, s_grad, s_color, s_bgd, s_bgc = ctx.meta
        saved = list(ctx.saved_tensors)
        gacc, sdf_c, grad_c, color_c, dists_c, pts_c, dirs_c = saved[:7]
        k = 7
        bgd = bgc = bgdist = None
        if bg:
            bgd, bgc, bgdist = saved[k:k + 3]
            k += 3
        bgrgb = saved[k] if ctx.has_bgrgb else None
        dev = dists_c.device
        a = _lib.iron_neus_composite_args()
        a.dists, a.pts, a.dirs, a.sdf, a.grad, a.color = (t.data_ptr() for t in (dists_c, pts_c, dirs_c, sdf_c, grad_c, color_c))
        if bg:
            a.bg_dists, a.bg_density, a.bg_color = bgdist.data_ptr(), bgd.data_ptr(), bgc.data_ptr()
        a.background_rgb = _lib.ptr(bgrgb)
        a.n, a.m, a.mo, a.inv_s, a.cos_anneal_ratio = n, m, mo, inv_s_value, ca
        g = _lib.iron_neus_composite_grads()
        ups = [_opt(d_color, (n, 3)), _opt(d_wsum, (n,)), _opt(d_weights, (n, mo)), _opt(d_gerr, (1,))]
        g.d_color, g.d_weight_sum, g.d_weights, g.d_gradient_error = (_lib.ptr(u) for u in ups)
        relax = gacc[1:2].contiguous()
        g.relax_count = relax.data_ptr()
        d_sdf, d_grad, d_col = torch.empty_like(sdf_c), torch.empty_like(grad_c), torch.empty_like(color_c)
        d_inv = torch.zeros(1, dtype=torch.float32, device=dev)
        d_bgd = torch.empty_like(bgd) if bg else None
        d_bgc = torch.empty_like(bgc) if bg else None
        g.d_sdf, g.d_grad, g.d_sample_color, g.d_inv_s = d_sdf.data_ptr(), d_grad.data_ptr(), d_col.data_ptr(), d_inv.data_ptr()
        g.d_bg_density, g.d_bg_color = _lib.ptr(d_bgd), _lib.ptr(d_bgc)
        with torch.cuda.device(dev):
            _lib.check_train(_lib.load_train().iron_neus_composite_backward(C.byref(a), C.byref(g), _lib.stream_ptr(dev)))
        return (d_sdf.reshape(s_sdf), d_grad.reshape(s_grad), d_col.reshape(s_color), d_inv.reshape(()) if inv_s_is_tensor else None,
                d_bgd.reshape(s_bgd) if bg else None, d_bgc.reshape(s_bgc) if bg else None, None, None, None, None, None, None)


class PyramidL2Fn(torch.autograd.Function):
    """loss = PyramidL2Loss()(x, y) (models/image_losses.py:29-48); x, y [B, 3, H, W], H, W >= 16.  `taps` is the HOST ctypes
    float[49] of the 7x7 filter.  The loss is a device scalar; the backward reads its upstream gradient on the device."""

    @staticmethod
    def forward(ctx, x, y, taps):
        xc, yc = _lib.require_cuda_f32(x, "pred_img"), _lib.require_cuda_f32(y, "trgt_img")
        b, c, h, w = xc.shape
        lib = _lib.load_train()
        dev = xc.device
        with torch.cuda.device(dev):
            ws = torch.empty(max(int(lib.iron_pyramid_l2_workspace_bytes(b * c, h, w)), 16), dtype=torch.uint8, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check_train(lib.iron_pyramid_l2_forward(xc.data_ptr(), yc.data_ptr(), b * c, h, w, taps, loss.data_ptr(), ws.data_ptr(),
                                                         ws.numel(), _lib.stream_ptr(dev)))
        ctx.taps, ctx.ws = taps, ws  # the workspace carries d_1..d_4 to the backward
        ctx.save_for_backward(xc, yc)
        return loss

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, g):
        xc, yc = ctx.saved_tensors
        b, c, h, w = xc.shape
        g = _lib.require_cuda_f32(g, "upstream gradient").reshape(1)
        lib = _lib.load_train()
        dev = xc.device
        with torch.cuda.device(dev):
            dx = torch.empty_like(xc)
            dy = torch.empty_like(yc) if ctx.needs_input_grad[1] else None
            _lib.check_train(lib.iron_pyramid_l2_backward(xc.data_ptr(), yc.data_ptr(), b * c, h, w, ctx.taps, g.data_ptr(), ctx.ws.data_ptr(),
                                                          ctx.ws.numel(), dx.data_ptr(), _lib.ptr(dy), _lib.stream_ptr(dev)))
        return dx, dy, None


class SSIMFn(torch.autograd.Function):
    """loss = ssim_loss_fn(x, y, mask, ...) (models/image_losses.py:97-158) for [B, C, H, W] x, y.  `win` is the HOST ctypes
    float[win_size] window, `mask` None or a contiguous [B, 1, H, W] bool / uint8 / float32 CUDA tensor."""

    @staticmethod
    def forward(ctx, x, y, mask, win, win_size, c1, c2):
        xc, yc = _lib.require_cuda_f32(x, "X"), _lib.require_cuda_f32(y, "Y")
        b, c, h, w = xc.shape
        lib = _lib.load_train()
        dev = xc.device
        kind = 0
        if mask is not None:
            if mask.dtype == torch.bool:
                mask = mask.view(torch.uint8)
            kind = 1 if mask.dtype == torch.uint8 else 2
        state_b, scratch_b = C.c_size_t(0), C.c_size_t(0)
        _lib.check_train(lib.iron_ssim_workspace_bytes(b, c, h, w, win_size, kind != 0, C.byref(state_b), C.byref(scratch_b)))
        with torch.cuda.device(dev):
            state = torch.empty(max(state_b.value, 16), dtype=torch.uint8, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check_train(lib.iron_ssim_forward(xc.data_ptr(), yc.data_ptr(), b, c, h, w, win, win_size, c1, c2, _lib.ptr(mask), kind,
                                                   loss.data_ptr(), state.data_ptr(), state.numel(), _lib.stream_ptr(dev)))
        ctx.args = (win, win_size, c1, c2, kind != 0, scratch_b.value)
        ctx.state = state  # the eroded mask and |E|
        ctx.save_for_backward(xc, yc)
        return loss

    @staticmethod
    @once_differentiable  # closed-form first-order backward: differentiating it again raises instead of returning zeros
    def backward(ctx, g):
        xc, yc = ctx.saved_tensors
        b, c, h, w = xc.shape
        win, win_size, c1, c2, masked, scratch_bytes = ctx.args
        g = _lib.require_cuda_f32(g, "upstream gradient").reshape(1)
        lib = _lib.load_train()
        dev = xc.device
        with torch.cuda.device(dev):
            scratch = _lib.workspace(scratch_bytes, dev, "ssim_backward")
            dx = torch.empty_like(xc)
            dy = torch.empty_like(yc) if ctx.needs_input_grad[1] else None
            _lib.check_train(lib.iron_ssim_backward(xc.data_ptr(), yc.data_ptr(), b, c, h, w, win, win_size, c1, c2, 1 if masked else 0,
                                                    g.data_ptr(), ctx.state.data_ptr(), ctx.state.numel(), scratch.data_ptr(), scratch.numel(),
                                                    dx.data_ptr(), _lib.ptr(dy), _lib.stream_ptr(dev)))
        return dx, dy, None, None, None, None, None


class SurfaceRegFn(torch.autograd.Function):
    """(eik_loss, roughrange_loss, counts) = the regularisers of render_surface.py:580-613, 639 (include/iron_train.h:
    iron_surface_reg).  eik_grad [M, 3], normal [P, 3], mask [P] uint8, roughness [P], edge_normal [E, 3] or None; counts is the
    device int64 [3] (cnt, n_mask, n_selected).  Gradients go to eik_grad, normal, roughness and edge_normal."""

    @staticmethod
    def forward(ctx, eik_grad, normal, mask, roughness, edge_normal, eik_weight, roughrange_weight):
        lib = _lib.load_train()
        dev = eik_grad.device
        a = _lib.iron_surface_reg_args()
        a.eik_grad, a.normal, a.mask, a.roughness, a.edge_normal = (eik_grad.data_ptr(), normal.data_ptr(), mask.data_ptr(),
                                                                    roughness.data_ptr(), _lib.ptr(edge_normal))
        a.m, a.n_pix, a.e = eik_grad.shape[0], normal.shape[0], 0 if edge_normal is None else edge_normal.shape[0]
        a.eik_weight, a.roughrange_weight = eik_weight, roughrange_weight
        with torch.cuda.device(dev):
            ws = _lib.workspace(lib.iron_surface_reg_workspace_bytes(a.m, a.n_pix, a.e), dev, "surface_reg")
            eik = torch.empty((), dtype=torch.float32, device=dev)
            rr = torch.empty((), dtype=torch.float32, device=dev)
            counts = torch.empty(3, dtype=torch.int64, device=dev)
            state = torch.empty(4, dtype=torch.float64, device=dev)
            _lib.check_train(lib.iron_surface_reg(C.byref(a), eik.data_ptr(), rr.data_ptr(), counts.data_ptr(),
                                                  state.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        ctx.args, ctx.state = a, state
        ctx.save_for_backward(eik_grad, normal, mask, roughness, edge_normal)   # keeps the buffers `a` points to alive
        ctx.mark_non_differentiable(counts)
        return eik, rr, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g_eik, g_rr, _g_counts):
        eik_grad, normal, mask, roughness, edge_normal = ctx.saved_tensors
        lib = _lib.load_train()
        dev = eik_grad.device
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            g_eik = None if g_eik is None else _lib.require_cuda_f32(g_eik, "upstream gradient").reshape(1)
            g_rr = None if g_rr is None else _lib.require_cuda_f32(g_rr, "upstream gradient").reshape(1)
            d_eik = torch.empty_like(eik_grad) if need[0] else None
            d_normal = torch.empty_like(normal) if need[1] else None
            d_rough = torch.empty_like(roughness) if need[3] else None
            d_edge = torch.empty_like(edge_normal) if edge_normal is not None and need[4] else None
            _lib.check_train(lib.iron_surface_reg_backward(C.byref(ctx.args), ctx.state.data_ptr(), _lib.ptr(g_eik), _lib.ptr(g_rr),
                                                           _lib.ptr(d_eik), _lib.ptr(d_normal), _lib.ptr(d_rough), _lib.ptr(d_edge),
                                                           _lib.stream_ptr(dev)))
        return d_eik, d_normal, None, d_rough, d_edge, None, None


class VolumeLossFn(torch.autograd.Function):
    """(loss, record) = the stage-1 loss of render_volume.py:458-496 (include/iron_train.h: iron_volume_loss).  color_fine [B, 3],
    true_rgb [B, >= 3 with a row stride], raw mask [B, >= 1 with a row stride] or None, weight_sum [B], weight_max [B], cdf_fine
    [B, M], gradient_error: 0-d device tensor; record is the device fp32 [8] of _lib.VOLUME_LOSS_RECORD.  Gradients go to
    color_fine, weight_sum and gradient_error."""

    @staticmethod
    def forward(ctx, color_fine, true_rgb, mask, weight_sum, weight_max, cdf_fine, gradient_error, igr_weight, mask_weight):
        lib = _lib.load_train()
        dev = color_fine.device
        a = _lib.iron_volume_loss_args()
        a.color_fine, a.true_rgb, a.mask, a.weight_sum = color_fine.data_ptr(), true_rgb.data_ptr(), _lib.ptr(mask), weight_sum.data_ptr()
        a.weight_max, a.cdf_fine, a.gradient_error = weight_max.data_ptr(), cdf_fine.data_ptr(), gradient_error.data_ptr()
        a.b, a.rgb_stride, a.cdf_stride = color_fine.shape[0], true_rgb.stride(0), cdf_fine.stride(0)
        a.mask_stride = 1 if mask is None else mask.stride(0)
        a.igr_weight, a.mask_weight = igr_weight, mask_weight
        with torch.cuda.device(dev):
            ws = _lib.workspace(lib.iron_volume_loss_workspace_bytes(a.b), dev, "volume_loss")
            loss = torch.empty((), dtype=torch.float32, device=dev)
            record = torch.empty(len(_lib.VOLUME_LOSS_RECORD), dtype=torch.float32, device=dev)
            state = torch.empty(4, dtype=torch.float64, device=dev)
            _lib.check_train(lib.iron_volume_loss(C.byref(a), loss.data_ptr(), record.data_ptr(), state.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), _lib.stream_ptr(dev)))
        ctx.args, ctx.state = a, state
        ctx.save_for_backward(color_fine, true_rgb, mask, weight_sum, weight_max, cdf_fine, gradient_error)   # keeps `a`'s buffers alive
        ctx.mark_non_differentiable(record)
        return loss, record

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_record):
        color_fine, _, _, weight_sum, _, _, gradient_error = ctx.saved_tensors
        lib = _lib.load_train()
        dev = color_fine.device
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            g_loss = _lib.require_cuda_f32(g_loss, "upstream gradient").reshape(1)
            d_color = torch.empty_like(color_fine) if need[0] else None
            d_wsum = torch.empty_like(weight_sum) if need[3] else None
            d_gerr = torch.empty_like(gradient_error) if need[6] else None
            _lib.check_train(lib.iron_volume_loss_backward(C.byref(ctx.args), ctx.state.data_ptr(), g_loss.data_ptr(), _lib.ptr(d_color),
                                                           _lib.ptr(d_wsum), _lib.ptr(d_gerr), _lib.stream_ptr(dev)))
        return d_color, None, None, d_wsum, None, None, d_gerr, None, None


def numeric_status(reset: bool = True, device=None) -> bool:
    """True when a backward pass since the last reset met an operand outside the range of its split-fp16 layer products
    (|x| > 65 504 or non-finite: the gradients of that pass are inf / NaN where fp32 autograd has numbers; include/iron_train.h).
    Synchronises the current stream of `device`."""
    lib = _lib.load_train()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    rc = lib.iron_train_numeric_status(1 if reset else 0, _lib.stream_ptr(dev))
    if rc not in (0, -6):
        raise _lib.IronError("iron_train_numeric_status failed (%d)" % rc)
    return rc == -6


def any_requires_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def refuse_grad(what: str, *tensors) -> None:
    """Operators without a backward must not hand detached results to a training graph."""
    flat = []
    for t in tensors:
        flat += list(t.values()) if isinstance(t, dict) else [t]
    if any_requires_grad(*flat):
        raise NotImplementedError("%s has no backward pass in iron_amd (SURVEY 8 row f-2 covers SDFNetwork, RenderingNetwork and "
                                  "GGXColocatedRenderer); call it under torch.no_grad() or on detached inputs" % what)
