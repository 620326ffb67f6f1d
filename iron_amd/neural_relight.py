"""Environment-map relighting of the neural scene (csrc/envlight.hip, the k_nenv_* kernels): the direct integrator
of the exported asset's environment render (mesh_render.render_asset_env) on the trained SDF and material networks
themselves, with sphere-traced shadow rays (RayTracer.occluded) in place of the BVH walk.

A G-buffer -- render_camera's dictionary: convergent_mask, points, normal, ray_d, diffuse_albedo, specular_albedo,
specular_roughness -- is relit in blocks of pixels: the integrator emits the shadow rays of a block's counting samples, the tracer
answers them, the integrator adds the visible samples' terms.  The samples, their random numbers, the balance heuristic and the
order of every sum are those of iron_asset_shade_env; the shading normal stands where that kernel has a geometric normal.  Direct
illumination only.  There is no CPU path: CPU tensors are refused.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _args, _lib
from .mesh_render import _mts_tables, subpixel_uvs
from .raytracer import SDFCallable, SDFHandle, intersect_sphere, raytrace_pixels, render_normal_and_color

WHAT = "neural relight"
GBUFFER = ("convergent_mask", "points", "normal", "ray_d", "diffuse_albedo", "specular_albedo", "specular_roughness")
DUMPS = ("dump_dir", "dump_denom", "dump_vis", "dump_contrib")
STAGES = ("emit", "trace", "resolve")


def _as_sdf(sdf):
    """What RayTracer.occluded takes: an SDFNetwork is wrapped in its handle; SDFHandle and SDFCallable pass."""
    if isinstance(sdf, (SDFHandle, SDFCallable)):
        return sdf
    if hasattr(sdf, "hip_net"):
        return SDFHandle(sdf)
    raise _lib.IronError("%s: sdf must be an iron_amd SDFNetwork, an SDFHandle or an SDFCallable, got %s" % (WHAT, type(sdf).__name__))


class _Timer:
    """Event pairs around the three stages of every block, summed into stats["ms"] (one wait, at the end)."""

    def __init__(self, stats):
        self.pairs = [] if stats is not None else None

    def __call__(self, stage):
        return _Stage(self, stage)

    def finish(self, stats):
        if self.pairs is None:
            return
        torch.cuda.synchronize()
        ms = stats.setdefault("ms", {})
        for stage, a, b in self.pairs:
            ms[stage] = ms.get(stage, 0.0) + a.elapsed_time(b)


class _Stage:
    def __init__(self, timer, stage):
        self.timer, self.stage = timer, stage

    def __enter__(self):
        if self.timer.pairs is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.timer.pairs is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.timer.pairs.append((self.stage, self.a, b))


@torch.no_grad()
def relight_results(results, sdf, raytracer, envmap, n_light=64, n_brdf=64, seed=0, shadow_eps=1e-3, pixel_idx=None,
                    max_shadow_rays=1 << 22, dump=False, stats=None):
    """Relight the G-buffer `results` (the GBUFFER keys, [..., 3] / [...]; the tensors may come from anywhere, on one GPU) under
    `envmap` (EnvMap): per hit pixel the sum over n_light environment samples and n_brdf BRDF samples of
    L(w) roughplastic_point(n, -ray_d, w) V(w) / (n_light p_light(w) + n_brdf p_brdf(w)), the multi-sample balance heuristic of
    iron_asset_shade_env with the same random numbers (seed, pixel_idx [P] int32 or the pixel's position, sample, dimension).  A
    sample counts when n.w > 0, n.v > 0 and w is finite; V(w) = 1 when it counts and the shadow ray from x + shadow_eps n along w,
    cut to the unit sphere by intersect_sphere, is not raytracer.occluded(sdf, ...); a ray that misses the sphere is visible.
    shadow_eps (default 1e-3 = 20 x the tracer's sdf_threshold) is a parameter, not a measurement.

    `sdf`: an SDFNetwork, an SDFHandle or an SDFCallable.  Pixels are worked in blocks of max_shadow_rays // (n_light + n_brdf),
    which bounds the memory (about 170 bytes per shadow ray) and changes no bit of the result.  Every block waits once for the host
    to read the number of its shadow rays, the size of the tracer's call.
    -> {"color", "diffuse_color", "specular_color"} [..., 3], color = diffuse_color + specular_color, zeros on a miss; dump=True adds
    "dump_dir" [..., N, 3], "dump_denom" [..., N], "dump_vis" [..., N] uint8 and "dump_contrib" [..., N, 3] as MeshAsset.shade_env
    does.  stats (a dict) receives shadow_rays, occluded (counts) and ms per stage (emit, trace, resolve) by event pairs; with
    stats["trace_stats"] = True also the tracer's counters summed over the blocks (n_evals ...)."""
    missing = [k for k in GBUFFER if k not in results]
    if missing:
        raise _lib.IronError("%s: the G-buffer lacks %s" % (WHAT, ", ".join(missing)))
    _args.refuse_cpu(WHAT, *[results[k] for k in GBUFFER], pixel_idx)
    sdf = _as_sdf(sdf)
    n_light, n_brdf = int(n_light), int(n_brdf)
    N = n_light + n_brdf
    if n_light < 0 or n_brdf < 0 or N < 1 or N > 1 << 20:
        raise _lib.IronError("%s: n_light and n_brdf must be >= 0, not both 0, with at most 2^20 samples together" % WHAT)
    if int(max_shadow_rays) < N or int(max_shadow_rays) > (1 << 31) - 65:
        raise _lib.IronError("%s: max_shadow_rays must hold one pixel's %d samples and stay below 2^31 - 64" % (WHAT, N))
    mask = results["convergent_mask"]
    if mask.dtype != torch.bool:
        raise _lib.IronError("%s: convergent_mask must be bool" % WHAT)
    dev = mask.device
    shape = list(mask.shape)
    hit = mask.reshape(-1).contiguous()
    P = int(hit.shape[0])
    g3 = {k: _lib.require_cuda_f32(results[k], k).reshape(-1, 3) for k in ("points", "normal", "ray_d", "diffuse_albedo", "specular_albedo")}
    rough = _lib.require_cuda_f32(results["specular_roughness"], "specular_roughness").reshape(-1)
    for k, t in list(g3.items()) + [("specular_roughness", rough)]:
        if t.shape[0] != P or t.device != dev:
            raise _lib.IronError("%s: %s must have one row per pixel of convergent_mask, on its device" % (WHAT, k))
    lib = _lib.load()
    out = {k: torch.zeros((P, 3), dtype=torch.float32, device=dev) for k in ("color", "diffuse_color", "specular_color")}
    d = _lib.iron_env_dump(None, None, None, None)
    if dump:
        out["dump_dir"] = torch.zeros((P, N, 3), dtype=torch.float32, device=dev)
        out["dump_denom"] = torch.zeros((P, N), dtype=torch.float32, device=dev)
        out["dump_vis"] = torch.zeros((P, N), dtype=torch.uint8, device=dev)
        out["dump_contrib"] = torch.zeros((P, N, 3), dtype=torch.float32, device=dev)
        d = _lib.iron_env_dump(*[out[k].data_ptr() for k in DUMPS])
    timer = _Timer(stats)
    if stats is not None:
        stats.setdefault("shadow_rays", 0)
        stats.setdefault("occluded", 0)
    with torch.cuda.device(dev):
        pix = None if pixel_idx is None else _args.device_array(pixel_idx, torch.int32, dev, "pixel_idx", (), what=WHAT)
        if pix is not None and pix.shape[0] != P:
            raise _lib.IronError("%s: the G-buffer has %d pixels, pixel_idx %d" % (WHAT, P, pix.shape[0]))
        block = min(max(int(max_shadow_rays) // N, 1), max(P, 1))
        cap = block * N
        g = _lib.iron_neural_gbuffer(hit.data_ptr(), g3["points"].data_ptr(), g3["normal"].data_ptr(), g3["ray_d"].data_ptr(),
                                     g3["diffuse_albedo"].data_ptr(), g3["specular_albedo"].data_ptr(), rough.data_ptr(), _lib.ptr(pix), P)
        env = envmap.c_struct()
        tables = _mts_tables(dev)
        st = _lib.stream_ptr(dev)
        ws = _args.sized_workspace(lib.iron_neural_env_workspace_bytes, cap, device=dev, tag="neural_env") if P > 0 else None
        ray_o = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        ray_d = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        idx = torch.empty(cap, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        for p0 in range(0, P, block):
            nb = min(block, P - p0)
            with timer("emit"):
                _lib.check(lib.iron_neural_env_emit(C.byref(g), C.byref(env), p0, nb, n_light, n_brdf, int(seed) & 0xFFFFFFFF, float(shadow_eps),
                                                    cap, ws.data_ptr(), ws.numel(), ray_o.data_ptr(), ray_d.data_ptr(), idx.data_ptr(),
                                                    count.data_ptr(), st))
                m = int(count.item())   # the size of the tracer's call
            occ = None
            with timer("trace"):
                if m > 0:
                    o, w = ray_o[:m], ray_d[:m]
                    work, near, far = intersect_sphere(o, w, r=1.0)
                    want_counters = stats is not None and stats.get("trace_stats")
                    occ = raytracer.occluded(sdf, o, w, near, far, work, collect_stats=bool(want_counters))
                    if want_counters:
                        acc = stats.setdefault("tracer", {})
                        for k, v in (raytracer.last_stats or {}).items():
                            acc[k] = acc.get(k, 0) + v
            with timer("resolve"):
                _lib.check(lib.iron_neural_env_resolve(C.byref(g), C.byref(env), tables[0].data_ptr(), tables[1].data_ptr(), p0, nb, n_light,
                                                       n_brdf, int(seed) & 0xFFFFFFFF, cap, ws.data_ptr(), ws.numel(), _lib.ptr(occ),
                                                       idx.data_ptr(), m, out["color"].data_ptr(), out["diffuse_color"].data_ptr(),
                                                       out["specular_color"].data_ptr(), C.byref(d), st))
            if stats is not None:
                stats["shadow_rays"] += m
                stats["occluded"] += int(occ.sum()) if occ is not None else 0
        timer.finish(stats)
    res = {k: out[k].reshape(shape + [3]) for k in ("color", "diffuse_color", "specular_color")}
    if dump:
        res["dump_dir"], res["dump_contrib"] = out["dump_dir"].reshape(shape + [N, 3]), out["dump_contrib"].reshape(shape + [N, 3])
        res["dump_denom"], res["dump_vis"] = out["dump_denom"].reshape(shape + [N]), out["dump_vis"].reshape(shape + [N])
    return res


def _ggx_render_fn():
    from .network_conf import choose_renderer
    from .rendering_func import make_render_fn
    return make_render_fn(choose_renderer("ggx"))


# the maps relight_camera averages over a pixel's samples (misses count as zero: a box filter over the pixel), as
# mesh_render.render_asset_camera does
AVERAGED = ("color", "diffuse_color", "specular_color", "normal", "diffuse_albedo", "specular_albedo", "specular_roughness", "distance",
            "depth", "points")


@torch.no_grad()
def relight_uv(camera, sdf_network, raytracer, color_network_dict, envmap, uv, n_light=64, n_brdf=64, seed=0, shadow_eps=1e-3,
               background=False, max_shadow_rays=1 << 22, stats=None):
    """One ray per entry of uv [H, W, 2]: raytrace_pixels, render_normal_and_color with the GGX render function (inference; no
    hole filling, no edge pass), then relight_results -> render_camera's dictionary with the three colours replaced."""
    timer = _Timer(stats)
    with timer("gbuffer"):
        res = raytrace_pixels(sdf_network, raytracer, uv, camera)
        res["depth"] = res["depth"] * res["convergent_mask"].float()
        render_normal_and_color(res, sdf_network, color_network_dict, _ggx_render_fn())
    timer.finish(stats)
    lit = relight_results(res, sdf_network, raytracer, envmap, n_light=n_light, n_brdf=n_brdf, seed=seed, shadow_eps=shadow_eps,
                          max_shadow_rays=max_shadow_rays, stats=stats)
    res.update(lit)
    if background:  # the map itself behind the scene
        H, W = res["convergent_mask"].shape
        sky = envmap.lookup(res["ray_d"].reshape(-1, 3)).reshape(H, W, 3)
        res["color"] = torch.where(res["convergent_mask"][..., None], res["color"], sky)
    return res


@torch.no_grad()
def relight_camera(camera, sdf_network, raytracer, color_network_dict, envmap, n_light=64, n_brdf=64, seed=0, shadow_eps=1e-3,
                   samples_per_axis=1, background=False, max_shadow_rays=1 << 22, stats=None):
    """Render the neural scene from `camera` under `envmap`: the G-buffer of render_camera's inference path (GGX render function,
    no hole filling, no edge pass), relit by relight_results.  Returns render_camera's keys with color, diffuse_color and
    specular_color replaced.  The options follow mesh_render.render_asset_env: samples_per_axis = s > 1 casts s^2 rays
    per pixel on the regular sub-pixel grid of subpixel_uvs, sample k with seed + k; the AVERAGED maps are the sum of the frames in
    that order divided by s^2, convergent_mask is coverage >= 1/2, the per-ray keys are the first sample's and uv the pixel centres.
    background=True fills `color` of every ray that misses with envmap.lookup(ray_d), before the averaging."""
    s = int(samples_per_axis)
    if s < 1:
        raise _lib.IronError("samples_per_axis must be >= 1")
    _args.refuse_cpu(WHAT, camera.K)
    kw = dict(n_light=n_light, n_brdf=n_brdf, shadow_eps=shadow_eps, background=background, max_shadow_rays=max_shadow_rays, stats=stats)
    if s == 1:
        return relight_uv(camera, sdf_network, raytracer, color_network_dict, envmap, camera.get_uv(), seed=int(seed), **kw)
    res = coverage = None
    for k, uv in enumerate(subpixel_uvs(camera, s)):
        f = relight_uv(camera, sdf_network, raytracer, color_network_dict, envmap, uv, seed=int(seed) + k, **kw)
        if res is None:
            res, coverage = f, f["convergent_mask"].float()
        else:
            for key in AVERAGED:
                res[key] = res[key] + f[key]
            coverage = coverage + f["convergent_mask"].float()
    for key in AVERAGED:
        res[key] = res[key] / float(s * s)
    res["convergent_mask"] = coverage / float(s * s) >= 0.5
    res["uv"] = camera.get_uv()
    return res
