"""Environment-map relighting of the neural scene (csrc/envlight.hip, the k_nenv_* kernels): the direct integrator
of the exported asset's environment render (mesh_render.render_asset_env) on the trained SDF and material networks
themselves, with sphere-traced shadow rays (RayTracer.occluded) in place of the BVH walk.

A G-buffer -- render_camera's dictionary: convergent_mask, points, normal, ray_d, diffuse_albedo, specular_albedo,
specular_roughness -- is relit in blocks of pixels: the integrator emits the shadow rays of a block's counting samples, the tracer
answers them, the integrator adds the visible samples' terms.  The samples, their random numbers, the balance heuristic and the
order of every sum are those of iron_asset_shade_env; the shading normal stands where that kernel has a geometric normal.  There
is no CPU path: CPU tensors are refused.

max_depth > 1 adds the interreflections (the k_npath_* kernels): the paths of MeshAsset.shade_env_indirect as a
wavefront over depth, a path's state kept on the device between two tracer calls -- per block of pixels and depth the integrator
lists the shadow rays and the bounce rays of the paths that are alive, the tracer answers them (occluded; forward with chunk = 1,
the reference tracer's answer for each ray alone), the surface under the bounce hits is shaded as a G-buffer pixel is, and the
integrator adds the terms and forms the next vertices.  The direct term is untouched.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _args, _lib
from .mesh_render import _mts_tables, check_path_args, subpixel_uvs
from .raytracer import HashFieldSDF, SDFCallable, SDFHandle, as_traceable, intersect_sphere, raytrace_pixels, render_normal_and_color

WHAT = "neural relight"
GBUFFER = ("convergent_mask", "points", "normal", "ray_d", "diffuse_albedo", "specular_albedo", "specular_roughness")
DUMPS = ("dump_dir", "dump_denom", "dump_vis", "dump_contrib")
STAGES = ("emit", "trace", "resolve")
SURFACE = ("normal", "diffuse_albedo", "specular_albedo", "specular_roughness")
# per (pixel, path, vertex): key -> (trailing shape, dtype); per (pixel, path): PATH_DUMPS_PER_PATH
PATH_DUMPS = {"bounce_dir": ((3,), torch.float32), "bounce_org": ((3,), torch.float32), "reached": ((), torch.int32),
              "distance": ((), torch.float32), "vertex_points": ((3,), torch.float32), "vertex_normal": ((3,), torch.float32),
              "vertex_diffuse_albedo": ((3,), torch.float32), "vertex_specular_albedo": ((3,), torch.float32),
              "vertex_roughness": ((), torch.float32), "light_dir": ((3,), torch.float32), "light_vis": ((), torch.uint8),
              "denom_light": ((), torch.float32), "denom_brdf": ((), torch.float32), "light_term": ((3,), torch.float32),
              "escape_term": ((3,), torch.float32), "throughput": ((3,), torch.float32)}
PATH_DUMPS_PER_PATH = ("lobe_diffuse", "lobe_specular", "path_value")
PATH_STAGES = ("path_emit", "path_shadow", "path_bounce", "path_surface", "path_resolve")


def _as_sdf(sdf):
    """What RayTracer.occluded takes: an SDFNetwork is wrapped in its handle; SDFHandle, SDFCallable and HashFieldSDF pass."""
    handle = as_traceable(sdf)
    if handle is not None:
        return handle
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
                    max_shadow_rays=1 << 22, dump=False, stats=None, max_depth=1, n_paths=64, surface_fn=None, color_network_dict=None):
    """Relight the G-buffer `results` (the GBUFFER keys, [..., 3] / [...]; the tensors may come from anywhere, on one GPU) under
    `envmap` (EnvMap): per hit pixel the sum over n_light environment samples and n_brdf BRDF samples of
    L(w) roughplastic_point(n, -ray_d, w) V(w) / (n_light p_light(w) + n_brdf p_brdf(w)), the multi-sample balance heuristic of
    iron_asset_shade_env with the same random numbers (seed, pixel_idx [P] int32 or the pixel's position, sample, dimension).  A
    sample counts when n.w > 0, n.v > 0 and w is finite; V(w) = 1 when it counts and the shadow ray from x + shadow_eps n along w,
    cut to the unit sphere by intersect_sphere, is not raytracer.occluded(sdf, ...); a ray that misses the sphere is visible.
    shadow_eps (default 1e-3 = 20 x the tracer's sdf_threshold) is a parameter, not a measurement.

    `sdf`: an SDFNetwork, an SDFHandle or an SDFCallable; a HashFieldSDF (TCNNSDF.as_traced) is taken by occluded / forward(chunk=1)
    like any handle and, as an SDFCallable does, needs a surface_fn above max_depth 1.  Pixels are worked in blocks of max_shadow_rays // (n_light + n_brdf),
    which bounds the memory (about 170 bytes per shadow ray) and changes no bit of the result.  Every block waits once for the host
    to read the number of its shadow rays, the size of the tracer's call.
    -> {"color", "diffuse_color", "specular_color"} [..., 3], color = diffuse_color + specular_color, zeros on a miss; dump=True adds
    "dump_dir" [..., N, 3], "dump_denom" [..., N], "dump_vis" [..., N] uint8 and "dump_contrib" [..., N, 3] as MeshAsset.shade_env
    does.  stats (a dict) receives shadow_rays, occluded (counts) and ms per stage (emit, trace, resolve) by event pairs; with
    stats["trace_stats"] = True also the tracer's counters summed over the blocks (n_evals ...).

    max_depth (1 .. 8): the largest number of surface vertices on a light path, the primary hit included.  1 is the direct term
    alone: nothing else runs and no key is added.  Above 1, n_paths (1 .. 2^16) paths per pixel add the interreflections (DESIGN.md
    §20; the direct term is unchanged): the result gains indirect_diffuse, indirect_specular and indirect_color (their sum);
    diffuse_color and specular_color become direct + indirect of that lobe and color their sum.  Path p of a pixel draws
    env_rand(seed, pixel, p, 8 (j + 1) + c) at vertex j (the direct term uses dimensions 0 .. 2).  A bounce ray leaves
    x + shadow_eps n, is cut to the unit sphere, and its closest hit is raytracer.forward(..., chunk=1); the surface there is
    surface_fn(points [M, 3], ray_d [M, 3]) -> {normal (unit), diffuse_albedo, specular_albedo [M, 3], specular_roughness [M]}, or,
    when surface_fn is None, render_normal_and_color with the fused GGX render function on `sdf` (an SDFNetwork, or its handle) and
    color_network_dict, the call that shades a G-buffer pixel.  An SDFCallable needs a surface_fn.  Pixels are worked in blocks of
    max_shadow_rays // n_paths (at most one shadow ray and one bounce ray per path and depth), which changes no bit; every block and
    depth waits once for the host to read the two ray counts.  dump=True adds, per (pixel, path, vertex) [..., n_paths, max_depth(, 3)],
    "dump_" + each key of PATH_DUMPS and, per (pixel, path), "dump_lobe_diffuse", "dump_lobe_specular", "dump_path_value"
    (include/iron_hip.h: iron_neural_path_dump).  stats gains bounce_rays, bounce_hits, indirect_shadow_rays, indirect_occluded,
    alive (a list: the alive paths at every depth) and ms for the PATH_STAGES; with stats["trace_stats"] = True also bounce_tracer,
    the tracer's counters summed over the bounce calls."""
    check_path_args(max_depth, n_paths)
    max_depth, n_paths = int(max_depth), int(n_paths)
    surface = None
    if max_depth > 1:
        if int(max_shadow_rays) < n_paths:
            raise _lib.IronError("%s: max_shadow_rays must hold one pixel's %d paths" % (WHAT, n_paths))
        surface = _surface(sdf, surface_fn, color_network_dict)
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
        ind = None
        if max_depth > 1:  # the interreflections, lobe by lobe; the direct term above is untouched
            ind = _indirect(g, P, dev, sdf, raytracer, env, tables, st, n_paths, max_depth, int(seed) & 0xFFFFFFFF, float(shadow_eps),
                            int(max_shadow_rays), surface, dump, stats, timer)
        timer.finish(stats)
    if ind is not None:
        out["indirect_diffuse"], out["indirect_specular"] = ind.pop("indirect_diffuse"), ind.pop("indirect_specular")
        out["indirect_color"] = out["indirect_diffuse"] + out["indirect_specular"]
        out["diffuse_color"] = out["diffuse_color"] + out["indirect_diffuse"]
        out["specular_color"] = out["specular_color"] + out["indirect_specular"]
        out["color"] = out["diffuse_color"] + out["specular_color"]
    res = {k: out[k].reshape(shape + [3]) for k in ("color", "diffuse_color", "specular_color", "indirect_diffuse", "indirect_specular",
                                                    "indirect_color") if k in out}
    if dump:
        res["dump_dir"], res["dump_contrib"] = out["dump_dir"].reshape(shape + [N, 3]), out["dump_contrib"].reshape(shape + [N, 3])
        res["dump_denom"], res["dump_vis"] = out["dump_denom"].reshape(shape + [N]), out["dump_vis"].reshape(shape + [N])
        for k, t in (ind or {}).items():
            res[k] = t.reshape(shape + list(t.shape[1:]))
    return res


def _surface(sdf, surface_fn, color_network_dict):
    """-> f(ray_o, ray_d, points [m, 3], hit [m] bool) -> the SURFACE keys, one row per ray (rows without a hit are not read)."""
    if surface_fn is not None:
        if not callable(surface_fn):
            raise _lib.IronError("%s: surface_fn must be callable" % WHAT)

        def from_fn(ray_o, ray_d, points, hit):
            at = torch.nonzero(hit)[:, 0]
            M, dev = int(at.shape[0]), points.device
            got = surface_fn(points.index_select(0, at).contiguous(), ray_d.index_select(0, at).contiguous())
            if not isinstance(got, dict) or any(k not in got for k in SURFACE):
                raise _lib.IronError("%s: surface_fn must return a dictionary with %s" % (WHAT, ", ".join(SURFACE)))
            full = {}
            for k in SURFACE:
                want = (M,) if k == "specular_roughness" else (M, 3)
                v = got[k]
                if not torch.is_tensor(v) or not v.is_cuda or v.device != dev or v.dtype != torch.float32 or tuple(v.shape) != want:
                    raise _lib.IronError("%s: surface_fn's %s must be a float32 tensor of shape %s on the device of its arguments"
                                         % (WHAT, k, list(want)))
                full[k] = torch.zeros((points.shape[0],) + want[1:], dtype=torch.float32, device=dev).index_copy_(0, at, v.contiguous())
            return full
        return from_fn
    if isinstance(sdf, (SDFCallable, HashFieldSDF)):
        raise _lib.IronError("%s: interreflections on %s need a surface_fn"
                             % (WHAT, "an SDFCallable" if isinstance(sdf, SDFCallable) else "a HashFieldSDF"))
    net = sdf.sdf_network if isinstance(sdf, SDFHandle) else sdf
    if not hasattr(net, "hip_net") or not hasattr(net, "get_all"):
        raise _lib.IronError("%s: interreflections need an iron_amd SDFNetwork (or its handle), or a surface_fn" % WHAT)
    if color_network_dict is None:
        raise _lib.IronError("%s: interreflections need color_network_dict (the material networks), or a surface_fn" % WHAT)
    render_fn = _ggx_render_fn()

    def from_networks(ray_o, ray_d, points, hit):
        rec = {"ray_o": ray_o, "ray_d": ray_d, "points": points, "convergent_mask": hit}
        render_normal_and_color(rec, net, color_network_dict, render_fn)
        return {k: rec[k].contiguous() for k in SURFACE}
    return from_networks


@torch.no_grad()
def closest_hits(raytracer, sdf, ray_o, ray_d, near, far, work, collect_stats=False):
    """raytracer.forward(sdf, ..., chunk=1) on the rays that hit: every ray traced as a reference call of its own (its own bisection
    count), so what a ray gets does not depend on the rays beside it.  For an SDFNetwork that is one fused call.  For an SDFCallable
    forward's chunk = 1 is a host loop over the rays, and only the rays a call bisects depend on the call: the rays the sphere-tracing
    stage finishes hold their answer after it, a ray's convergent_mask is final once the sampler has looked for a sign change, and
    a ray that misses is not read.  So the whole list is traced once, and the rays that sphere tracing left unfinished and that
    then converged -- the bisected ones -- are traced again one by one.  collect_stats: the fused tracer's counters of the call in
    raytracer.last_stats (an SDFNetwork only)."""
    if not isinstance(sdf, SDFCallable):
        return raytracer.forward(sdf, ray_o, ray_d, near, far, work, chunk=1, collect_stats=collect_stats)
    _, unfinished, _, _, _ = raytracer.sphere_tracing(sdf, ray_o, ray_d, near, far, work)
    res = raytracer.forward(sdf, ray_o, ray_d, near, far, work)
    for k in torch.nonzero(unfinished & res["convergent_mask"])[:, 0].tolist():
        one = raytracer.forward(sdf, ray_o[k:k + 1], ray_d[k:k + 1], near[k:k + 1], far[k:k + 1], work[k:k + 1])
        for key in res:
            res[key][k] = one[key][0]
    return res


def _indirect(g, P, dev, sdf, raytracer, env, tables, st, n_paths, max_depth, seed, shadow_eps, max_shadow_rays, surface, dump, stats, timer):
    """The wavefront of DESIGN.md §20 over the G-buffer `g` -> indirect_diffuse, indirect_specular [P, 3] and the dumps."""
    lib = _lib.load()
    out = {k: torch.zeros((P, 3), dtype=torch.float32, device=dev) for k in ("indirect_diffuse", "indirect_specular")}
    d = _lib.iron_neural_path_dump()
    if dump:
        for k, (tail, dtype) in PATH_DUMPS.items():
            out["dump_" + k] = torch.full((P, n_paths, max_depth) + tail, -2 if k == "reached" else 0, dtype=dtype, device=dev)
        for k in PATH_DUMPS_PER_PATH:
            out["dump_" + k] = torch.zeros((P, n_paths, 3), dtype=torch.float32, device=dev)
        for k in _lib.NEURAL_PATH_DUMP_FIELDS:
            setattr(d, k, out["dump_" + k].data_ptr())
    if stats is not None:
        for k in ("bounce_rays", "bounce_hits", "indirect_shadow_rays", "indirect_occluded"):
            stats.setdefault(k, 0)
        alive_at = stats.setdefault("alive", [])
        alive_at.extend([0] * (max_depth - len(alive_at)))
    if P == 0:
        return out
    block = min(max(max_shadow_rays // n_paths, 1), P)
    cap = block * n_paths
    ws = _args.sized_workspace(lib.iron_neural_path_workspace_bytes, cap, device=dev, tag="neural_path")
    rays = [torch.empty((cap, 3), dtype=torch.float32, device=dev) for _ in range(4)]   # shadow o, d; bounce o, d
    idx = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2)]
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    for p0 in range(0, P, block):
        nb = min(block, P - p0)
        common = (p0, nb, n_paths, max_depth)
        with timer("path_emit"):
            _lib.check(lib.iron_neural_path_begin(C.byref(g), *common, cap, ws.data_ptr(), ws.numel(), st))
        for j in range(max_depth):
            with timer("path_emit"):
                _lib.check(lib.iron_neural_path_emit(C.byref(g), C.byref(env), *common, j, seed, shadow_eps, cap, ws.data_ptr(), ws.numel(),
                                                     rays[0].data_ptr(), rays[1].data_ptr(), idx[0].data_ptr(), rays[2].data_ptr(),
                                                     rays[3].data_ptr(), idx[1].data_ptr(), counts.data_ptr(), st))
                ms_, mb, alive = (int(x) for x in counts.tolist())   # the sizes of the tracer's two calls: one read
            if stats is not None:
                stats["alive"][j] += alive
            if alive == 0:
                break   # nothing left to resolve: the dumps of the depths from here on keep "no ray" and zeros
            occ = None
            with timer("path_shadow"):
                if ms_ > 0:
                    o, w = rays[0][:ms_], rays[1][:ms_]
                    work, near, far = intersect_sphere(o, w, r=1.0)
                    occ = raytracer.occluded(sdf, o, w, near, far, work)
            b = _lib.iron_neural_bounce()
            keep = None
            if mb > 0:
                with timer("path_bounce"):
                    o, w = rays[2][:mb], rays[3][:mb]
                    work, near, far = intersect_sphere(o, w, r=1.0)
                    want_counters = stats is not None and bool(stats.get("trace_stats")) and not isinstance(sdf, SDFCallable)
                    tr = closest_hits(raytracer, sdf, o, w, near, far, work, collect_stats=want_counters)
                    if want_counters:
                        acc = stats.setdefault("bounce_tracer", {})
                        for k, v in (raytracer.last_stats or {}).items():
                            acc[k] = acc.get(k, 0) + v
                    hit = tr["convergent_mask"].contiguous()
                with timer("path_surface"):
                    rec = surface(o, w, tr["points"], hit)
                keep = (hit, tr["distance"].contiguous(), tr["points"].contiguous(), rec)
                b.hit, b.distance, b.points = hit.data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
                b.normal, b.diffuse_albedo, b.specular_albedo = (rec[k].data_ptr() for k in SURFACE[:3])
                b.specular_roughness = rec["specular_roughness"].data_ptr()
            with timer("path_resolve"):
                _lib.check(lib.iron_neural_path_resolve(C.byref(g), C.byref(env), tables[0].data_ptr(), tables[1].data_ptr(), *common, j, seed,
                                                        shadow_eps, cap, ws.data_ptr(), ws.numel(), _lib.ptr(occ), ms_, C.byref(b), mb,
                                                        C.byref(d), st))
            if stats is not None:
                stats["indirect_shadow_rays"] += ms_
                stats["indirect_occluded"] += int(occ.sum()) if occ is not None else 0
                stats["bounce_rays"] += mb
                stats["bounce_hits"] += int(keep[0].sum()) if keep is not None else 0
            del keep
        with timer("path_resolve"):
            _lib.check(lib.iron_neural_path_finish(C.byref(g), *common, cap, ws.data_ptr(), ws.numel(), out["indirect_diffuse"].data_ptr(),
                                                   out["indirect_specular"].data_ptr(), C.byref(d), st))
    return out


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
               background=False, max_shadow_rays=1 << 22, stats=None, max_depth=1, n_paths=64):
    """One ray per entry of uv [H, W, 2]: raytrace_pixels, render_normal_and_color with the GGX render function (inference; no
    hole filling, no edge pass), then relight_results -> render_camera's dictionary with the three colours replaced; max_depth > 1
    adds indirect_color (relight_results: the bounce hits are shaded by the same networks)."""
    timer = _Timer(stats)
    with timer("gbuffer"):
        res = raytrace_pixels(sdf_network, raytracer, uv, camera)
        res["depth"] = res["depth"] * res["convergent_mask"].float()
        render_normal_and_color(res, sdf_network, color_network_dict, _ggx_render_fn())
    timer.finish(stats)
    lit = relight_results(res, sdf_network, raytracer, envmap, n_light=n_light, n_brdf=n_brdf, seed=seed, shadow_eps=shadow_eps,
                          max_shadow_rays=max_shadow_rays, stats=stats, max_depth=max_depth, n_paths=n_paths,
                          color_network_dict=color_network_dict)
    lit.pop("indirect_diffuse", None), lit.pop("indirect_specular", None)   # diffuse_color and specular_color carry them
    res.update(lit)
    if background:  # the map itself behind the scene
        H, W = res["convergent_mask"].shape
        sky = envmap.lookup(res["ray_d"].reshape(-1, 3)).reshape(H, W, 3)
        res["color"] = torch.where(res["convergent_mask"][..., None], res["color"], sky)
    return res


@torch.no_grad()
def relight_camera(camera, sdf_network, raytracer, color_network_dict, envmap, n_light=64, n_brdf=64, seed=0, shadow_eps=1e-3,
                   samples_per_axis=1, background=False, max_shadow_rays=1 << 22, stats=None, max_depth=1, n_paths=64):
    """Render the neural scene from `camera` under `envmap`: the G-buffer of render_camera's inference path (GGX render function,
    no hole filling, no edge pass), relit by relight_results.  Returns render_camera's keys with color, diffuse_color and
    specular_color replaced.  The options follow mesh_render.render_asset_env: samples_per_axis = s > 1 casts s^2 rays
    per pixel on the regular sub-pixel grid of subpixel_uvs, sample k with seed + k; the AVERAGED maps are the sum of the frames in
    that order divided by s^2, convergent_mask is coverage >= 1/2, the per-ray keys are the first sample's and uv the pixel centres.
    background=True fills `color` of every ray that misses with envmap.lookup(ray_d), before the averaging.
    max_depth (1 .. 8) and n_paths (1 .. 2^16) as in render_asset_env: above 1 the interreflections of relight_results are added,
    the dictionary gains indirect_color (averaged like the colours), frame k keeps seed + k for both passes, and color is
    diffuse_color + specular_color of the averaged maps."""
    s = int(samples_per_axis)
    if s < 1:
        raise _lib.IronError("samples_per_axis must be >= 1")
    check_path_args(max_depth, n_paths)
    _args.refuse_cpu(WHAT, camera.K)
    kw = dict(n_light=n_light, n_brdf=n_brdf, shadow_eps=shadow_eps, background=background, max_shadow_rays=max_shadow_rays, stats=stats,
              max_depth=int(max_depth), n_paths=int(n_paths))
    if s == 1:
        return relight_uv(camera, sdf_network, raytracer, color_network_dict, envmap, camera.get_uv(), seed=int(seed), **kw)
    res = coverage = None
    for k, uv in enumerate(subpixel_uvs(camera, s)):
        f = relight_uv(camera, sdf_network, raytracer, color_network_dict, envmap, uv, seed=int(seed) + k, **kw)
        if res is None:
            res, coverage = f, f["convergent_mask"].float()
            averaged = AVERAGED + tuple(key for key in ("indirect_color",) if key in f)
        else:
            for key in averaged:
                res[key] = res[key] + f[key]
            coverage = coverage + f["convergent_mask"].float()
    for key in averaged:
        res[key] = res[key] / float(s * s)
    if "indirect_color" in res:   # as render_asset_env: the colour of the averaged lobes
        lobes = res["diffuse_color"] + res["specular_color"]
        # a pixel with a ray that misses under background=True keeps the mean of its frames' colours, which holds the map
        res["color"] = torch.where((coverage >= float(s * s))[..., None], lobes, res["color"]) if background else lobes
    res["convergent_mask"] = coverage / float(s * s) >= 0.5
    res["uv"] = camera.get_uv()
    return res
