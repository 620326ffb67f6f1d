"""GPU: environment-map relighting of the neural scene (iron_amd/neural_relight.py, RayTracer.occluded, csrc/envlight.hip k_nenv_*;
DESIGN.md §19).  The occlusion query is pinned to RayTracer.forward's own mask (bitwise) and to the oracle tracer's fp64 run; the
integrator to the fp64 restatement of tests/_envlight_oracle.py and, bit for bit, to the mesh integrator on a scene both can light.

Bounds described as measured are the oracle's own fp32 evaluation against its fp64 one on the same inputs, times 4, with a floor
of 1e-6 (tests/test_gpu_envlight.py): what fp32 can give, not what the kernel gives.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _envlight_oracle as EO
import _hard_fields as HF
import _neuralenv_oracle as NO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_MARGIN = 1e-4   # tests/test_gpu_envlight.py: coordinates closer than this to a texel / table step may resolve either way in fp32
STEP_SHARE = 5e-3
SIDE_MARGIN = 1e-6   # |n.w|, |n.v| below this: whether the sample counts may resolve either way in fp32
SEED = 5


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def tables():
    from iron_amd.renderer_ggx import load_mts_tables
    return tuple(t.to(dev()) for t in load_mts_tables())


def measured(a32, a64, relative, keep=None):
    """4 x the largest error of the oracle's fp32 evaluation against its fp64 one, floor 1e-6"""
    e = (a32.double() - a64).abs()
    if relative:
        e = e / a64.abs().clamp_min(1e-300)
    if keep is not None:
        e = e[keep]
    return max(4 * float(e.max()) if e.numel() else 0.0, 1e-6)


def per_sample(x, N):
    return x[:, None].expand(x.shape[0], N, *x.shape[1:]).reshape(-1, *x.shape[1:])


@functools.lru_cache(maxsize=None)
def net_on_device(name):
    return NO.build(name).to(dev())   # a second build: the oracle's copy stays on the CPU, parameters bit-identical


def ray_sets(name):
    """(label, o, d, near, far, work) on the device: the 56 x 56 fixture view and the shadow rays of the recipe"""
    f = lambda *xs: tuple(x.to(dev()) for x in xs)  # noqa: E731
    ro, rd, near, far, hit = HF.fixture_rays(56, NO.yaw_of(name))
    s = NO.shadow_rays(name)
    return (("view",) + f(ro, rd, near, far, hit), ("shadow",) + f(s.o, s.w, s.near, s.far, s.work))


# ---- 1. occluded is forward's mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NO.FIELDS))
def test_occluded_is_forwards_mask_bitwise(name):
    from iron_amd import _lib
    from iron_amd.raytracer import RayTracer, SDFCallable, SDFHandle
    net = net_on_device(name)
    sdf, tr, lib = SDFHandle(net), RayTracer(), _lib.load()
    for label, o, d, near, far, work in ray_sets(name):
        n = o.shape[0]
        fwd = tr.forward(sdf, o, d, near, far, work)["convergent_mask"]
        occ = tr.occluded(sdf, o, d, near, far, work)
        print("%s %s: %d rays, %d in the sphere, %d occluded" % (name, label, n, int(work.sum()), int(occ.sum())))
        assert occ.dtype == torch.bool and occ.shape == (n,)
        assert torch.equal(occ, fwd), (name, label)
        assert not bool(occ[~work].any())
        if label == "view":
            assert 0 < int(occ.sum()) < n
        # a work mask with holes
        holes = work & (torch.arange(n, device=dev()) % 3 != 0)
        assert torch.equal(tr.occluded(sdf, o, d, near, far, holes), tr.forward(sdf, o, d, near, far, holes)["convergent_mask"]), (name, label)
        # no work mask: every ray
        if label == "shadow":
            every = torch.ones_like(work)
            assert torch.equal(tr.occluded(sdf, o, d, near, far), tr.forward(sdf, o, d, near, far, every)["convergent_mask"]), (name, label)
        # the screen's and the stride's switches change nothing
        for setter in (lib.iron_set_sampler_stride, lib.iron_set_sampler_screen):
            prev = setter(0)
            try:
                off = tr.occluded(sdf, o, d, near, far, work)
            finally:
                setter(prev)
            assert torch.equal(off, occ), (name, label)
        # an opaque callable: forward's mask of that form (not shortened)
        if label == "shadow":
            fn = SDFCallable(lambda x: net.sdf(x)[..., 0])
            assert torch.equal(tr.occluded(fn, o, d, near, far, work), tr.forward(fn, o, d, near, far, work)["convergent_mask"]), name


def test_occluded_refuses_what_forward_refuses():
    from iron_amd._lib import IronError
    from iron_amd.raytracer import RayTracer, SDFHandle
    net = net_on_device("S0")
    _, o, d, near, far, work = ray_sets("S0")[1]
    tr = RayTracer()
    with pytest.raises(IronError):
        tr.occluded(lambda x: x[:, 0], o, d, near, far, work)          # a bare callable that wraps no network
    with pytest.raises(IronError):
        tr.occluded(SDFHandle(net), o.cpu(), d, near, far, work)       # CPU tensors
    with pytest.raises(IronError):
        tr.occluded(SDFHandle(net), o, d, near, far, work.cpu())
    assert tr.occluded(SDFHandle(net), o[:0], d[:0], near[:0], far[:0], work[:0]).shape == (0,)


# ---- 2. visibility against the fp64 oracle -----------------------------------------------------------------------------------------
def test_visibility_against_the_fp64_oracle():
    from iron_amd.raytracer import RayTracer, SDFHandle
    tr = RayTracer()
    for name in ("bumpy04_s1", "S0"):
        _, o, d, near, far, work = ray_sets(name)[1]
        occ = tr.occluded(SDFHandle(net_on_device(name)), o, d, near, far, work).cpu()
        o64 = NO.oracle_occluded(name, "fp64")
        gap = NO.precision_gap(name)
        share = float((occ != o64).double().mean())
        print("%s: %d shadow rays, occluded %d (device) / %d (oracle fp64); differing share %.3e, the oracle's own fp32 against fp64 %.3e "
              "(bound: that + %g)" % (name, occ.numel(), int(occ.sum()), int(o64.sum()), share, gap, EO.VIS_SHARE))
        assert share <= gap + EO.VIS_SHARE
        if name == "S0":
            assert int(occ.sum()) == 0
        else:
            assert 0 < int(occ.sum()) < occ.numel()


# ---- 3. the integrator, through the dumps ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def material_nets():
    from iron_amd import scenes
    return {k: v.to(dev()) for k, v in scenes.build_networks("S0").items() if k != "sdf_network"}


@functools.lru_cache(maxsize=None)
def bumpy_gbuffer():
    """The product's render_camera (no edge pass: the G-buffer of relight_camera) on bumpy04_s1 at 33 x 31, flattened."""
    from iron_amd import scenes
    from iron_amd.neural_relight import GBUFFER, _ggx_render_fn
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    K, W2C = scenes.fixture_camera_matrices(33, 31, 0.0)
    cam = Camera(33, 31, K.to(dev()), W2C.to(dev()))
    res = render_camera(cam, net_on_device("bumpy04_s1"), RayTracer(), material_nets(), _ggx_render_fn(), handle_edges=False)
    torch.cuda.synchronize()
    return {k: res[k].reshape(33 * 31, -1).squeeze(-1).contiguous() for k in GBUFFER}


@functools.lru_cache(maxsize=None)
def hot_env():
    from iron_amd.envmap import EnvMap
    hot = EO.hot_map().to(dev())
    return EnvMap(hot.float()), EO.EnvOracle(hot), EO.EnvOracle(hot, dtype=torch.float32)


def relight(gb, sdf, env, n_light, n_brdf, seed=SEED, **kw):
    from iron_amd.neural_relight import relight_results
    from iron_amd.raytracer import RayTracer
    out = relight_results(gb, sdf, RayTracer(), env, n_light=n_light, n_brdf=n_brdf, seed=seed, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("counts", [(5, 3), (8, 0), (0, 8), (64, 64)])
def test_integrator_through_the_dumps(counts):
    from iron_amd.raytracer import RayTracer, SDFHandle, intersect_sphere
    gb = bumpy_gbuffer()
    env, e64, e32 = hot_env()
    net = net_on_device("bumpy04_s1")
    n_light, n_brdf = counts
    N = n_light + n_brdf
    eps = 1e-3
    out = relight(gb, net, env, n_light, n_brdf, dump=True)
    hit = gb["convergent_mask"]
    P = int(hit.sum())
    assert 100 < P < hit.numel() - 100  # hits and misses interleaved
    pix = torch.nonzero(hit)[:, 0]
    nrm32, x32, d32 = gb["normal"][hit], gb["points"][hit], gb["ray_d"][hit]
    nrm, v = nrm32.double(), -d32.double()
    kd, ks, rough = gb["diffuse_albedo"][hit].double(), gb["specular_albedo"][hit].double(), gb["specular_roughness"][hit].double()
    alpha = rough.clamp(min=1e-4)
    w32 = out["dump_dir"][hit].reshape(-1, 3)
    w = w32.double()
    den = out["dump_denom"][hit].reshape(-1).double()
    vis = out["dump_vis"][hit].reshape(-1).bool()
    con = out["dump_contrib"][hit].reshape(-1, 3).double()
    # (a) directions and denominators against the oracle's, from the restated random numbers
    S64 = EO.pixel_samples(e64, nrm, v, alpha, pix, n_light, n_brdf, SEED)
    S32 = EO.pixel_samples(e32, nrm, v, alpha, pix, n_light, n_brdf, SEED, dtype=torch.float32)
    flipped = S64["gap"] <= 4
    odd = S64["ok"] != (w != 0).any(-1)  # a GGX sample whose v.h changes sign between fp32 and fp64
    anywhere = torch.tensor([0.3, 0.5, 0.8], dtype=torch.float64, device=dev())
    clear = (e64.texel_margin(torch.where(S64["ok"][:, None], S64["dir"], anywhere[None])) >= STEP_MARGIN) | ~S64["ok"]
    is_light = (torch.arange(N, device=dev()) < n_light)[None].expand(P, N).reshape(-1)
    good = ~flipped & ~odd & (clear | is_light)
    bdir = measured(S32["dir"], S64["dir"], False, keep=(good & (S32["ok"] == S64["ok"]))[:, None].expand(-1, 3))
    # denominators are compared where the sample can count at all (the shading normal in the geometric normal's place): opposite the
    # viewer v + w cancels and the half vector of the GGX density is rounding noise in fp32; V is 0 there anyway
    n_s, v_s = per_sample(nrm, N), per_sample(v, N)
    side = (EO._dot(n_s, S64["dir"]) > 0) & (EO._dot(n_s, v_s) > 0)
    pos = good & side & (S64["denom"] > 0) & torch.isfinite(S64["denom"])
    bden = measured(S32["denom"], S64["denom"], True, keep=pos & (S32["ok"] == S64["ok"]))
    edir = float((w - S64["dir"]).abs()[good].max())
    eden = float(((den - S64["denom"]).abs() / S64["denom"].clamp_min(1e-300))[pos].max())
    print("%s: hits %d, samples %d; near a CDF boundary %d, v.h sign changes %d, near a texel boundary %d; |dir error| %.3e (measured "
          "bound %.3e), denominator rel error %.3e (measured bound %.3e)"
          % (counts, P, P * N, int(flipped.sum()), int(odd.sum()), int((~clear & ~is_light).sum()), edir, bdir, eden, bden))
    assert float(flipped.double().mean()) <= EO.FLIP_SHARE and float(odd.double().mean()) <= 1e-4
    assert float((~clear & ~is_light).double().mean()) <= STEP_SHARE
    assert edir <= bdir and eden <= bden
    assert (den[good & (S64["denom"] == 0)] == 0).all()
    if n_brdf == 0:
        assert float(((den - n_light * S64["p_light"]).abs() / S64["denom"].clamp_min(1e-300))[pos].max()) <= bden
    if n_light == 0:
        assert float(((den - n_brdf * S64["p_brdf"]).abs() / S64["denom"].clamp_min(1e-300))[pos].max()) <= bden
    # (b) visibility is the tracer's answer, bitwise: the shadow rays rebuilt here from the dumped directions and x + eps n (one
    # rounding per product and sum: torch's separate mul and add), cut by intersect_sphere, through RayTracer.occluded
    nw, nv = EO._dot(n_s, w), EO._dot(n_s, v_s)
    sample = (w != 0).any(-1) & torch.isfinite(w).all(-1)
    decided = (nw.abs() > SIDE_MARGIN) & (nv.abs() > SIDE_MARGIN)
    counting = sample & (nw > 0) & (nv > 0)
    cast = decided & counting & (den > 0)
    org = (per_sample(x32, N) + eps * per_sample(nrm32, N))[cast].contiguous()
    way = w32[cast].contiguous()
    work, near, far = intersect_sphere(org, way, r=1.0)
    occ = torch.zeros_like(cast)
    occ[cast] = RayTracer().occluded(SDFHandle(net), org, way, near, far, work)
    print("%s: visible %d of %d; counting samples %d, of which occluded %d; undecided sides %d"
          % (counts, int(vis.sum()), vis.numel(), int(cast.sum()), int((cast & occ).sum()), int((~decided).sum())))
    assert float((~decided & sample).double().mean()) <= EO.VIS_SHARE
    assert torch.equal(vis[cast], ~occ[cast])
    assert not bool(vis[decided & ~counting].any()) and not bool(vis[~sample].any())
    assert 0 < int((cast & occ).sum()) < int(cast.sum())
    # (c) every sample's term, and the sums, from the device's own directions, denominators and visibility in fp64
    kds, kss, rs = per_sample(kd, N), per_sample(ks, N), per_sample(rough, N)
    td64, ts64 = EO.sample_terms(e64, n_s, v_s, kds, kss, rs, w, den, vis, tables(), texel=S64["texel"])
    f32d, f32s = EO.roughplastic_point(n_s, v_s, w, kds, kss, rs, tables(), dtype=torch.float32)
    f64d, f64s = EO.roughplastic_point(n_s, v_s, w, kds, kss, rs, tables())
    step_clear = (EO.table_margin(n_s, v_s, w, rs) >= STEP_MARGIN) & (clear | is_light) & ~flipped
    lit = (vis & (den > 0) & step_clear)[:, None].expand(-1, 3)
    bf = measured(f32d + f32s, f64d + f64s, True, keep=lit) + 4e-7  # and the product with L and the division, one rounding each
    tot = td64 + ts64
    eterm = float(((con - tot).abs() / tot.abs().clamp_min(1e-300))[lit].max())
    print("%s: per-sample term rel error %.3e (measured bound %.3e); near a table step %d" % (counts, eterm, bf, int((~step_clear).sum())))
    assert float((~step_clear).double().mean()) <= 2 * STEP_SHARE
    assert eterm <= bf
    assert (con[~vis] == 0).all()
    col = out["color"][hit].double()
    s_abs = con.abs().reshape(P, N, 3).sum(1)
    esum = float(((col - con.reshape(P, N, 3).sum(1)).abs() / s_abs.clamp_min(1e-300))[s_abs > 0].max())
    print("%s: colour against the fp64 sum of the dumped terms: %.3e of the sum of absolute terms (bound 1e-5)" % (counts, esum))
    assert esum <= 1e-5
    assert (col[s_abs == 0] == 0).all()
    assert torch.equal(out["color"], out["diffuse_color"] + out["specular_color"])
    # (e) misses write zeros everywhere
    for key in ("color", "diffuse_color", "specular_color", "dump_dir", "dump_denom", "dump_vis", "dump_contrib"):
        assert (out[key][~hit] == 0).all(), key
    # (d) bitwise: a second run, without the dumps, a sub-rectangle with its own pixel indices, and another block size
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731
    again = relight(gb, net, env, n_light, n_brdf, dump=True)
    plain = relight(gb, net, env, n_light, n_brdf)
    small = relight(gb, net, env, n_light, n_brdf, dump=True, max_shadow_rays=1000)
    rect = (torch.arange(31)[:, None] * 33 + torch.arange(33)[None, :])[7:20, 5:23].reshape(-1).to(dev())
    part = relight({k: t[rect] for k, t in gb.items()}, net, env, n_light, n_brdf, pixel_idx=rect.int())
    for key in ("color", "diffuse_color", "specular_color"):
        for other, idx in ((plain, None), (again, None), (small, None), (part, rect)):
            assert torch.equal(bits(out[key]) if idx is None else bits(out[key])[idx], bits(other[key])), key
    for key in ("dump_dir", "dump_denom", "dump_vis", "dump_contrib"):
        assert torch.equal(bits(out[key]), bits(again[key])) and torch.equal(bits(out[key]), bits(small[key])), key
    other_seed = relight(gb, net, env, n_light, n_brdf, seed=SEED + 1)
    assert not torch.equal(other_seed["color"], out["color"])


def test_relight_results_refusals():
    from iron_amd._lib import IronError
    gb = bumpy_gbuffer()
    env, _, _ = hot_env()
    net = net_on_device("bumpy04_s1")
    with pytest.raises(IronError):
        relight({k: v.cpu() for k, v in gb.items()}, net, env, 4, 4)
    with pytest.raises(IronError):
        relight(gb, lambda x: x[:, 0], env, 4, 4)
    with pytest.raises(IronError):
        relight(gb, net, env, 0, 0)
    with pytest.raises(IronError):
        relight(gb, net, env, 4, 4, max_shadow_rays=7)
    with pytest.raises(IronError):
        relight({k: v for k, v in gb.items() if k != "normal"}, net, env, 4, 4)


# ---- 4. one integrator, two scenes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(5, 3), (64, 64)])
def test_one_integrator_two_scenes(counts):
    """The floor scene of the mesh integrator's tests, face normals as shading normals (shading and geometric normal are then one
    vector, and the two integrators' counting rules one rule): its hits and materials as a G-buffer, under an SDF that is 1
    everywhere, so that nothing is occluded."""
    from iron_amd.mesh_render import MeshAsset
    from iron_amd.raytracer import SDFCallable
    env, _, _ = hot_env()
    sc = EO.scene("floor")
    f = lambda x: x.float().to(dev())  # noqa: E731
    asset = MeshAsset(f(sc["V"]), sc["F"].to(dev()), f(sc["uvs"]), sc["face_uvs"].to(dev()), f(sc["material"]), normals="face")
    o, d = (f(x) for x in EO.scene_rays(sc))
    t, face, bary = asset.bvh.raycast(o, d)
    n_light, n_brdf = counts
    mesh = asset.shade_env(o, d, t, face, bary, env, tables(), n_light=n_light, n_brdf=n_brdf, seed=SEED, dump=True)
    hit = face >= 0
    assert 100 < int(hit.sum()) < hit.numel() - 100
    gb = {"convergent_mask": hit, "ray_d": d}
    gb.update({k: mesh[k] for k in ("points", "normal", "diffuse_albedo", "specular_albedo", "specular_roughness")})
    out = relight(gb, SDFCallable(lambda x: torch.ones(x.shape[0], dtype=torch.float32, device=x.device)), env, n_light, n_brdf, dump=True)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(out["dump_dir"][hit]), bits(mesh["dump_dir"][hit]))
    assert torch.equal(bits(out["dump_denom"][hit]), bits(mesh["dump_denom"][hit]))
    seen = mesh["dump_vis"][hit].bool()
    print("%s: mesh-visible samples %d of %d, neural-visible %d" % (counts, int(seen.sum()), seen.numel(), int(out["dump_vis"][hit].sum())))
    assert 0 < int(seen.sum()) < seen.numel()
    assert bool(out["dump_vis"][hit].bool()[seen].all())   # nothing is occluded: every sample the mesh lets through counts here too
    assert torch.equal(bits(out["dump_contrib"][hit])[seen], bits(mesh["dump_contrib"][hit])[seen])
    assert (out["color"][~hit] == 0).all()


# ---- 5. relight_camera ---------------------------------------------------------------------------------------------------------------
def test_relight_camera_on_s0():
    from iron_amd import scenes
    from iron_amd.envmap import EnvMap
    from iron_amd.mesh_render import subpixel_uvs
    from iron_amd.neural_relight import _ggx_render_fn, relight_camera, relight_uv
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    net, nets, tr = net_on_device("S0"), material_nets(), RayTracer()
    K, W2C = scenes.fixture_camera_matrices(32, 32, 0.0)
    cam = Camera(32, 32, K.to(dev()), W2C.to(dev()))
    env = EnvMap(torch.ones((16, 32, 3), device=dev()))
    kw = dict(n_light=16, n_brdf=16, seed=3)
    ref = render_camera(cam, net, tr, nets, _ggx_render_fn(), handle_edges=False)
    stats = {}
    res = relight_camera(cam, net, tr, nets, env, stats=stats, **kw)
    assert set(res.keys()) == set(ref.keys())
    for k in ref:
        assert res[k].shape == ref[k].shape and res[k].dtype == ref[k].dtype, k
    for k in ("convergent_mask", "points", "normal", "diffuse_albedo", "specular_albedo", "specular_roughness", "depth", "distance"):
        assert torch.equal(res[k], ref[k]), k  # the G-buffer is render_camera's
    m = res["convergent_mask"]
    assert 100 < int(m.sum()) < 32 * 32 - 100
    # every counting sample is visible: S0 shadows nothing
    print("relight_camera S0 32 x 32: %d hits, %d shadow rays, %d occluded" % (int(m.sum()), stats["shadow_rays"], stats["occluded"]))
    assert stats["shadow_rays"] > 0 and stats["occluded"] == 0
    assert (res["color"][~m] == 0).all() and float(res["color"][m].min()) > 0 and torch.isfinite(res["color"]).all()
    assert torch.equal(res["color"], res["diffuse_color"] + res["specular_color"])
    # background=True changes the miss pixels of `color` and nothing else
    bg = relight_camera(cam, net, tr, nets, env, background=True, **kw)
    for k in res:
        if k != "color":
            assert torch.equal(res[k], bg[k]), k
    assert torch.equal(bg["color"][m], res["color"][m])
    assert torch.equal(bg["color"][~m], env.lookup(res["ray_d"][~m]))
    assert float(bg["color"][~m].min()) > 0
    # samples_per_axis = 2: the mean of the four sub-frames, sample k with seed + k
    ss = relight_camera(cam, net, tr, nets, env, samples_per_axis=2, **kw)
    frames = [relight_uv(cam, net, tr, nets, env, uv, n_light=16, n_brdf=16, seed=3 + k) for k, uv in enumerate(subpixel_uvs(cam, 2))]
    mean = (((frames[0]["color"] + frames[1]["color"]) + frames[2]["color"]) + frames[3]["color"]) / 4.0
    assert torch.equal(ss["color"].view(torch.int32), mean.view(torch.int32))
    assert set(ss.keys()) == set(ref.keys())
    for k in ref:
        assert ss[k].shape == ref[k].shape and ss[k].dtype == ref[k].dtype, k


# ---- 6. the command line -------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    from iron_amd import scenes
    from iron_amd.envmap import EnvMap
    from iron_amd.neural_relight import relight_camera
    from iron_amd.raytracer import Camera, RayTracer
    from iron_amd.relight import load_networks
    from iron_amd.render_asset import to8b_gamma
    nets = scenes.build_networks("S0")
    ckpt = os.path.join(tmp_path, "ckpt_1000.pth")
    torch.save({k: v.state_dict() for k, v in nets.items()}, ckpt)
    K, W2C = scenes.fixture_camera_matrices(16, 16, 0.0)
    cams = {"7.png": {"K": K.reshape(-1).tolist(), "W2C": W2C.reshape(-1).tolist(), "img_size": [16, 16]}}
    with open(os.path.join(tmp_path, "cam_dict_norm.json"), "w") as fp:
        json.dump(cams, fp)
    probe = EO.hot_map().float().numpy()
    np.save(os.path.join(tmp_path, "probe.npy"), probe)
    rdir = os.path.join(tmp_path, "relit")
    r = subprocess.run([sys.executable, "-m", "iron_amd.relight", "--ckpt", ckpt, "--cam_dict", os.path.join(tmp_path, "cam_dict_norm.json"),
                        "--envmap", os.path.join(tmp_path, "probe.npy"), "--out", rdir, "--n-light", "8", "--n-brdf", "8", "--seed", "3",
                        "--samples-per-axis", "2", "--background", "--shadow-eps", "0.002"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if os.path.exists(os.path.join(rdir, "image", "7.npy")):
        img = np.load(os.path.join(rdir, "image", "7.npy"))
    else:
        import imageio
        img = np.asarray(imageio.imread(os.path.join(rdir, "image", "7.exr")), dtype=np.float32)
    sdf_network, mats = load_networks(ckpt, dev())
    cam = Camera(16, 16, torch.tensor(cams["7.png"]["K"], dtype=torch.float32).reshape(4, 4).to(dev()),
                 torch.tensor(cams["7.png"]["W2C"], dtype=torch.float32).reshape(4, 4).to(dev()))
    api = relight_camera(cam, sdf_network, RayTracer(), mats, EnvMap(np.load(os.path.join(tmp_path, "probe.npy"))), n_light=8, n_brdf=8, seed=3,
                         samples_per_axis=2, background=True, shadow_eps=0.002)["color"].cpu().numpy()
    assert img.dtype == np.float32 and img.shape == (16, 16, 3) and np.array_equal(img.view(np.int32), api.view(np.int32))
    assert float(api.max()) > 0
    from PIL import Image
    png = np.asarray(Image.open(os.path.join(rdir, "image", "7.png")))
    assert np.array_equal(png[..., :3], to8b_gamma(api))
