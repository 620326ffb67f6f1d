"""High-precision side of the per-row tests of the fused hit shading (tests/test_shading_oracle.py on the CPU,
tests/test_gpu_hit_shading.py on the GPU): iron_shade_ggx / iron_shade_composite of iron_amd/csrc/shade.hip, i.e. hit list ->
get_all -> material networks -> co-located BRDF -> scatter.

Networks.  Three sets, every network generalise()d (tests/_nets.py): "ggx" (scene S1), "mat2_6" (S1 with 2- and 6-layer
albedo nets: launch_material's other branches) and "comp" (scene S2: the SDF net and the eight heads of R.COMP_SPECS).

Base rows.  7 strata x 130 rows (two full waves plus two lanes).  The points are N.sdf_inputs; per row the view direction is
built around the fp64 oracle normal n of that point: view = n cos(a) + t sin(a) with a random unit tangent t and a = 0, 2, 20,
60, 85, 89.9, 120 degrees by stratum, dist uniform in [1, 3], ray_o = fp32(x + dist view), ray_d = fp32(-view).  Uniformly
random directions leave most rows back-facing and the specular lobe below 1e-3; with the strata it reaches ~9 at 0 degrees
(n.v on the 0.99999 clamp), and the 120-degree stratum sits on the 1e-5 clamp.

Reference.  The chain R.sdf_get_all -> normalise -> R.get_materials / R.get_materials_comp -> R.ggx_colocated /
R.composite_forward, called part by part (R.render_fn_* store into fp32 maps), in fp64 and in fp32 on the same fp32 inputs.  The
fp64 runs hold the fp32 program's clamp bounds (_brdf_oracle.clamp_bounds).

Floors, from the reference alone, per key and stratum:
  F  stage-1 keys (normal, albedos, roughness, the composite's five scalars): max over rows of |chain32 - chain64| (row norm);
  B  radiance keys: max over entries of |BRDF32 - BRDF64|, both fed the fp64 chain's normal and materials rounded once to fp32
     (and the fp32 points / ray_o / ray_d): the price of the BRDF stage alone.

judge() applies the bounds both test files share:
  stage-1   |got_i - chain64_i| <= max(margin F[key, stratum], ROW_FACTOR TOL rms),  rms the key's rms fp64 row norm;
  radiance  |got_i - BRDF64(got's own normal and materials)_i| <= margin max(B[key, stratum], 2 ulp32(BRDF64_i)), rows whose
            fp64 table coordinate (dot^0.25 100, (alpha/4)^0.25 50) lies within STEP_MARGIN of an integer left out, their
            share capped at STEP_SHARE.
The CPU file runs it with margin 1 on the evaluation the floors were measured on (which meets it with equality) and with the GPU
file's margin 4 on the whole fp32 chain; the GPU file runs it on the device's rows with margin 4.

Nothing here touches the GPU."""
from __future__ import annotations

import functools
import math
from typing import Dict

import numpy as np
import torch

import _brdf_oracle as E
import _nets as N
from _neus_oracle import run_as, ulp32
from iron_amd import scenes
from iron_amd.fields import RenderingNetwork
from oracle import iron_ref as R

ANGLES_DEG = (0.0, 2.0, 20.0, 60.0, 85.0, 89.9, 120.0)
ROWS_PER_STRATUM = 130
N_BASE = len(ANGLES_DEG) * ROWS_PER_STRATUM      # 910
NETSETS = ("ggx", "mat2_6", "comp")

TOL = 1e-5          # tests/test_gpu_net_shapes.py: TOL_SDF (materials), TOL_GRAD (the normal), ROW_FACTOR
TOL_NORMAL = 2e-5
ROW_FACTOR = 10
STEP_MARGIN = 1e-4  # tests/test_gpu_envlight.py
STEP_SHARE = 5e-3

STAGE1 = {"ggx": ("normal", "diffuse_albedo", "specular_albedo", "specular_roughness"),
          "comp": ("normal", "diffuse_albedo", "specular_albedo", "specular_roughness", "metallic", "dielectric", "metallic_eta",
                   "metallic_k", "dielectric_eta")}
RADIANCE = {"ggx": ("color", "diffuse_color", "specular_color"),
            "comp": ("color", "diffuse_color", "specular_color", "metallic_rgb", "dielectric_rgb")}
_RES_KEY = {"color": "rgb", "diffuse_color": "diffuse_rgb", "specular_color": "specular_rgb", "metallic_rgb": "metallic_rgb",
            "dielectric_rgb": "dielectric_rgb"}


def kind_of(netset: str) -> str:
    return "comp" if netset == "comp" else "ggx"


def keys_of(netset: str) -> tuple:
    return RADIANCE[kind_of(netset)] + STAGE1[kind_of(netset)]


def _tables():
    from iron_amd.renderer_ggx import load_mts_tables
    return load_mts_tables()


def scene(variant):
    """S1 with every network generalise()d; "mat2_6": its diffuse / specular-albedo nets replaced by 2- and 6-layer nets."""
    nets = scenes.build_networks("S1")
    specs = dict(R.GGX_SPECS)
    if variant == "mat2_6":
        for key, depth in (("diffuse_albedo_network", 2), ("specular_albedo_network", 6)):
            kw = dict(N.RENDER_FAMILIES["idr_0_4" if key.startswith("diffuse") else "nvd_6"], n_layers=depth)
            torch.manual_seed(depth)
            nets[key] = RenderingNetwork(**kw)
            specs[key] = N.render_spec(kw)
    for i, key in enumerate(sorted(specs) + ["sdf_network"]):
        N.generalise(nets[key], 50 + i)
    mt, md = _tables()
    sc = R.Scene({k: v.detach().clone() for k, v in nets["sdf_network"].state_dict().items()}, R.SDFSpec(),
                 {k: ({n: v.detach().clone() for n, v in nets[k].state_dict().items()}, specs[k]) for k in specs}, float(nets["point_light_network"]()), mt, md)
    return nets, sc


def comp_scene():
    """Scene S2 (scenes.build_comp_networks) with the SDF net and the eight R.COMP_SPECS nets generalise()d."""
    nets = scenes.build_comp_networks()
    specs = dict(R.COMP_SPECS)
    for i, key in enumerate(sorted(specs) + ["sdf_network"]):
        N.generalise(nets[key], 80 + i)
    mt, md = _tables()
    sc = R.Scene({k: v.detach().clone() for k, v in nets["sdf_network"].state_dict().items()}, R.SDFSpec(),
                 {k: ({n: v.detach().clone() for n, v in nets[k].state_dict().items()}, specs[k]) for k in specs}, float(nets["point_light_network"]()), mt, md,
                 renderer="comp")
    return nets, sc


@functools.lru_cache(maxsize=None)
def networks(netset: str):
    """(modules on the CPU, R.Scene) of a network set; built once, never modified."""
    return comp_scene() if netset == "comp" else scene("s1" if netset == "ggx" else netset)


# ---- the chain, part by part ------------------------------------------------------------------------------------------------
def _stage1(sdf_sd, sdf_spec, nets, kind, is_metal, x):
    _, feat, g = R.sdf_get_all(sdf_sd, sdf_spec, x)
    n = g / (g.norm(dim=-1, keepdim=True) + 1e-10)
    m = R.get_materials(nets, x, n, feat, is_metal=is_metal) if kind == "ggx" else R.get_materials_comp(nets, x, n, feat)
    out = {k: v.detach() for k, v in m.items()}
    out["normal"] = n.detach()
    return out


def _brdf(light, mt, md, kind, x, ray_o, ray_d, s1):
    dist = (x - ray_o).norm(dim=-1, keepdim=True)
    fn = R.ggx_colocated if kind == "ggx" else R.composite_forward
    res = fn(light, dist, s1["normal"], -ray_d, s1, mt, md)
    return {k: res[_RES_KEY[k]] for k in RADIANCE[kind]}


def stage1(netset: str, is_metal: bool, x: torch.Tensor, dtype) -> Dict[str, torch.Tensor]:
    """Normal and materials of the points `x` (fp32) through the oracle in `dtype`."""
    _, sc = networks(netset)
    with E.clamp_bounds("fp32" if dtype == torch.float64 else None):
        return run_as(dtype, _stage1, sc.sdf_sd, sc.sdf_spec, sc.nets, kind_of(netset), is_metal, x)


def brdf(netset: str, rows: Dict[str, torch.Tensor], s1: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    """The radiance keys from the fp32 points / ray_o / ray_d of `rows` and the normal and materials `s1`, in `dtype`."""
    _, sc = networks(netset)
    with E.clamp_bounds("fp32" if dtype == torch.float64 else None):
        return run_as(dtype, _brdf, sc.light, sc.mts_trans, sc.mts_diff_trans, kind_of(netset), rows["points"], rows["ray_o"], rows["ray_d"],
                      {k: v for k, v in s1.items()})


# ---- base rows --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_rows(netset: str) -> Dict[str, torch.Tensor]:
    """points, ray_o, ray_d [910, 3] fp32 and stratum [910] (row // 130) of a network set (the views hang on its SDF's normals)."""
    gen = torch.Generator().manual_seed(4242)
    x = N.sdf_inputs(N_BASE, 4243).float().contiguous()
    n = stage1(netset, False, x, torch.float64)["normal"]
    t = torch.randn(N_BASE, 3, generator=gen, dtype=torch.float64)
    t = torch.nn.functional.normalize(t - (t * n).sum(-1, keepdim=True) * n, dim=-1)
    stratum = torch.arange(N_BASE) // ROWS_PER_STRATUM
    a = torch.tensor([math.radians(d) for d in ANGLES_DEG], dtype=torch.float64)[stratum][:, None]
    view = n * torch.cos(a) + t * torch.sin(a)
    dist = 1.0 + 2.0 * torch.rand(N_BASE, 1, generator=gen, dtype=torch.float64)
    return {"points": x, "ray_o": (x.double() + dist * view).float().contiguous(), "ray_d": (-view).float().contiguous(), "stratum": stratum}


def raw_dot(rows, normal) -> torch.Tensor:
    """fp64 n.v [n, 1] of the rows' view directions with `normal`."""
    return (-rows["ray_d"].double() * normal.double()).sum(-1, keepdim=True)


def step_rows(netset: str, rows, s1) -> torch.Tensor:
    """[n] bool: rows whose fp64 table coordinate lies within STEP_MARGIN of an integer (their diffuse lobe may take either bin)."""
    c = raw_dot(rows, s1["normal"]).clamp(E.COS_LO, E.COS_HI)
    a = s1["specular_roughness"].double().reshape(-1, 1)
    if kind_of(netset) == "comp":
        a = a.clamp(min=E.BOUNDS_COMPOSITE["rough"][0])
    a = a.clamp(min=E.BOUNDS_GGX["rough"][0])
    near = torch.zeros(c.shape[0], dtype=torch.bool)
    for w in (c ** 0.25 * 100.0, (a / 4.0) ** 0.25 * 50.0):
        near |= ((w - torch.round(w)).abs() < STEP_MARGIN)[:, 0]
    return near


def _per_stratum(v: torch.Tensor, stratum: torch.Tensor) -> torch.Tensor:
    return torch.stack([v[stratum == s].max() for s in range(len(ANGLES_DEG))])


@functools.lru_cache(maxsize=None)
def reference(netset: str, is_metal: bool = False):
    """Everything both test files compare against, for the 910 base rows of a network set."""
    rows = base_rows(netset)
    kind = kind_of(netset)
    st = rows["stratum"]
    c64, c32 = stage1(netset, is_metal, rows["points"], torch.float64), stage1(netset, is_metal, rows["points"], torch.float32)
    once = {k: v.float() for k, v in c64.items()}
    b64, b32 = brdf(netset, rows, once, torch.float64), brdf(netset, rows, once, torch.float32)
    F = {k: _per_stratum((c32[k].double() - c64[k]).norm(dim=-1), st) for k in STAGE1[kind]}
    B = {k: _per_stratum((b32[k].double() - b64[k]).abs().amax(dim=-1), st) for k in RADIANCE[kind]}
    rms = {k: float(c64[k].pow(2).sum(dim=-1).mean().sqrt()) for k in STAGE1[kind]}
    full32 = dict(c32)
    full32.update(brdf(netset, rows, c32, torch.float32))
    return {"rows": rows, "chain64": c64, "chain32": full32, "rad64": brdf(netset, rows, c64, torch.float64), "F": F, "B": B, "rms": rms,
            "step": step_rows(netset, rows, c64)}


def _as2d(v, n) -> torch.Tensor:
    v = v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
    return v.reshape(n, -1)


def judge(netset: str, is_metal: bool, got: Dict[str, torch.Tensor], margin: float, tag: str = "", strict: bool = True) -> Dict[str, dict]:
    """Hold the 910 base rows `got` (every key of keys_of(netset), fp32, base order) to the bounds of the module docstring.
    Returns {key: {"ratio": worst err / floor, "term": which term of the bound was the larger one at the worst row, ...}};
    raises AssertionError naming key, row and stratum of the worst offender of every failing key (strict=False: returns them under
    "_failures" instead, so that a caller can print the report first)."""
    ref = reference(netset, is_metal)
    kind, rows, st = kind_of(netset), ref["rows"], ref["rows"]["stratum"]
    got = {k: _as2d(got[k], N_BASE) for k in keys_of(netset)}
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (tag, k, "non-finite")
    report, failures = {}, []
    for k in STAGE1[kind]:
        err = (got[k].double() - ref["chain64"][k]).norm(dim=-1)
        floor = ref["F"][k][st]
        yard = ROW_FACTOR * (TOL_NORMAL if k == "normal" else TOL) * ref["rms"][k]
        bound = torch.clamp(margin * floor, min=yard)
        i = int((err / bound).argmax())
        report[k] = {"ratio": float((err / floor.clamp(min=1e-300)).max()), "worst": float((err / bound).max()), "row": i,
                     "term": "F" if margin * float(floor[i]) >= yard else "rms"}
        if float(err[i]) > float(bound[i]):
            failures.append("%s row %d (stratum %d): |err| %.3e > bound %.3e (F %.3e, rms term %.3e)" % (k, i, int(st[i]), err[i], bound[i], floor[i], yard))
    s1 = {k: got[k] for k in STAGE1[kind]}
    f64 = brdf(netset, rows, s1, torch.float64)
    step = step_rows(netset, rows, s1)
    share = float(step.double().mean())
    if share > STEP_SHARE:
        failures.append("table-step rows: share %.2e > %.2e" % (share, STEP_SHARE))
    for k in RADIANCE[kind]:
        err = (got[k].double() - f64[k]).abs()
        floor = torch.maximum(ref["B"][k][st][:, None].expand_as(err), 2.0 * ulp32(f64[k]))
        r = (err / (margin * floor)).masked_fill(step[:, None], 0.0)
        i = int(r.amax(dim=-1).argmax())
        report[k] = {"ratio": float((err / floor).masked_fill(step[:, None], 0.0).max()), "worst": float(r.max()), "row": i,
                     "term": "B" if float(ref["B"][k][st[i]]) >= float(2.0 * ulp32(f64[k][i]).max()) else "ulp"}
        if float(r.max()) > 1.0:
            c = int(r[i].argmax())
            failures.append("%s row %d ch %d (stratum %d): |err| %.3e > %g x floor %.3e (value %.6e)" % (k, i, c, int(st[i]), err[i, c], margin, floor[i, c], f64[k][i, c]))
    report["_step_share"], report["_failures"] = share, failures
    if not strict:
        return report
    assert not failures, "%s: %s" % (tag, "; ".join(failures))
    return report


def describe(report: Dict[str, dict]) -> str:
    """Per key: worst error over its floor (F or max(B, 2 ulp)), the share of the bound it used, and which term of the bound was
    the larger one at the worst row."""
    return ", ".join("%s %.2f floor / %.2f bound [%s] (row %d)" % (k, v["ratio"], v["worst"], v["term"], v["row"])
                     for k, v in report.items() if not k.startswith("_"))
