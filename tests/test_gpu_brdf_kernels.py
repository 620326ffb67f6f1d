"""The co-located BRDF heads (csrc/ggx_core.h with float in pointwise.hip, with Dual<N> in k_ggx_back / k_composite_back /
k_coloc_head_back of train.hip, and the wrappers of iron_amd/autograd.py) against oracle/iron_ref.py evaluated in fp64
(tests/_brdf_oracle.py), per ROW and per entry, forward and backward: 130 rows per stratum (two full waves plus two lanes) and one
n = 1 case; interior, grazing, near-normal, glossy and very rough rows, and every clamp with rows dead, live and exactly on the
fp32 bound.

Tolerance: |gpu_i - fp64_i| <= 4 max(1, r_cpu) y_i, y_i the yardstick of that entry (2 ulp32 + the effect of one rounding of each
consumed scalar + the cancellation term, from the fp64 side alone) and r_cpu what torch's fp32 CPU evaluation of the oracle needs
of it, measured here.  The 4 is the project's margin over the honest-fp32 floor (test_gpu_neus_kernels.py): device sqrtf / hypotf /
powf / division against the CPU's, and the summation order of the dual-number derivative against autograd's.  Where the reference's
gradient is exactly 0 the kernel's is exactly 0.  Lines starting with "brdf-k" carry the measured figures (DESIGN.md keeps the
table); tests/test_brdf_oracle.py checks the yardstick, the flags and the strata on the CPU."""
import pytest
import torch

import _brdf_oracle as B

pytestmark = pytest.mark.gpu

MARGIN = 4.0


@pytest.fixture(scope="module")
def heads():
    from iron_amd import renderer_ggx as G
    return {"ggx": G.GGXColocatedRenderer(use_cuda=True), "composite": G.CompositeRenderer(use_cuda=True),
            "smooth_dielectric": G.SmoothDielectricRenderer(), "thin_dielectric": G.ThinDielectricRenderer(),
            "smooth_conductor": G.SmoothConductorCoLocRenderer(), "rough_conductor": G.RoughConductorCoLocRenderer()}


def _call(heads, head, v):
    """The head on a dict of CUDA tensors (the names of the stratum dicts; light a tensor or a float)."""
    if head == "ggx":
        return heads["ggx"](v["light"], v["distance"], v["normal"], v["viewdir"],
                            {"diffuse_albedo": v["kd"], "specular_albedo": v["ks"], "specular_roughness": v["rough"]})
    if B.is_composite(head):
        p = {"diffuse_albedo": v["kd"], "specular_albedo": v["ks"], "specular_roughness": v["rough"], "metallic_eta": v["m_eta"],
             "metallic_k": v["m_k"], "dielectric_eta": v["d_eta"], "metallic": v["rough"].detach(), "dielectric": v["rough"].detach(),
             "env_light": v["env_light"]}
        return heads["composite"](v["light"], v["distance"], v["normal"], v["viewdir"], p, use_env_light=head == "composite_env")
    return heads[head](v["light"], v["distance"], v["normal"], v["viewdir"], v["kd"], v["ks"], v["rough"] if head == "rough_conductor" else None)


LEAVES = ("light", "distance", "normal", "viewdir", "kd", "ks", "rough", "m_eta", "m_k", "d_eta", "env_light")


def _run(heads, head, inp, ups, light=None, shape=None):
    """Forward and backward on the GPU: (outputs, gradients of every leaf, None where autograd returned none), on the CPU.
    `inp` / `ups` are CPU fp32 rows; `shape` gives every tensor that leading shape; `light` overrides the 0-dim tensor."""
    dev = torch.device("cuda", 0)
    v = {}
    for k in B.FIELDS:
        x = inp[k].to(dev)
        v[k] = (x.reshape(tuple(shape) + (x.shape[-1],)) if shape else x).requires_grad_(True)
    v["light"] = torch.tensor(B.LIGHT, device=dev, requires_grad=True) if light is None else light
    out = _call(heads, head, v)
    loss = 0.0
    for k, u in ups.items():
        if u is not None:
            loss = loss + (out[k].reshape(u.shape) * u.to(dev)).sum()
    leaves = [k for k in LEAVES if torch.is_tensor(v[k])]
    g = torch.autograd.grad(loss, [v[k] for k in leaves], allow_unused=True)
    torch.cuda.synchronize()
    return ({k: o.detach().cpu() for k, o in out.items()}, {k: (None if x is None else x.detach().cpu()) for k, x in zip(leaves, g)})


def _rows(t, sl):
    return None if t is None else t[sl]


def _check(head, ref, cfg, sl, out, g, worst, tag, forward=True, skip=(), light=True):
    """Every entry of one (stratum, configuration) against fp64; returns nothing, raises with the figures."""
    r = ref["cfg"][cfg]
    bound = ref["flags"]["bound"][sl]
    keys = [k for k in B.entry_keys(head, ref, cfg) if (forward or k.startswith("d:")) and k not in skip]
    for key in keys:
        kind, name = key.split(":")
        got = out[name] if kind == "out" else g[name]
        assert got is not None, (tag, key)
        want = (r["out64"] if kind == "out" else r["g64"])[name][sl]
        got = got.reshape(want.shape)
        rc = B.r_cpu(head, ref, cfg, key, sl)
        v = B.ratio(got, want, r["y"][key][sl], B.skip_mask(head, ref, cfg, key)[sl])
        worst.setdefault(key, [0.0, 0.0])
        worst[key] = [max(worst[key][0], v), max(worst[key][1], rc)]
        assert v <= MARGIN * max(1.0, rc), (tag, cfg, key, "ratio to y %.2f" % v, "r_cpu %.2f" % rc)
        if kind == "d":   # dead entries: exactly zero (rows flagged on a bound may fall on either side)
            dead = B.dead(r["g32"][name][sl], r["g64"][name][sl]) & ~bound[:, None]
            assert bool((got[dead] == 0).all()), (tag, cfg, key, "dead entries with a gradient: %d" % int((got[dead] != 0).sum()))
    if head == "composite_env":   # the light and the distance take no part
        assert g.get("light") is None or float(g["light"].abs().max()) == 0.0
        assert g["distance"] is None or float(g["distance"].abs().max()) == 0.0
        return
    if head == "composite":
        assert g["env_light"] is None or float(g["env_light"].abs().max()) == 0.0
    if not light:
        return
    rc = B.r_cpu(head, ref, cfg, "d:light", sl)
    tol = B.light_tolerance(r["y"]["d:light"][sl], r["t64"][sl], rc)
    err = abs(float(g["light"]) - float(r["t64"][sl].sum()))
    worst.setdefault("d:light", [0.0, 0.0])
    worst["d:light"] = [max(worst["d:light"][0], err / tol), max(worst["d:light"][1], rc)]
    assert err <= tol, (tag, cfg, "d:light", err, tol)


@pytest.mark.parametrize("head", B.HEADS)
def test_head_forward_and_backward_per_row(heads, head):
    """Every stratum of the head (n = 130, and n = 1) under every upstream configuration: each output alone with a positive
    upstream and None for the others (the kernels' null-pointer paths; an output that takes no part in the loss), and all together
    random-signed.  d_light: against the fp64 sum within sum_i 4 max(1, r_cpu) y_i + n 2^-24 sum_i |t_i|; under use_env_light
    exactly 0 (or not returned)."""
    ref = B.reference(head)
    inp = ref["inputs"]
    for s, sl in ref["slices"].items():
        worst = {}
        rows = {k: inp[k][sl] for k in B.FIELDS}
        for i, (cfg, r) in enumerate(ref["cfg"].items()):
            ups = {k: _rows(u, sl) for k, u in r["ups"].items()}
            out, g = _run(heads, head, rows, ups)
            if B.is_composite(head):
                assert torch.equal(out["diffuse_rgb"], out["rgb"])
            _check(head, ref, cfg, sl, out, g, worst, (head, s), forward=i == 0 or cfg == "mixed")
        flagged = int((ref["flags"]["table"] | ref["flags"]["bound"])[sl].sum())
        print("brdf-k %s %s n=%d flagged=%d ratio-to-y(r_cpu):" % (head, s, sl.stop - sl.start, flagged),
              " ".join("%s=%.2f(%.2f)" % (k, a, b) for k, (a, b) in worst.items()))
        assert flagged <= 0.01 * (sl.stop - sl.start)


@pytest.mark.parametrize("s", B.SMITH_STRATA)
def test_standalone_smith_g1(s):
    from iron_amd.renderer_ggx import smithG1
    ref, lo, y = B.smith_reference(s)
    c, a = B.smith_inputs(s)
    with torch.no_grad():
        got = smithG1(c.cuda(), a.cuda()).cpu()
    rc = float(((lo.double() - ref).abs() / y).max())
    v = float(((got.double() - ref).abs() / y).max())
    print("brdf-k smith_g1 %s ratio-to-y %.2f r_cpu %.2f" % (s, v, rc))
    assert v <= MARGIN * max(1.0, rc)


# ---- the wrapper layer of iron_amd/autograd.py --------------------------------------------------------------------------------
WRAPPED = ("ggx", "composite", "composite_env", "rough_conductor", "smooth_dielectric")   # the last one: the wrapper's alpha = None branch


def _interior(head):
    ref = B.reference(head)
    sl = ref["slices"]["interior"]
    r = ref["cfg"]["mixed"]
    return ref, sl, {k: ref["inputs"][k][sl] for k in B.FIELDS}, {k: _rows(u, sl) for k, u in r["ups"].items()}


@pytest.mark.parametrize("head", WRAPPED)
def test_wrapper_leading_shape(heads, head):
    """Inputs of shape [2, 65, .]: the same rows, the same fp64 numbers, outputs and gradients in the inputs' shape."""
    ref, sl, rows, ups = _interior(head)
    out, g = _run(heads, head, rows, ups, shape=(2, 65))
    assert all(o.shape[:2] == (2, 65) for o in out.values())
    assert all(x is None or k == "light" or x.shape[:2] == (2, 65) for k, x in g.items())
    _check(head, ref, "mixed", sl, out, g, {}, (head, "leading shape"))


@pytest.mark.parametrize("head", WRAPPED)
def test_wrapper_light_as_python_float(heads, head):
    """light given as a float: no gradient is returned for it, everything else is the same numbers."""
    ref, sl, rows, ups = _interior(head)
    out, g = _run(heads, head, rows, ups, light=B.LIGHT)
    assert "light" not in g
    _check(head, ref, "mixed", sl, out, g, {}, (head, "float light"), light=False)


@pytest.mark.parametrize("head", WRAPPED)
def test_wrapper_albedo_with_one_channel(heads, head):
    """kd and ks given as [n, 1]: broadcast over the channels, the gradient summed over them.  The reference is the fp64 run on
    the albedo repeated over the channels; the sum of three entries gets the sum of their tolerances."""
    _, sl, rows, _ = _interior(head)
    wide = dict(rows)
    wide["kd"], wide["ks"] = rows["kd"][:, :1].expand(-1, 3).contiguous(), rows["ks"][:, :1].expand(-1, 3).contiguous()
    ref = B.reference_for(head, wide)
    r = ref["cfg"]["mixed"]
    narrow = dict(rows)
    narrow["kd"], narrow["ks"] = rows["kd"][:, :1].contiguous(), rows["ks"][:, :1].contiguous()
    out, g = _run(heads, head, narrow, r["ups"])
    al = slice(0, sl.stop - sl.start)
    _check(head, ref, "mixed", al, out, g, {}, (head, "[n, 1] albedo"), skip=("d:kd", "d:ks"))
    for k in ("kd", "ks"):
        assert g[k].shape == narrow[k].shape
        rc = B.r_cpu(head, ref, "mixed", "d:" + k, al)
        tol = (MARGIN * max(1.0, rc) * r["y"]["d:" + k]).sum(-1, keepdim=True)
        err = (g[k].double() - r["g64"][k].sum(-1, keepdim=True)).abs()
        keep = ~(ref["flags"]["bound"] | ref["flags"]["table"])[:, None]
        assert bool((err <= tol)[keep].all()), (head, k, float((err / tol)[keep].max()))
