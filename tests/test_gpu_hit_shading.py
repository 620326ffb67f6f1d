"""The fused hit shading (iron_shade_ggx / iron_shade_composite, iron_amd/csrc/shade.hip, reached through the render functions'
iron_fused_ggx), row by row: hit list -> get_all -> material networks -> co-located BRDF -> scatter.

a  the 910 base rows of tests/_shading_oracle.py, all hits, every row of every output against the fp64 oracle with the bounds of
   _shading_oracle.judge (margin 4 over the honest-fp32 floors, as tests/test_gpu_brdf_kernels.py and test_gpu_neus_kernels.py):
   three network sets, is_metal 0 / 1, the default and the exact core.
b  the same rows embedded into masks of other sizes (hit counts 0, 1, around the 32-hit tile and the 128-hit group, the last ray
   alone, a second grid-stride trip, a permutation, the same call twice): every hit row returns the bits it returned in (a)
   wherever it lands in the hit list, every non-hit entry of every output is +0, the non-hit rows of the inputs hold NaN, the
   shared workspace is filled with 0xFF before every call (what an earlier call left reads as NaN) and the numeric status of
   every network stays clean.
c  the interface: mask dtypes, [H, W, ...] and non-contiguous inputs, NULL outputs, workspace size / alignment / reuse.

Measured worst ratios: DESIGN.md section 24."""
import ctypes as C

import pytest
import torch

from iron_amd import _lib
from iron_amd.renderer_ggx import CompositeRenderer, GGXColocatedRenderer
from iron_amd.rendering_func import make_render_fn, make_render_fn_comp

import _shading_oracle as S

pytestmark = pytest.mark.gpu

MARGIN = 4.0
DEV = torch.device("cuda", 0)
CASES = [("ggx", False), ("ggx", True), ("mat2_6", False), ("comp", False)]
CORES = ("default", "exact")
_GGX_KEYS = ("color", "diffuse_color", "specular_color", "diffuse_albedo", "specular_albedo", "specular_roughness", "normal")

_cache = {}


def _nets(netset, exact):
    """The network set on the device, one copy per core (a handle pinned to the exact core stays pinned)."""
    if ("nets", netset, exact) not in _cache:
        import copy
        nets = {k: copy.deepcopy(m).to(DEV) for k, m in S.networks(netset)[0].items()}
        if exact:
            for m in nets.values():
                if hasattr(m, "force_exact"):
                    m.force_exact(True)
        _cache[("nets", netset, exact)] = nets
    return _cache[("nets", netset, exact)]


def _fn(netset, is_metal):
    if ("fn", netset, is_metal) not in _cache:
        _cache[("fn", netset, is_metal)] = (make_render_fn_comp(CompositeRenderer(use_cuda=True)) if netset == "comp"
                                            else make_render_fn(GGXColocatedRenderer(use_cuda=True), is_metal=is_metal))
    return _cache[("fn", netset, is_metal)]


def _embed(netset, n, pos, rows):
    """`results` of n rays: base row rows[k] at ray pos[k] with the mask set, NaN in every other row of points / ray_o / ray_d."""
    base = S.base_rows(netset)
    pos, rows = torch.as_tensor(pos, dtype=torch.long), torch.as_tensor(rows, dtype=torch.long)
    res = {}
    for k in ("points", "ray_o", "ray_d"):
        v = torch.full((n, 3), float("nan"))
        v[pos] = base[k][rows]
        res[k] = v.to(DEV)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[pos] = True
    res["convergent_mask"] = mask.to(DEV)
    return res


def _run(netset, is_metal, exact, results):
    nets = _nets(netset, exact)
    stale = _lib.current_workspace(DEV, "shade")
    if stale is not None:   # what an earlier call left in the shared workspace reads as NaN (and as a hit count of -1)
        stale.fill_(0xFF)
    out = _fn(netset, is_metal).iron_fused_ggx(results, nets["sdf_network"], nets)
    torch.cuda.synchronize()
    assert set(out) == set(S.keys_of(netset))
    for k, m in nets.items():
        if hasattr(m, "numeric_status"):
            assert m.numeric_status() == {"overflow_seen": False, "exact_core": exact, "pending": False}, (k, m.numeric_status())
    return {k: v.cpu() for k, v in out.items()}


def _base(netset, is_metal, exact):
    """(a)'s device rows: the 910 base rows in base order, all hits.  Computed once per case and never modified."""
    key = ("base", netset, is_metal, exact)
    if key not in _cache:
        _cache[key] = _run(netset, is_metal, exact, _embed(netset, S.N_BASE, range(S.N_BASE), range(S.N_BASE)))
    return _cache[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- a: per row against fp64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("netset,is_metal", CASES)
@torch.no_grad()
def test_base_rows_against_fp64(netset, is_metal, core):
    got = _base(netset, is_metal, core == "exact")
    n = S.N_BASE
    for k, v in got.items():
        assert v.shape[0] == n and v.numel() in (n, 3 * n), (k, v.shape)
    rep = S.judge(netset, is_metal, got, MARGIN, strict=False)
    print("hit shading %s is_metal=%d %-7s: %s" % (netset, is_metal, core, S.describe(rep)))   # the measured figures, also when a row fails
    assert not rep["_failures"], (netset, is_metal, core, rep["_failures"])
    ks = got["specular_albedo"]
    if netset == "comp":
        assert _same_bits(got["diffuse_color"], got["color"])   # the composite returns one tensor under both keys
    elif is_metal:
        assert float((ks.max(dim=-1).values - ks.min(dim=-1).values).median()) > 1e-3   # per channel (and judged against the per-channel oracle)
    else:
        assert _same_bits(ks[:, 0], ks[:, 1]) and _same_bits(ks[:, 1], ks[:, 2])     # the channel mean, broadcast


# ---- b: hit-list edges ------------------------------------------------------------------------------------------------------------
def _edge_cases():
    pick = lambda c: ((torch.arange(c) * 27) % S.N_BASE).tolist()   # 27 is coprime to 910: distinct rows across all strata
    cases = {"n1_hit": (1, [0]), "n1_miss": (1, []), "n33_all": (33, list(range(33))), "n4099_ends": (4099, [0, 4098]),
             "n70001_last": (70001, [70000]), "n70001_none": (70001, [])}
    for c in (31, 32, 33, 127, 128, 129):
        cases["alternate_%d" % c] = (2 * c + 1, list(range(1, 2 * c, 2)))
    n = 2048 * 256 + 77   # past one trip of k_compact's and the shade kernels' 2048 x 256 grid
    cases["second_trip"] = (n, list(range(0, n, 1009)) + [n - 1])
    out = {name: (n, pos, pick(len(pos))) for name, (n, pos) in cases.items()}
    out["permutation"] = (S.N_BASE, list(range(S.N_BASE)), torch.randperm(S.N_BASE, generator=torch.Generator().manual_seed(9)).tolist())
    out["twice"] = (S.N_BASE, list(range(S.N_BASE)), list(range(S.N_BASE)))
    return out


EDGES = _edge_cases()


def _check_embedded(tag, out, base, n, pos, rows):
    """Hit rows carry (a)'s bits, every other entry is +0."""
    pos, rows = torch.as_tensor(pos, dtype=torch.long), torch.as_tensor(rows, dtype=torch.long)
    bad = []
    for k, v in out.items():
        v, b = v.reshape(n, -1), base[k].reshape(S.N_BASE, -1)
        want = torch.zeros_like(v)
        want[pos] = b[rows]
        diff = (_bits(v) != _bits(want)).any(dim=-1).nonzero()[:, 0]
        if diff.numel():
            r = int(diff[0])
            bad.append("%s: %d rows differ, first ray %d (%s): got %s want %s" % (k, diff.numel(), r, "hit" if bool((pos == r).any()) else "non-hit",
                                                                              v[r].tolist(), want[r].tolist()))
    assert not bad, "%s: %s" % (tag, "; ".join(bad))


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("netset,is_metal", CASES)
@torch.no_grad()
def test_hit_list_edges_bit_for_bit(netset, is_metal, core, edge):
    exact = core == "exact"
    base = _base(netset, is_metal, exact)
    n, pos, rows = EDGES[edge]
    res = _embed(netset, n, pos, rows)
    assert int(torch.isnan(res["points"]).all(dim=-1).sum()) == n - len(pos)
    out = _run(netset, is_metal, exact, res)
    _check_embedded("%s is_metal=%s %s %s" % (netset, is_metal, core, edge), out, base, n, pos, rows)


@pytest.mark.parametrize("netset", ["ggx", "comp"])
@torch.no_grad()
def test_no_rays(netset):
    res = {k: torch.empty((0, 3), device=DEV) for k in ("points", "ray_o", "ray_d")}
    res["convergent_mask"] = torch.empty((0,), dtype=torch.bool, device=DEV)
    out = _run(netset, False, False, res)
    for k, v in out.items():
        assert v.numel() == 0, k


# ---- c: interface -------------------------------------------------------------------------------------------------------------------
def _all_same(tag, a, b):
    for k in a:
        assert _same_bits(a[k], b[k]), (tag, k)


@pytest.mark.parametrize("netset", ["ggx", "comp"])
@torch.no_grad()
def test_mask_dtypes_and_layouts(netset):
    n, pos, rows = EDGES["alternate_32"]          # 65 rays = 5 x 13
    res = _embed(netset, n, pos, rows)
    flat = _run(netset, False, False, res)
    _check_embedded(netset + " flat", flat, _base(netset, False, False), n, pos, rows)
    for value in (1, 2, 255):
        alt = dict(res, convergent_mask=res["convergent_mask"].to(torch.uint8) * value)
        _all_same("uint8 mask holding %d" % value, flat, _run(netset, False, False, alt))
    image = {k: v.reshape(5, 13, *v.shape[1:]) for k, v in res.items()}
    _all_same("[H, W, ...]", flat, _run(netset, False, False, image))
    wide = {}
    for k in ("points", "ray_o", "ray_d"):       # columns 1..3 of every second row of a [2 n, 5] tensor
        big = torch.full((2 * n, 5), 7.0, device=DEV)
        big[::2, 1:4] = res[k]
        wide[k] = big[::2, 1:4]
        assert not wide[k].is_contiguous()
    big = torch.ones(3 * n, dtype=torch.bool, device=DEV)
    big[::3] = res["convergent_mask"]
    wide["convergent_mask"] = big[::3]
    _all_same("non-contiguous slices", flat, _run(netset, False, False, wide))


def _c_entry(netset, res, keys, ws=None, ws_bytes=None, ws_ptr=None):
    """iron_shade_ggx / iron_shade_composite called directly: outputs for `keys` only (NULL otherwise), the given workspace.
    Returns (status, {key: tensor})."""
    lib = _lib.load()
    nets = _nets(netset, False)
    fn = _fn(netset, False)
    n = res["points"].shape[0]
    comp = netset == "comp"
    all_keys = _lib.COMP_OUT_FIELDS if comp else _GGX_KEYS
    wide = (lambda k: k in fn._VEC) if comp else (lambda k: k != "specular_roughness")
    bufs = {k: torch.full((n, 3) if wide(k) else (n, 1), 5.0, device=DEV) for k in keys}
    so = _lib.iron_shade_comp_out() if comp else _lib.iron_shade_out()
    for k in all_keys:
        setattr(so, k, bufs[k].data_ptr() if k in bufs else None)
    ns = _lib.iron_shade_comp_nets() if comp else _lib.iron_shade_nets()
    keep = [nets["sdf_network"].hip_net()]
    ns.sdf = keep[0].handle
    for k in [f for f, _ in ns._fields_ if f != "sdf"]:
        keep.append(nets[k + "_network"].hip_net())
        setattr(ns, k, keep[-1].handle)
    t1, t2 = fn.renderer._tables_on(DEV)
    need = (lib.iron_shade_composite_workspace_bytes if comp else lib.iron_shade_workspace_bytes)(n)
    if ws is None:
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ws_bytes = need if ws_bytes is None else ws_bytes
    ws_ptr = ws.data_ptr() if ws_ptr is None else ws_ptr
    light = float(nets["point_light_network"]().detach())
    conv = res["convergent_mask"].to(torch.uint8)
    args = (t1.data_ptr(), t2.data_ptr(), res["ray_o"].data_ptr(), res["ray_d"].data_ptr(), res["points"].data_ptr(), conv.data_ptr(), n,
            C.byref(so), ws_ptr, ws_bytes, _lib.stream_ptr(DEV))
    rc = lib.iron_shade_composite(C.byref(ns), light, *args) if comp else lib.iron_shade_ggx(C.byref(ns), light, 0, *args)
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in bufs.items()}


@pytest.mark.parametrize("netset", ["ggx", "comp"])
@torch.no_grad()
def test_null_outputs(netset):
    n, pos, rows = EDGES["alternate_33"]
    res = _embed(netset, n, pos, rows)
    base = _base(netset, False, False)
    for only in ("color", "normal"):
        rc, out = _c_entry(netset, res, (only,))
        assert rc == 0, rc
        _check_embedded("%s only %s" % (netset, only), out, base, n, pos, rows)


@pytest.mark.parametrize("netset", ["ggx", "comp"])
@torch.no_grad()
def test_workspace_size_alignment_and_reuse(netset):
    lib = _lib.load()
    base = _base(netset, False, False)
    keys = S.keys_of(netset)
    n, pos, rows = EDGES["n33_all"]
    res = _embed(netset, n, pos, rows)
    need = (lib.iron_shade_composite_workspace_bytes if netset == "comp" else lib.iron_shade_workspace_bytes)(n)
    # exactly the advertised size, with a 4 KiB tail behind it that must survive
    buf = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
    buf[need:] = 0xA5
    rc, out = _c_entry(netset, res, keys, ws=buf, ws_bytes=need)
    assert rc == 0, rc
    _check_embedded(netset + " exact workspace", out, base, n, pos, rows)
    assert bool((buf[need:] == 0xA5).all()), "the call wrote past iron_shade*_workspace_bytes(n)"
    rc, _ = _c_entry(netset, res, keys, ws=buf, ws_bytes=need - 1)
    assert rc == -5, rc     # IRON_ERR_WORKSPACE
    rc, _ = _c_entry(netset, res, keys, ws=buf, ws_bytes=need, ws_ptr=buf.data_ptr() + 4)
    assert rc == -1, rc     # IRON_ERR_BAD_ARG: off 16-byte alignment
    # a workspace that the 524 365-ray case has used, then the 33-ray case: nothing stale may be read
    nb, posb, rowsb = EDGES["second_trip"]
    resb = _embed(netset, nb, posb, rowsb)
    needb = (lib.iron_shade_composite_workspace_bytes if netset == "comp" else lib.iron_shade_workspace_bytes)(nb)
    ws = torch.zeros(needb, dtype=torch.uint8, device=DEV)
    rc, outb = _c_entry(netset, resb, keys, ws=ws)
    assert rc == 0, rc
    _check_embedded(netset + " second_trip (C entry)", outb, base, nb, posb, rowsb)
    rc, again = _c_entry(netset, res, keys, ws=ws, ws_bytes=need)
    assert rc == 0, rc
    _all_same(netset + " reused workspace", out, again)
