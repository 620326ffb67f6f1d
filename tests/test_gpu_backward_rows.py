"""GPU: the three layer-wise backward entries of libiron_train.so (iron_sdf_backward, iron_render_backward, iron_nerf_backward), row
by row against the fp64 oracle (tests/_backward_oracle.py).

The whole-batch tests (test_gpu_train.py, test_gpu_net_shapes.py) compare one rel-L2 per parameter tensor over hundreds or
thousands of points, where one wrong point is diluted by 1 / sqrt(n).  Here the batches are EMBEDDED: the upstream gradient is exactly
zero except on at most 8 live rows placed at the edges of the kernels' row blocks (32 points when value and tangent rows are paired,
64 rows otherwise), at the 256-row gate between the split kernel and the row kernel, and at the chunk boundaries; the oracle is
evaluated on the live rows alone.  The entries are called through ctypes with a layer table, as tests/test_gpu_gemm.py drives
iron_train_gemm: they need no forward handle, so hidden widths iron_net_create does not serve ("alt": fused and unfused layers in
turn) and NULL upstream parts run too.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iron_amd import _lib, autograd

import _backward_oracle as B

pytestmark = pytest.mark.gpu

FUSED = os.environ.get("IRON_TRAIN_FUSE", "1")[:1] != "0"
NAN = float("nan")
_dev_params = {}
_touched = set()
_worst = {}           # (operator, route) -> worst error / F seen in this process (printed per test: the table of DESIGN 25)


def _note(op, route, ratio_f, who):
    key = (op, route + ("" if FUSED else " unfused"))
    if ratio_f > _worst.get(key, (0.0, ""))[0]:
        _worst[key] = (ratio_f, who)
    _touched.add(key)


GUARD = 1 << 18      # floats (1 MiB) of NaN behind every input and upstream buffer: a read past the end shows instead of going unnoticed


def _guarded(t):
    """`t` on the device, at the front of a buffer whose tail is NaN."""
    buf = torch.full((t.numel() + GUARD,), NAN, device="cuda")
    out = buf[:t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _params_on_device(net, cache=True):
    key = (net.kind, net.name)
    if cache and key in _dev_params:
        return _dev_params[key]
    p = {k: v.detach().float().contiguous().cuda() for k, v in net.sd.items()}
    if cache:
        _dev_params[key] = p
    return p


def run(net, n, batch_in, up, ws_mode="empty", short=0, cache=True):
    """One call of the operator's C entry on the batch.  Every output buffer is pre-filled with NaN, so a row or tensor the entry
    did not write cannot pass.  ws_mode: "empty" (torch.empty, as iron_amd/autograd.py passes it), "nan" or "ff" (the workspace of
    exactly *_workspace_bytes - short bytes filled with NaN / 0xFF bytes).  Returns (status, {parameter: gradient} on the CPU,
    [input gradients or None], raw device gradient buffers)."""
    lib = _lib.load_train()
    dev = torch.device("cuda", torch.cuda.current_device())
    params = _params_on_device(net, cache)
    grads = {k: torch.full_like(params[k], NAN) for k in net.param_names()}
    arr = (_lib.iron_train_layer * len(net.layers))()
    for i, (pre, wn) in enumerate(net.layers):
        v = params[pre + (".weight_v" if wn else ".weight")]
        arr[i].weight_v, arr[i].d_weight_v = v.data_ptr(), grads[pre + (".weight_v" if wn else ".weight")].data_ptr()
        arr[i].bias, arr[i].d_bias = params[pre + ".bias"].data_ptr(), grads[pre + ".bias"].data_ptr()
        arr[i].weight_g = params[pre + ".weight_g"].data_ptr() if wn else None
        arr[i].d_weight_g = grads[pre + ".weight_g"].data_ptr() if wn else None
        arr[i].out_dim, arr[i].in_dim = v.shape
    ins = [_guarded(t) for t in batch_in]
    ups = {k: (None if v is None else _guarded(v)) for k, v in up.items()}
    spec = net.spec
    if net.kind == "sdf":
        desc = _lib.iron_sdf_train_desc()
        desc.n_linear, desc.multires, desc.skip_layer, desc.layers = len(net.layers), net.meta["multires"], net.meta["skip"], arr
        nbytes = lib.iron_sdf_backward_workspace_bytes(C.byref(desc), n)
    elif net.kind == "render":
        desc = _lib.iron_render_train_desc()
        desc.n_linear, desc.mode, desc.multires, desc.multires_view = len(net.layers), _lib.MODES[spec.mode], spec.multires, spec.multires_view
        desc.d_feature, desc.d_out, desc.skip_layer, desc.squeeze_out = spec.d_feature, spec.d_out, net.meta["skip"], 1 if spec.squeeze_out else 0
        desc.output_bias, desc.output_scale, desc.squeeze_out_scale = float(spec.output_bias), float(spec.output_scale), float(spec.squeeze_out_scale)
        desc.layers = arr
        nbytes = lib.iron_render_backward_workspace_bytes(C.byref(desc), n)
    else:
        desc = _lib.iron_nerf_train_desc()
        desc.D, desc.W, desc.d_in, desc.d_in_view = spec.D, spec.W, spec.d_in, spec.d_in_view
        desc.multires, desc.multires_view, desc.skip, desc.layers = spec.multires, spec.multires_view, net.meta["skip"], arr
        nbytes = lib.iron_nerf_backward_workspace_bytes(C.byref(desc), n)
    assert nbytes > 0, "the entry refuses this layer table"
    ws = torch.empty(nbytes - short, dtype=torch.uint8, device=dev)
    if ws_mode == "nan":
        ws[:(nbytes - short) // 4 * 4].view(torch.float32).fill_(NAN)
    elif ws_mode == "ff":
        ws.fill_(255)
    st = _lib.stream_ptr(dev)
    in_grads = []
    if net.kind == "sdf":
        rc = lib.iron_sdf_backward(C.byref(desc), ins[0].data_ptr(), n, _lib.ptr(ups["s"]), _lib.ptr(ups["f"]), _lib.ptr(ups["g"]), ws.data_ptr(),
                                   nbytes - short, st)
    elif net.kind == "render":
        in_grads = [torch.full_like(t, NAN) if t.numel() else None for t in ins]
        rc = lib.iron_render_backward(C.byref(desc), ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), _lib.ptr(ins[3]) if ins[3].numel() else None,
                                      n, ups["o"].data_ptr(), *[_lib.ptr(g) for g in in_grads], ws.data_ptr(), nbytes - short, st)
    else:
        rc = lib.iron_nerf_backward(C.byref(desc), ins[0].data_ptr(), ins[1].data_ptr(), n, _lib.ptr(ups["a"]), _lib.ptr(ups["r"]), ws.data_ptr(),
                                    nbytes - short, st)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().reshape(net.sd[k].shape) for k, v in grads.items()}, [None if g is None else g.cpu() for g in in_grads], grads


def _one(net, n, live, parts, tag, route, op):
    """One embedded batch against the oracle; returns worst error / bound."""
    live, dropped = B.drop_kinks(net, live)
    assert dropped <= B.KINK_CAP * (len(live) + dropped), (tag, "kink rows", dropped)
    batch_in, up = B.embed(net, n, live, parts)
    if all(v is None for v in up.values()):
        return 0.0
    ex = B.expect(net, batch_in, up, live)
    rc, got, in_got, _ = run(net, n, batch_in, up)
    assert rc == 0, (tag, rc)
    worst, worst_f, who = B.compare_params(net, got, ex, tag)
    for j, ref in enumerate(ex.in_ref):
        if ref is None:   # the mode ignores this input: no path, exactly zero
            assert in_got[j] is None or float(in_got[j].abs().max()) == 0.0, (tag, "input", j)
            continue
        worst = max(worst, B.compare_rows(in_got[j], ref, ex.in_floor[j], live, tag + " input %d" % j))
        err = (in_got[j][live].double() - ref).norm(dim=1)
        ok = ex.in_floor[j] > 0
        rf = float((err[ok] / ex.in_floor[j][ok]).max()) if bool(ok.any()) else 0.0
        if rf > worst_f:
            worst_f, who = rf, "a row of input %d" % j
    _note(op, route, worst_f, "%s, %s" % (who, tag))
    return worst


def _report(title):
    assert autograd.numeric_status(reset=True) is False, "a finite operand raised the numeric flag"
    print(title + "; worst error / F by route so far: " + ", ".join("%s %s %.2f at %s" % (k[0], k[1], _worst[k][0], _worst[k][1]) for k in sorted(_touched) if k in _worst))
    _touched.clear()


@pytest.mark.parametrize("name", B.SDF_NETS)
def test_sdf_rows(name):
    """Sizes around the 256-row gate: with a gradient cotangent the rows are [n values | n tangents] (gate at 128 points, 32-point
    blocks), without one the gate is at 256 points (64-row blocks).  The smallest size of each route runs every part on its own and
    every live row on its own; a gradient-only loss leaves the last bias exactly 0 (compare_params: no path in the oracle)."""
    net = B.net_of("sdf", name)
    autograd.numeric_status(reset=True)
    worst, calls = 0.0, 0
    for sizes, parts_all, block, full, gate in ((B.SDF_TANGENT_SIZES, B.SDF_TANGENT_PARTS, 32, "sfg", 128), (B.SDF_PLAIN_SIZES, B.SDF_PLAIN_PARTS, 64, "sf", 256)):
        small = (sizes[0], gate)
        for n in sizes:
            live = B.live_set(n, block)
            cases = [(full, live)]
            if n in small:
                cases += [(p, live) for p in parts_all if p != full] + [(full, [r]) for r in live if len(live) > 1]
            route = ("row" if n >= gate else "split") + (" paired" if block == 32 else "")
            for parts, S in cases:
                worst = max(worst, _one(net, n, S, parts, "sdf %s n=%d %s S=%s" % (name, n, parts, S), route, "sdf"))
                calls += 1
    _report("sdf %-9s %d embedded batches, worst error / bound %.3f" % (name, calls, worst))


@pytest.mark.parametrize("name", B.RENDER_NETS)
def test_render_rows(name):
    """Parameter gradients, and d_points / d_normals / d_view_dirs / d_features row by row: every live row within its own floor, every
    other row exactly zero."""
    net = B.net_of("render", name)
    autograd.numeric_status(reset=True)
    worst, calls = 0.0, 0
    for n in B.NET_SIZES:
        live = B.live_set(n, 64)
        cases = [live] + ([[r] for r in live if len(live) > 1] if n in (1, 256) else [])
        for S in cases:
            worst = max(worst, _one(net, n, S, "o", "render %s n=%d S=%s" % (name, n, S), "row" if n >= 256 else "split", "render"))
            calls += 1
    _report("render %-20s %d embedded batches, worst error / bound %.3f" % (name, calls, worst))


def test_nerf_rows():
    net = B.net_of("nerf", "prod")
    autograd.numeric_status(reset=True)
    worst, calls = 0.0, 0
    for n in B.NET_SIZES:
        live = B.live_set(n, 64)
        cases = [("ar", live)]
        if n in (1, 256):
            cases += [("a", live), ("r", live)] + [("ar", [r]) for r in live if len(live) > 1]
        for parts, S in cases:
            worst = max(worst, _one(net, n, S, parts, "nerf n=%d %s S=%s" % (n, parts, S), "row" if n >= 256 else "split", "nerf"))
            calls += 1
    _report("nerf prod %d embedded batches, worst error / bound %.3f" % (calls, worst))


@pytest.mark.parametrize("tangent", [True, False])
@pytest.mark.parametrize("extra", B.SDF_CHUNK_EXTRA)
def test_sdf_chunk_edges(extra, tangent):
    """65 536 + {0, 1, 128, 129} points: the second chunk is absent, one point (split kernel), 128 points (row kernel with tangent rows,
    split kernel without) or 129; its gradients are ADDED to the first chunk's (beta = 1).  Live rows on both sides of the boundary."""
    net = B.net_of("sdf", "prod")
    autograd.numeric_status(reset=True)
    n = B.SDF_CHUNK + extra
    live = B.live_set(n, 32 if tangent else 64, B.SDF_CHUNK)
    w = _one(net, n, live, "sfg" if tangent else "sf", "sdf chunk +%d tangent=%s S=%s" % (extra, tangent, live), "chunk tail %d%s" % (extra, " paired" if tangent else ""), "sdf")
    _report("sdf chunk + %d tangent=%s S=%s: worst error / bound %.3f" % (extra, tangent, live, w))


@pytest.mark.parametrize("name", ["idr_0_4/prod", "idr_10_4_skip/prod"])
@pytest.mark.parametrize("extra", B.RENDER_CHUNK_EXTRA)
def test_render_chunk_edges(name, extra):
    net = B.net_of("render", name)
    autograd.numeric_status(reset=True)
    n = B.RENDER_CHUNK + extra
    live = B.live_set(n, 64, B.RENDER_CHUNK)
    w = _one(net, n, live, "o", "render chunk %s +%d S=%s" % (name, extra, live), "chunk tail %d" % extra, "render")
    _report("render chunk %s + %d S=%s: worst error / bound %.3f" % (name, extra, live, w))


# ---- workspace ---------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("kind,name,n,parts", [("sdf", "prod", 161, "sfg"), ("sdf", "n4_skip2", 321, "sf"), ("render", "idr_10_4_skip/prod", 321, "o"),
                                              ("nerf", "prod", 321, "ar")])
def test_workspace_is_scratch(kind, name, n, parts):
    """The entries take the workspace as they find it (iron_amd/autograd.py passes torch.empty; dW relies on beta = 0 in the first
    chunk): filled with NaN or with 0xFF bytes the results have the same bits as on the torch.empty run.  The bias gradient is a
    float atomicAdd over the 64-row strips of a column, so two identical runs are compared first: where THEY differ, only the weight
    gradients are compared bit for bit and the bias gradients against the oracle's floor.  A workspace one byte short is refused with
    nothing written; n = 0 writes zeros.  Dense upstream here (every row live): an uninitialised read shows wherever it lands."""
    net = B.net_of(kind, name)
    autograd.numeric_status(reset=True)
    live, _ = B.drop_kinks(net, list(range(n)))
    batch_in, up = B.embed(net, n, live, parts)
    rc, first, in_first, _ = run(net, n, batch_in, up)
    assert rc == 0
    rc, again, in_again, _ = run(net, n, batch_in, up)
    assert rc == 0
    moved = [k for k in first if not _same_bits(first[k], again[k])]
    print("%s %s n=%d: two identical runs differ in %s" % (kind, name, n, moved or "nothing"))
    assert all(k.endswith(".bias") for k in moved), moved      # the weight gradients have a fixed summation order
    if moved:   # every bias gradient is such a sum: one pair of runs that happened to agree on a tensor does not make it repeatable
        moved = [k for k in first if k.endswith(".bias")]
    ex = B.expect(net, batch_in, up, live)
    B.compare_params(net, first, ex, "dense %s %s" % (kind, name))
    for mode in ("nan", "ff"):
        rc, got, in_got, _ = run(net, n, batch_in, up, ws_mode=mode)
        assert rc == 0, mode
        for k in got:
            if k in moved:
                assert float((got[k].double() - ex.ref[k]).norm()) <= ex.bound(k), (mode, k)
            else:
                assert _same_bits(got[k], first[k]), (mode, k)
        for a, b in zip(in_got, in_first):
            assert (a is None and b is None) or _same_bits(a, b), mode
    rc, _, _, raw = run(net, n, batch_in, up, ws_mode="nan", short=1)
    assert rc == -5                                              # IRON_ERR_WORKSPACE
    assert all(bool(torch.isnan(v).all()) for v in raw.values())  # nothing was enqueued: every output still holds its fill
    empty_in, empty_up = B.embed(net, 0, [], parts)
    rc, zero, _, _ = run(net, 0, empty_in, empty_up, ws_mode="nan")
    assert rc == 0
    assert all(float(v.abs().max()) == 0.0 for v in zero.values())
    _report("workspace %s %s" % (kind, name))


# ---- activation probe --------------------------------------------------------------------------------------------------------
def _probe_net(width, rot, relu):
    W0, b0, W1, b1, z, asserted = B.probe_layers(width, rot, relu)
    sd = {"lin0.weight": W0, "lin0.bias": b0, "lin1.weight": W1, "lin1.bias": b1}
    layers = [("lin0", False), ("lin1", False)]
    if relu:
        spec = B.R.RenderSpec(d_feature=0, mode="points_only", d_in=3, d_out=1, n_layers=1, multires=0, multires_view=0, squeeze_out=False)
        net = B.Net("render", "probe", sd, spec, layers, dict(skip=-1))
    else:
        net = B.Net("sdf", "probe", sd, B.R.SDFSpec(d_out=1, n_layers=1, skip_in=(), multires=0), layers, dict(multires=0, skip=-1, d_out=1))
    return net, (W0, b0, W1, b1), z, asserted


def _probe_batch(n, live, relu, tangent):
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, 3, generator=g) * 2 - 1
    x[live] = torch.tensor(B.PROBE_X)
    d = torch.zeros(n, 1)
    d[live] = B.PROBE_D_SDF
    if relu:
        return (x, torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 0)), {"o": d}
    v = None
    if tangent:
        v = torch.zeros(n, 3)
        v[live] = torch.tensor(B.PROBE_V)
    return (x,), {"s": d, "f": None, "g": v}


@pytest.mark.parametrize("width", B.PROBE_FUSED_WIDTHS + B.PROBE_UNFUSED_WIDTHS)
def test_activation_probe_softplus(width):
    """A two-layer SDF net 3 -> width -> 1 (plain nn.Linear, multires 0) whose hidden pre-activation at the one live point is set per
    column (z = bias exactly: every first-layer row is orthogonal to the point).  d_bias of layer 0 is then
    zbar_j = s1 abar + s2 zdot adotbar, read off column by column against torch's F.softplus(beta = 100) under double backward in
    fp64, at 100 z = 0, +-0.5, +-5, +-15, 19.9, the fp32 neighbours of 20 / 25 / 60, -20, -60 and -87 .. -104, every stratum in every
    column over the 22 rotations.  Widths 256 / 217 / 129 take the fused epilogues (softplus100_fast: hardware exp2 / log2 / rcp)
    at n = 128 with a gradient cotangent (paired rows) and n = 256 without; 128 / 300 the unfused row kernel; n = 64 the split path
    with the activation passes as kernels of their own (expf / log1pf).  Bound per column: _backward_oracle.probe_bounds."""
    autograd.numeric_status(reset=True)
    n_strata = len(B.softplus_strata())
    worst, s2 = {}, {}
    for n, tangent in ((128, True), (256, False), (64, True), (64, False)):
        live = 37 % n
        batch_in, up = _probe_batch(n, live, False, tangent)
        for rot in range(n_strata):
            net, (W0, b0, W1, b1), z, _ = _probe_net(width, rot, False)
            r64 = B.probe_reference(W0, b0, W1, b1, False, tangent, torch.float64)
            r32 = B.probe_reference(W0, b0, W1, b1, False, tangent, torch.float32)
            bb, bw = B.probe_bounds(W0, W1, r64, r32, tangent)
            rc, got, _, _ = run(net, n, batch_in, up, cache=False)
            assert rc == 0
            eb = (got["lin0.bias"].double() - r64["b0"]).abs()
            ew = (got["lin0.weight"].double() - r64["w0"]).abs().max(dim=1).values
            j = int((eb / bb).argmax())
            assert bool((eb <= bb).all()), ("d_bias", width, n, tangent, rot, j, float(100 * z[j]), float(eb[j]), float(bb[j]))
            j = int((ew / bw).argmax())
            assert bool((ew <= bw).all()), ("d_weight", width, n, tangent, rot, j, float(100 * z[j]), float(ew[j]), float(bw[j]))
            # the output layer: d_weight = (a, adot-weighted tangent) of the hidden units, one fp32-accurate product per column
            e1 = (got["lin1.weight"].double() - r64["w1"]).abs()
            f1 = (r32["w1"].double() - r64["w1"]).abs()
            assert bool((e1 <= B.MARGIN * torch.maximum(f1, 2.0 ** -22 * r64["w1"].abs() + 1e-9)).all()), ("d_weight 1", width, n, tangent, rot)
            key = (n, tangent)
            worst[key] = max(worst.get(key, 0.0), float((eb / bb).max()), float((ew / bw).max()))
            if tangent and rot == 0:   # s2 as the device applied it just above torch's threshold: (zbar - abar) / (zdot adotbar) with s1 = 1
                w1 = W1[0].double()
                zd_all = W0.double() @ torch.tensor(B.PROBE_V, dtype=torch.float64)
                z_thr = np.min(np.where(100.0 * z.double().numpy() > 20.0, z.numpy(), np.inf))      # the stratum just above the threshold
                j = int(torch.where(torch.from_numpy(z.numpy() == z_thr), (zd_all * w1).abs(), torch.zeros_like(w1)).argmax())
                zdot = float(zd_all[j])
                s2[n] = (float(got["lin0.bias"][j]) - B.PROBE_D_SDF * float(w1[j])) / (zdot * float(w1[j]))
    print("softplus probe width %d: s2 applied at 100 z = 20 + 1 ulp: %s (exp form: %.2e; torch: 0)" % (width, {k: "%.2e" % v for k, v in s2.items()}, 100 * np.exp(-20.0)))
    _report("softplus probe width %d: worst error / bound %s" % (width, {k: round(v, 3) for k, v in worst.items()}))


@pytest.mark.parametrize("width", B.PROBE_FUSED_WIDTHS + B.PROBE_UNFUSED_WIDTHS)
def test_activation_probe_relu(width):
    """The same for a two-layer material net (points_only, no features): pre-activations of +-1e-3 and +-1 are asserted column by
    column (d_bias_j = [z_j > 0] abar_j); the columns at +-2^-126, one ulp-scale step from the kink, are left out (under KINK_CAP)."""
    autograd.numeric_status(reset=True)
    worst = 0.0
    for n in (256, 64):
        live = 37
        batch_in, up = _probe_batch(n, live, True, False)
        for rot in range(4):
            net, (W0, b0, W1, b1), z, asserted = _probe_net(width, rot, True)
            assert int((~asserted).sum()) <= B.KINK_CAP * width
            r64 = B.probe_reference(W0, b0, W1, b1, True, False, torch.float64)
            r32 = B.probe_reference(W0, b0, W1, b1, True, False, torch.float32)
            rc, got, in_got, _ = run(net, n, batch_in, up, cache=False)
            assert rc == 0
            abar = (B.PROBE_D_SDF * W1[0]).double().abs()
            bb = B.MARGIN * torch.maximum((r32["b0"].double() - r64["b0"]).abs(), 2.0 ** -22 * abar)
            eb = (got["lin0.bias"].double() - r64["b0"]).abs()
            ew = (got["lin0.weight"].double() - r64["w0"]).abs().max(dim=1).values
            assert bool((eb[asserted] <= bb[asserted]).all()), ("d_bias", width, n, rot)
            assert bool((ew[asserted] <= bb[asserted]).all()), ("d_weight", width, n, rot)
            assert bool((got["lin0.bias"][asserted & (z < 0)] == 0).all())          # a dead unit passes exactly nothing
            fx = (r32["x"].double() - r64["x"]).norm(dim=1)
            worst = max(worst, B.compare_rows(in_got[0], r64["x"], fx, [live], "relu probe d_points %d %d %d" % (width, n, rot)))
            worst = max(worst, float((eb[asserted] / bb[asserted]).max()))
    _report("relu probe width %d: worst error / bound %.3f" % (width, worst))


# ---- the operand scale ---------------------------------------------------------------------------------------------------------
def _gemm_dx(A, W):
    lib = _lib.load_train()
    m, k = A.shape
    n = W.shape[1]
    out = torch.full((m, n), NAN, device="cuda")
    nbytes = lib.iron_train_gemm_workspace_bytes(0, m, n)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = lib.iron_train_gemm(0, 0, m, n, k, A.data_ptr(), k, W.data_ptr(), n, 0.0, out.data_ptr(), n, ws.data_ptr(), nbytes, _lib.stream_ptr(A.device))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def test_operand_scale():
    """How much precision a small gradient row keeps beside a large one: every GEMM takes ONE power-of-two scale from the whole
    operand's |dZ|max (gemm_h2.h: gemm_scale_for brings the maximum into [2^13, 2^14)).

    Two live rows of the 8 x 256 SDF net without weight norm (so d_weight IS dW): A carries a feature cotangent of 1e3 on feature
    column 5, B one of d = 1e3 2^-k on feature column 100.  Row c_B of the last layer's weight gradient is then d h_B -- one product
    per element, formed under A's scale s = 2^(14 - 10) = 16 (frexp(1e3) = 0.977 2^10).

    Bound.  gemm_split8 writes an operand element v as hi + lo / 2048 with hi = fp16(v) and lo = fp16(2048 (v - f32(hi))), both
    rounded to nearest.  hi is off by <= 2^-11 |v| (normal) or <= 2^-25 (fp16 subnormal, |v| < 2^-14); v - hi is exact in fp32; lo
    loses <= 2^-11 of it or <= 2^-25, i.e. <= 2^-22 |v| or <= 2^-36 in units of v.  So the pair represents v to
    max(2^-22 |v|, 2^-36).  With v = s d for the gradient and v = h_i for the activation (unscaled), the three MFMA products
    hi hi + (hi lo + lo hi) / 2048 drop lo lo (<= 2^-22 |s d h_i|), and the accumulators and the final fmaf round <= 4 times at
    2^-24.  Undoing the scale:
        |dW[c_B, i] - d h_i| <= [ |h_i| max(2^-22 s d, 2^-36) + s d max(2^-22 |h_i|, 2^-36) ] / s + (2^-22 + 2^-22) d |h_i|
    plus the error of the recomputed h_i itself, d x max(4 |h32_i - h64_i|, TOL_SDF max|h|) (the forward's accepted error).  The
    absolute term 2^-36 / s is what a small row pays for the shared scale: relative to d h_i it is 2^-40 / d, 1e-3 at d ~ 1e-9
    (k ~ 40) if the matrix pipe keeps fp16 subnormals.  Measured relative errors are printed per k for DESIGN 25, for this product
    (split kernel, K = points) and for dX = dZ W through iron_train_gemm at 64 rows (split kernel) and 256 rows (row kernel)."""
    net = B.net_of("sdf", "n8_nown")
    autograd.numeric_status(reset=True)
    ra, rb, ca, cb = B.SCALE_ROW_A, B.SCALE_ROW_B, B.SCALE_COL_A, B.SCALE_COL_B
    last = net.layers[-1][0] + ".weight"
    ks = B.SCALE_KS + (40, 44, 48)
    table = {}
    for n in (64, 256):
        batch_in, _ = B.embed(net, n, [ra, rb], "f")
        for k in ks:
            d = B.SCALE_A * 2.0 ** -k
            f = torch.zeros(n, 256)
            f[rb, cb] = d
            only_b = {"s": None, "f": f.clone(), "g": None}
            r64, _ = B.oracle(net, batch_in, only_b, [rb], torch.float64)
            r32, _ = B.oracle(net, batch_in, only_b, [rb], torch.float32)
            h64, h32 = r64[last][cb + 1] / d, r32[last][cb + 1] / d
            f[ra, ca] = B.SCALE_A
            rc, got, _, _ = run(net, n, batch_in, {"s": None, "f": f, "g": None})
            assert rc == 0
            err = (got[last][cb + 1].double() - d * h64).abs()
            bound = B.scale_bound(h64, h32, d, B.SCALE_A)
            rel = float(err.norm() / (d * h64.norm()))
            table[("dW", n, k)] = rel
            assert bool((err <= bound).all()), ("dW row under A's scale", n, k, float((err / bound).max()), rel)
            assert autograd.numeric_status(reset=True) is False, ("a finite operand raised the numeric flag", n, k)
    # dX = dZ W on its own: row B of a [rows, 256] gradient operand beside row A, split kernel (64 rows) and row kernel (256 rows)
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(256, 256, generator=g) / 16.0)
    ua, ub = torch.rand(256, generator=g) * 0.5 + 0.5, torch.rand(256, generator=g) * 0.5 + 0.5
    s = B.gemm_scale(B.SCALE_A)
    for rows in (64, 256):
        for k in ks:
            d = B.SCALE_A * 2.0 ** -k
            A = torch.zeros(rows, 256)
            A[ra], A[rb] = B.SCALE_A * ua, d * ub
            out = _gemm_dx(A.cuda(), W.cuda()).cpu()
            ref = A[rb].double() @ W.double()
            err = (out[rb].double() - ref).abs()
            aw, ad = W.double().abs(), A[rb].double().abs()
            rep_d = torch.clamp(2.0 ** -22 * s * ad, min=2.0 ** -36)
            rep_w = torch.clamp(2.0 ** -22 * aw, min=2.0 ** -36)
            bound = (rep_d @ aw + (s * ad) @ rep_w) / s + (2.0 ** -22 + 256 * 2.0 ** -24) * (ad @ aw)    # + fp32 accumulation over K = 256
            table[("dX", rows, k)] = float(err.norm() / ref.norm())
            assert bool((err <= bound).all()), ("dX row under A's scale", rows, k, float((err / bound).max()))
            assert autograd.numeric_status(reset=True) is False, ("a finite operand raised the numeric flag", rows, k)
    print("operand scale: relative error of the small row, amax = 1e3, d = 1e3 2^-k")
    for what, size in (("dW", 64), ("dW", 256), ("dX", 64), ("dX", 256)):
        print("  %s %3d rows: " % (what, size) + "  ".join("k=%d %.1e" % (k, table[(what, size, k)]) for k in ks))
        over = [k for k in ks if table[(what, size, k)] > 1e-3]
        print("  %s %3d rows: first k with relative error > 1e-3: %s" % (what, size, over[0] if over else "none up to %d" % ks[-1]))
