"""Host-only checks of the hash-grid tracer's C ABI (include/iron_hip.h, iron_hashgrid_trace_*; csrc/hashgrid_trace.hip): workspace
sizing and the argument checks, all of which return before any device work.  Pointers that must merely be non-null are made-up
addresses: an entry that returned only after touching one would fault here instead of passing."""
import ctypes as C

import pytest

from iron_amd import _lib, build

INT_MAX = 2 ** 31 - 1
FAKE = 0x1000   # non-null, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _desc(n_neurons=64, n_hidden=2, n_out=1, act="ReLU", levels=16, features=2):
    d = _lib.iron_hashgrid_field_desc()
    d.encoding.n_levels, d.encoding.n_features_per_level = levels, features
    d.encoding.log2_hashmap_size, d.encoding.base_resolution, d.encoding.per_level_scale = 15, 16, 1.5
    d.n_neurons, d.n_hidden_layers, d.n_out = n_neurons, n_hidden, n_out
    d.activation = _lib.IRON_FIELD_ACT[act]
    return d


def _params(n_steps=128, chunk=0, iters=16):
    p = _lib.iron_trace_params()
    p.sdf_threshold, p.sphere_tracing_iters, p.n_steps, p.chunk = 5e-5, iters, n_steps, chunk
    return p


def _trace(lib, desc, prm, n, ws_bytes, null=(), entry="trace"):
    """the entry with made-up pointers; the names in `null` are passed as NULL"""
    a = {k: FAKE for k in ("table", "packed", "lin", "o", "d", "near", "far", "work", "conv", "points", "sdf", "dist", "ws")}
    for k in null:
        a[k] = None
    head = (C.byref(desc) if desc is not None else None, C.byref(prm) if prm is not None else None, None, None, a["table"], a["packed"], a["lin"],
            a["o"], a["d"])
    if entry == "trace":
        return lib.iron_hashgrid_trace(*head, a["near"], a["far"], a["work"], n, a["conv"], a["points"], a["sdf"], a["dist"], None, a["ws"],
                                       ws_bytes, None)
    if entry == "occluded":
        return lib.iron_hashgrid_trace_occluded(*head, a["near"], a["far"], a["work"], n, a["conv"], None, a["ws"], ws_bytes, None)
    stage = int(entry[-1])
    return lib.iron_hashgrid_trace_stage(stage, *head, a["near"], a["far"], a["near"], a["far"], a["work"], n, a["conv"], a["conv"], a["points"],
                                         a["sdf"], a["dist"], None, a["ws"], ws_bytes, None)


ENTRIES = ("trace", "occluded", "stage0", "stage1", "stage2")


def test_workspace_bytes_grow_with_n_and_end_at_int_max(lib):
    prm = _params()
    sizes = [lib.iron_hashgrid_trace_workspace_bytes(n, C.byref(prm)) for n in (0, 1, 63, 64, 65, 1000, 1024, 1025, 10 ** 6, INT_MAX - 1)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert lib.iron_hashgrid_trace_workspace_bytes(INT_MAX, C.byref(prm)) == 0
    assert lib.iron_hashgrid_trace_workspace_bytes(2 ** 40, C.byref(prm)) == 0
    assert lib.iron_hashgrid_trace_workspace_bytes(-1, C.byref(prm)) == 0
    # the chunk table: one int32 per chunk
    one = lib.iron_hashgrid_trace_workspace_bytes(10 ** 6, C.byref(_params(chunk=1)))
    assert one >= sizes[8] and one - sizes[8] <= 4 * 10 ** 6 + 256
    assert lib.iron_hashgrid_trace_workspace_bytes(1000, None) == sizes[5]


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers_and_short_workspaces_are_bad_arguments(lib, entry):
    desc, prm, n = _desc(), _params(), 100
    need = lib.iron_hashgrid_trace_workspace_bytes(n, C.byref(prm))
    assert _trace(lib, None, prm, n, need, entry=entry) == _lib.IRON_ERR_BAD_ARG
    assert _trace(lib, desc, None, n, need, entry=entry) == _lib.IRON_ERR_BAD_ARG
    names = {"trace": ("table", "packed", "lin", "o", "d", "near", "far", "work", "conv", "points", "sdf", "dist", "ws"),
             "occluded": ("table", "packed", "lin", "o", "d", "near", "far", "work", "conv", "ws"),
             "stage0": ("table", "packed", "o", "d", "near", "far", "work", "conv", "points", "sdf", "dist", "ws"),
             "stage1": ("table", "packed", "lin", "o", "d", "near", "far", "conv", "points", "sdf", "dist", "ws"),
             "stage2": ("table", "packed", "o", "d", "near", "far", "conv", "points", "sdf", "dist", "ws")}[entry]
    for k in names:
        assert _trace(lib, desc, prm, n, need, null=(k,), entry=entry) == _lib.IRON_ERR_BAD_ARG, k
    assert _trace(lib, desc, prm, n, need - 1, entry=entry) == _lib.IRON_ERR_BAD_ARG
    assert _trace(lib, desc, prm, n, 0, entry=entry) == _lib.IRON_ERR_BAD_ARG
    assert _trace(lib, desc, prm, -1, need, entry=entry) == _lib.IRON_ERR_BAD_ARG
    assert _trace(lib, desc, prm, INT_MAX, need, entry=entry) == _lib.IRON_ERR_BAD_ARG
    assert _trace(lib, desc, _params(iters=-1), n, need, entry=entry) == _lib.IRON_ERR_BAD_ARG


def test_stage_number_outside_0_to_2_is_a_bad_argument(lib):
    desc, prm = _desc(), _params()
    for stage in (-1, 3):
        rc = lib.iron_hashgrid_trace_stage(stage, C.byref(desc), C.byref(prm), None, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                           FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 1 << 20, None)
        assert rc == _lib.IRON_ERR_BAD_ARG


@pytest.mark.parametrize("entry", ENTRIES)
def test_refused_shapes_and_step_counts_are_range_errors(lib, entry):
    n = 100
    need = lib.iron_hashgrid_trace_workspace_bytes(n, C.byref(_params()))
    for bad in (_desc(n_neurons=48), _desc(n_hidden=5), _desc(n_out=17), _desc(levels=32, features=8)):
        assert lib.iron_hashgrid_field_check(C.byref(bad), None) == _lib.IRON_ERR_RANGE
        assert _trace(lib, bad, _params(), n, need, entry=entry) == _lib.IRON_ERR_RANGE
    for n_steps in (-1, 0, 1, 4097):
        assert _trace(lib, _desc(), _params(n_steps=n_steps), n, need, entry=entry) == _lib.IRON_ERR_RANGE
        assert _trace(lib, _desc(), _params(n_steps=n_steps), 0, need, entry=entry) == _lib.IRON_ERR_RANGE   # refused whatever n is
    for n_steps in (2, 4096):   # the ends of the range pass the check (n = 0: nothing is launched)
        assert _trace(lib, _desc(), _params(n_steps=n_steps), 0, need, entry=entry) == _lib.IRON_OK


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_rays_is_ok_and_needs_no_buffers(lib, entry):
    every = ("table", "packed", "lin", "o", "d", "near", "far", "work", "conv", "points", "sdf", "dist", "ws")
    for head in ((64, 2), (16, 1), (128, 3), (64, 4)):
        assert _trace(lib, _desc(n_neurons=head[0], n_hidden=head[1]), _params(), 0, 0, null=every, entry=entry) == _lib.IRON_OK
