"""Host-only checks of the fused hash-grid field's two launching entries (iron_hashgrid_field_eval, include/iron_hip.h,
csrc/hashgrid_field.hip; iron_hashgrid_field_backward, include/iron_train.h, csrc/hashgrid_field_train.hip): the argument checks, all
of which return before any device work, and their ORDER, which differs between the two behind the descriptor (the evaluation looks
at its pointers before the size limit, the backward after it).  The companion of test_hashfield_trace_host.py for the tracer's
entries; the codes are those the entries returned before they shared their field binding.  Pointers that must merely be non-null are
made-up addresses: an entry that returned only after touching one would fault here instead of passing.  n == 0 on the backward entry
enqueues memsets and is left out."""
import ctypes as C

import pytest

from iron_amd import _lib, build
from test_hashfield_trace_host import _desc

OK, BAD_ARG, RANGE, WORKSPACE = _lib.IRON_OK, _lib.IRON_ERR_BAD_ARG, _lib.IRON_ERR_RANGE, -5
FAKE = 0x1000      # non-null, 256-byte aligned, never dereferenced
LIMIT = (2 ** 31 - 1) * 32   # points per call of both entries
REFUSED = (dict(n_neurons=48), dict(n_hidden=5), dict(n_out=17), dict(levels=32, features=8))


@pytest.fixture(scope="module")
def libs():
    build.build()
    return _lib.load(), _lib.load_train()


def _eval(lib, desc, n, grad=False, **over):
    a = dict(p=FAKE, table=FAKE, packed=FAKE, out=FAKE)
    a.update(over)
    return lib.iron_hashgrid_field_eval(C.byref(desc) if desc is not None else None, a["p"], n, None, None, a["table"], a["packed"], a["out"],
                                        FAKE if grad else None, None)


def _backward(libt, desc, n, ws_bytes=None, **over):
    a = dict(p=FAKE, table=FAKE, packed=FAKE, train_packed=FAKE, d_weights=FAKE, ws=FAKE)
    a.update(over)
    d = C.byref(desc) if desc is not None else None
    if ws_bytes is None:
        ws_bytes = libt.iron_hashgrid_field_backward_workspace_bytes(d, n) if desc is not None and 0 <= n <= 10 ** 6 else 1 << 40
    return libt.iron_hashgrid_field_backward(d, a["p"], n, None, None, a["table"], a["packed"], a["train_packed"], FAKE, FAKE, a["d_weights"], FAKE,
                                             None, None, a["ws"], ws_bytes, None)


@pytest.mark.parametrize("grad", (False, True))
def test_eval_argument_checks_and_their_order(libs, grad):
    lib, n = libs[0], 100
    assert _eval(lib, None, n, grad) == BAD_ARG
    for bad in REFUSED:
        assert _eval(lib, _desc(**bad), n, grad) == RANGE
        assert _eval(lib, _desc(**bad), -1, grad) == RANGE               # the descriptor is looked at first
        assert _eval(lib, _desc(**bad), 0, grad, p=None) == RANGE
    desc = _desc()
    assert _eval(lib, desc, -1, grad) == BAD_ARG
    assert _eval(lib, desc, 0, grad, p=None, table=None, packed=None, out=None) == OK   # no points: nothing is needed
    for k in ("p", "table", "packed", "out"):
        assert _eval(lib, desc, n, grad, **{k: None}) == BAD_ARG, k
        assert _eval(lib, desc, LIMIT + 1, grad, **{k: None}) == BAD_ARG, k    # the pointers before the size limit
    for off in (4, 8, 12):
        assert _eval(lib, desc, n, grad, packed=FAKE + off) == BAD_ARG
    assert _eval(lib, desc, LIMIT + 1, grad) == RANGE
    assert _eval(lib, desc, 2 ** 62, grad) == RANGE
    for head in ((16, 1), (128, 3), (64, 4)):   # accepted shapes pass the descriptor check (n = 0: nothing is launched)
        assert _eval(lib, _desc(n_neurons=head[0], n_hidden=head[1]), 0, grad) == OK


def test_backward_argument_checks_and_their_order(libs):
    libt, n = libs[1], 100
    assert _backward(libt, None, n) == BAD_ARG
    for bad in REFUSED + (dict(n_neurons=128),):   # the backward is not built for 128 neurons
        assert _backward(libt, _desc(**bad), n) == RANGE
        assert _backward(libt, _desc(**bad), -1) == RANGE
        assert _backward(libt, _desc(**bad), n, d_weights=None) == RANGE
    desc = _desc()
    assert _backward(libt, desc, -1) == BAD_ARG
    assert _backward(libt, desc, n, d_weights=None) == BAD_ARG
    assert _backward(libt, desc, LIMIT + 1, d_weights=None) == BAD_ARG        # d_weights before the size limit ...
    for k in ("p", "table", "packed", "train_packed", "ws"):
        assert _backward(libt, desc, n, **{k: None}) == BAD_ARG, k
        assert _backward(libt, desc, LIMIT + 1, **{k: None}) == RANGE, k      # ... the other pointers after it
    assert _backward(libt, desc, LIMIT + 1) == RANGE
    assert _backward(libt, desc, 2 ** 62) == RANGE
    for off in (4, 8, 12):
        assert _backward(libt, desc, n, packed=FAKE + off) == BAD_ARG
        assert _backward(libt, desc, n, train_packed=FAKE + off) == BAD_ARG
    for off in (16, 64, 128):
        assert _backward(libt, desc, n, ws=FAKE + off) == BAD_ARG
    need = libt.iron_hashgrid_field_backward_workspace_bytes(C.byref(desc), n)
    assert need > 0
    assert _backward(libt, desc, n, ws_bytes=need - 1) == WORKSPACE
    assert _backward(libt, desc, n, ws_bytes=0) == WORKSPACE
    assert _backward(libt, desc, n, ws_bytes=need - 1, packed=None) == BAD_ARG   # the pointers before the workspace size
