"""GPU: RayTracer's front end is one argument, result and stats layer for its three arms (iron_amd/raytracer.py: _ray_call, _outputs,
_Arm): an SDFNetwork behind SDFHandle (csrc/trace.hip), an analytic sphere behind SDFCallable (csrc/trace_any.hip) and
a hash-grid field behind TCNNSDF.as_traced (csrc/hashgrid_trace.hip).  Every test runs on all three with n = 65 rays, one wave and
one ray: the same malformed arguments are refused by every entry of every arm before anything is launched (the C entries read n
entries from every array and cannot check it), the same argument shapes are accepted with the same bits, and last_stats carries the
arm's own keys."""
import functools

import pytest
import torch

import _hashfield_oracle as H
from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, SDFCallable, SDFHandle, intersect_sphere
from test_gpu_hashfield import make_field

pytestmark = pytest.mark.gpu
ARMS = ("network", "callable", "hashfield")
N = 65
KEYS = ("convergent_mask", "points", "sdf", "distance")
STATS_KEYS = {"network": set(_lib.TRACE_STATS_FIELDS),
              "callable": {"n_evals", "n_calls", "n_sampler", "n_bisect", "n_bisect_iters"},
              "hashfield": {k for k in _lib.HASHGRID_TRACE_STATS_FIELDS if not k.startswith("reserved")}}


def _sphere(x):
    return x.norm(dim=-1) - 0.5


@functools.lru_cache(maxsize=None)
def sdf_of(arm):
    if arm == "network":
        return SDFHandle(scenes.build_networks("S0")["sdf_network"].cuda())
    if arm == "callable":
        return SDFCallable(_sphere)
    c, _ = H.case_encoding("hashed_tiny_table")
    return make_field(c["cfg"], (16, 1), "ReLU", 1, c["table"], H.case_weights("hashed_tiny_table", (16, 1), 1)).as_traced(0.5, 0.5)


@functools.lru_cache(maxsize=None)
def rays():
    """65 rays from the middle of the 48 x 48 fixture view, where the unit sphere is: o, d, near, far, hit"""
    K, W2C = scenes.fixture_camera_matrices(48, 48)
    cam = Camera(48, 48, K.cuda(), W2C.cuda())
    o, d, _ = cam.get_rays(cam.get_uv())
    s = slice(24 * 48 + 5, 24 * 48 + 5 + N)
    o, d = o.reshape(-1, 3)[s].contiguous(), d.reshape(-1, 3)[s].contiguous()
    hit, near, far = intersect_sphere(o, d, 1.0)
    assert bool(hit.any())
    return o, d, near.contiguous(), far.contiguous(), hit.contiguous()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# the table of test_gpu_hashfield_trace.test_refusals: (what is wrong, the argument it is done to, the message)
WRONG = (("cpu", lambda t: t.cpu(), "CUDA"), ("double", lambda t: t.double(), "float32"), ("short", lambda t: t[:-1], "one entry per ray"))
MASK_WRONG = (("cpu", lambda t: t.cpu(), "work_mask"), ("short", lambda t: t[:-1], "work_mask"), ("float", lambda t: t.float(), "work_mask"))
INDEX_WRONG = (("cpu", lambda t: t.cpu(), "ray_index"), ("short", lambda t: t[:-1], "ray_index"), ("int32", lambda t: t.int(), "ray_index"))


def refusals(call, args, floats, mask=None, index=None):
    """call(*args) with one argument made wrong at a time.  floats: positions of the fp32 arguments, the first two of them ray_o and
    ray_d (a short ray_o makes every other argument the odd one: still one entry per ray); mask, index: positions of work_mask and
    ray_index"""
    tried = 0
    for pos, table in [(p, WRONG) for p in floats] + [(p, MASK_WRONG) for p in (mask,) if p is not None] + [
            (p, INDEX_WRONG) for p in (index,) if p is not None]:
        for what, spoil, match in table:
            bad = list(args)
            bad[pos] = spoil(args[pos])
            with pytest.raises(_lib.IronError, match=match):
                call(*bad)
            tried += 1
    with pytest.raises(_lib.IronError, match="CUDA"):   # everything on the host
        call(*[a.cpu() for a in args])
    return tried + 1


@pytest.mark.parametrize("arm", ARMS)
def test_the_same_refusals_on_every_arm(arm, monkeypatch):
    sdf = sdf_of(arm)
    o, d, near, far, hit = rays()
    tr = RayTracer()
    ok = tr(sdf, o, d, near, far, hit)   # the arm works (and has built what it builds on first use) before its library is taken away
    assert ok["convergent_mask"].shape == (N,)

    def launched(*a, **k):
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "load", launched)
    n = refusals(lambda *a: tr.forward(sdf, *a), (o, d, near, far, hit), (0, 1, 2, 3), mask=4)
    n += refusals(lambda *a: tr.occluded(sdf, *a), (o, d, near, far, hit), (0, 1, 2, 3), mask=4)
    n += refusals(lambda *a: tr.sphere_tracing(sdf, *a), (o, d, near, far, hit), (0, 1, 2, 3), mask=4)
    n += refusals(lambda *a: tr.ray_sampler(sdf, *a), (o, d, near, far), (0, 1, 2, 3))
    n += refusals(lambda f0, f1, d0, d1, ro, rd: tr.rootfind(sdf, f0, f1, d0, d1, ro, rd), (near, far, near, far, o, d), (4, 5, 0, 1, 2, 3))
    if arm == "network":
        idx = torch.arange(N, device="cuda")
        n += refusals(lambda *a: tr.phase_begin(sdf, *a, 1, N), (o, d, near, far, hit, idx), (0, 1, 2, 3), mask=4, index=5)
        n += refusals(lambda *a: tr.forward_phased(sdf, *a, 1, N, lambda x: None), (o, d, near, far, hit, idx), (0, 1, 2, 3), mask=4, index=5)
    assert n == (4 * 3 + 3 + 1) * 3 + (4 * 3 + 1) + (6 * 3 + 1) + (2 * (4 * 3 + 3 + 3 + 1) if arm == "network" else 0)
    assert tr.last_stats is None


@pytest.mark.parametrize("arm", ARMS)
def test_the_same_argument_shapes_are_accepted_on_every_arm(arm):
    sdf = sdf_of(arm)
    o, d, near, far, hit = rays()
    tr = RayTracer()
    want = tr(sdf, o, d, near, far, hit)
    strided = torch.stack((d, -d), dim=1)[:, 0]
    assert not strided.is_contiguous() and torch.equal(strided, d)
    got = tr(sdf, o, strided, near.unsqueeze(-1), far.unsqueeze(-1), hit.unsqueeze(-1))
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(bits(got[k]), bits(want[k])), k
    assert torch.equal(tr.occluded(sdf, o, strided, near.unsqueeze(-1), far.unsqueeze(-1), hit.unsqueeze(-1)), want["convergent_mask"])
    assert torch.equal(tr.occluded(sdf, o, d, near, far), tr.occluded(sdf, o, d, near, far, torch.ones_like(hit)))   # None: every ray
    none = tr(sdf, o[:0], d[:0], near[:0], far[:0], hit[:0])
    assert [tuple(none[k].shape) for k in KEYS] == [(0,), (0, 3), (0,), (0,)]
    assert tr.occluded(sdf, o[:0], d[:0], near[:0], far[:0]).shape == (0,)


@pytest.mark.parametrize("arm", ARMS)
def test_last_stats_carries_the_arms_own_keys(arm):
    sdf = sdf_of(arm)
    o, d, near, far, hit = rays()
    tr = RayTracer()
    tr(sdf, o, d, near, far, hit)
    assert tr.last_stats is None   # not asked for: nothing is read back
    out = tr(sdf, o, d, near, far, hit, collect_stats=True)
    assert set(tr.last_stats) == STATS_KEYS[arm] and all(isinstance(v, int) for v in tr.last_stats.values())
    assert tr.last_stats["n_evals"] >= int(hit.sum())
    tr.last_stats = None
    occ = tr.occluded(sdf, o, d, near, far, hit, collect_stats=True)
    assert set(tr.last_stats) == STATS_KEYS[arm]
    assert torch.equal(occ, out["convergent_mask"])
