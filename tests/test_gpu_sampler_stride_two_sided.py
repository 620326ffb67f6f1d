"""GPU: the two-sided stride of the screen's adaptive march (csrc/trace.hip k_sampler_screen) changes passes, never results.

After a good block the next one starts 1 + reach(e_7) behind e_7, a gap only e_7 vouches for; the gaps inside that block have an
evaluated sample at each end, so where the previous block's last two values rise its stride is up to twice the first gap.  Every gap
is certified after the evaluation by the unchanged walk, or the rest of the block is discarded and the slot resumes at stride 1
behind its last good sample -- with the stride no longer the first gap, a block discarded at its first sample resumes behind the
PREVIOUS block's last sample, which is found from that sample's parked value.

On S1, one bumpy field and one generalised net of tests/_hard_fields.py, 56 x 56 rays each, the dense sampler alone
(iron_trace_stage(1) on the rays and ranges sphere tracing leaves it) and the whole tracer (max_num_rays = 1000: four bisection
chunks) run with the rule on, with iron_sampler_screen_debug(6, 1) (one-sided: a block's stride is its first gap) and with
iron_set_sampler_stride(0): every output bit-equal, the tracer's statistics (n_evals among them) equal, the screen's and the slope
guard's status bits clear.  Against the one-sided march the passes fall on S1 and rise by no more than 3 % on the generalised net,
where strided blocks are discarded in numbers.  Under the calibrated slope bound a block is never discarded at its first sample (the
bound is twice the largest slope, and that takes a slope above half of it); a forced bound far below the field's slope makes it
common, and the march must still end, with a stride-1 pass behind every restart.

Measured on one MI355X (passes one-sided -> two-sided; sampler alone / whole tracer; the sampler's list is not the same from run
to run where rays overflow the resolve list): S1 1 446 -> 1 360 / 1 837 -> 1 766, bumpy03_s1 5 800 -> 5 851 (1.009), gen0 6 238 ->
6 266 / 6 832 -> 6 878 (1.004 / 1.007); the benchmark's frame (S0 800 x 800) 526 320 -> 486 521.  On rays that are NOT the sampler's
-- every ray of the view over its whole [near, far], approaching the surface instead of leaving it -- an earlier form of the rule
(a rise of L / 32 was enough) cost about 1 % (S1 21 640 -> 21 843): no caller marches those."""
import ctypes as C
import functools

import pytest
import torch

import _hard_fields as HF
from iron_amd import _lib, scenes
from iron_amd.raytracer import Camera, RayTracer, SDFHandle, intersect_sphere, raytrace_camera

pytestmark = pytest.mark.gpu
KEYS = ("convergent_mask", "points", "sdf", "distance", "depth")
FIELDS = ("S1", "bumpy03_s1", "gen0")
TWO_SIDED, ONE_SIDED, OFF = "two_sided", "one_sided", "off"
MODES = (OFF, ONE_SIDED, TWO_SIDED)
GEN_ALLOWANCE = 1.03   # passes on a generalised net against the one-sided march (the emulation: 1.006 - 1.017)


def _dev():
    return _lib.stream_ptr(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def _net(name):
    return (scenes.build_networks(name)["sdf_network"] if name in ("S0", "S1", "S3") else HF.build(name)).cuda()


def _camera(name):
    K, W2C = scenes.fixture_camera_matrices(HF.RES, HF.RES, 0.0 if name.startswith("S") else HF.yaw_of(name))
    return Camera(HF.RES, HF.RES, K.cuda(), W2C.cuda())


def _status(net):
    st = C.c_int32(0)
    _lib.check(_lib.load().iron_net_numeric_status(net.hip_net().handle, C.byref(st), _dev()))
    return st.value


def _counts():
    lib = _lib.load()
    ws = _lib.current_workspace(torch.device("cuda", 0), "trace")
    assert ws is not None
    a, b, d = (C.c_double * 5)(), (C.c_double * 4)(), (C.c_double * 9)()
    _lib.check(lib.iron_trace_screen_counts(ws.data_ptr(), a, _dev()))
    _lib.check(lib.iron_trace_stride_counts(ws.data_ptr(), b, _dev()))
    _lib.check(lib.iron_trace_stride_detail(ws.data_ptr(), d, _dev()))
    return {"screened": a[0], "resolved": a[1], "overflow": a[2], "pending": a[4],
            "passes": b[0], "strided": b[1], "slope": b[2], "adaptive": b[3], "restarts": d[2]}


class _mode:
    """The march of the calls inside: the stride switch and the one-sided hook, restored on the way out."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        lib = _lib.load()
        self.prev = lib.iron_set_sampler_stride(0 if self.mode == OFF else 1)
        _lib.check(lib.iron_sampler_screen_debug(6, 1.0 if self.mode == ONE_SIDED else 0.0))

    def __exit__(self, *exc):
        lib = _lib.load()
        _lib.check(lib.iron_sampler_screen_debug(6, 0.0))
        lib.iron_set_sampler_stride(self.prev)


@functools.lru_cache(maxsize=None)
def _sampler_inputs(name):
    """What the tracer hands its dense sampler: the rays sphere tracing (iron_trace_stage(0), which no switch of the march touches)
    leaves unfinished, over [acc_dis, far] where the last distance is positive and [near, acc_dis] where the ray has overshot."""
    cam = _camera(name)
    ro, rd, _ = cam.get_rays(cam.get_uv())
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    hit, near, far = intersect_sphere(ro, rd, 1.0)
    _, unf, _, s, t = RayTracer().sphere_tracing(SDFHandle(_net(name)), ro, rd, near, far, hit)
    s_min, s_max = HF.sampler_ranges(s[unf], t[unf], near[unf], far[unf])
    assert int(unf.sum()) > 100
    return ro[unf].contiguous(), rd[unf].contiguous(), s_min.contiguous(), s_max.contiguous()


def _sampler(name, mode, net=None):
    """iron_trace_stage(1) on the sampler's inputs."""
    ro, rd, s_min, s_max = _sampler_inputs(name)
    with _mode(mode):
        out = [x.clone() for x in RayTracer().ray_sampler(SDFHandle(net or _net(name)), ro, rd, s_min, s_max)]
        torch.cuda.synchronize()
        return out, _counts()


def _tracer(name, mode):
    import iron_amd.raytracer as RT
    old = RT.VERBOSE_MODE
    with _mode(mode):
        try:
            RT.VERBOSE_MODE = True
            tr = RayTracer()
            res = raytrace_camera(_camera(name), _net(name), tr, max_num_rays=HF.CHUNK)
            torch.cuda.synchronize()
            return {k: res[k].clone() for k in KEYS}, dict(tr.last_stats), _counts()
        finally:
            RT.VERBOSE_MODE = old


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Every march of one field, run once: {mode: (sampler outputs, sampler counts, tracer outputs, tracer stats, tracer counts)}."""
    runs = {}
    for m in MODES:
        s_out, s_cnt = _sampler(name, m)
        t_out, t_stats, t_cnt = _tracer(name, m)
        print("two-sided stride", name, m, "stage(1)", s_cnt, "| tracer", t_cnt, "n_evals", t_stats["n_evals"])
        runs[m] = (s_out, s_cnt, t_out, t_stats, t_cnt)
    runs["status"] = _status(_net(name))
    return runs


@torch.no_grad()
@pytest.mark.parametrize("name", FIELDS)
def test_results_do_not_depend_on_the_stride_choice(name):
    runs = _runs(name)
    want_s, c0_s, want_t, want_stats, c0_t = runs[OFF]
    assert c0_s["adaptive"] == 0 and c0_s["strided"] == 0 and c0_t["adaptive"] == 0 and c0_t["strided"] == 0, (c0_s, c0_t)
    for m in (ONE_SIDED, TWO_SIDED):
        got_s, c_s, got_t, stats, c_t = runs[m]
        assert c_s["adaptive"] == 1 and c_s["strided"] > 0 and c_t["adaptive"] == 1, (m, c_s, c_t)
        assert len(got_s) == len(want_s)
        for i, (a, b) in enumerate(zip(got_s, want_s)):
            assert torch.equal(a, b), (m, "stage(1) output", i)
        for k in KEYS:
            assert torch.equal(got_t[k], want_t[k]), (m, k)
        assert stats == want_stats, (m, stats, want_stats)           # n_evals and every other statistic of the call
        assert stats["n_evals"] == want_stats["n_evals"] > 0
        for c, c0 in ((c_s, c0_s), (c_t, c0_t)):
            if c["overflow"] == 0 and c0["overflow"] == 0:            # the screen lists and resolves the same samples
                assert c["resolved"] == c0["resolved"] and c["pending"] == c0["pending"], (m, c, c0)
            assert c["restarts"] <= c["strided"] and c["restarts"] <= c["passes"] - c["strided"], (m, c)
    assert runs["status"] & 24 == 0, runs["status"]                   # bit 3: the screen's guard, bit 4: the slope guard


@torch.no_grad()
def test_passes_fall_on_the_scene():
    runs = _runs("S1")
    for i in (1, 4):   # the sampler alone, the whole tracer
        one, two = runs[ONE_SIDED][i], runs[TWO_SIDED][i]
        assert two["passes"] < one["passes"], (one, two)
        assert two["screened"] < one["screened"], (one, two)


@torch.no_grad()
def test_generalised_net_stays_within_its_allowance_and_restarts():
    runs = _runs("gen0")
    for i in (1, 4):
        one, two = runs[ONE_SIDED][i], runs[TWO_SIDED][i]
        assert two["passes"] <= GEN_ALLOWANCE * one["passes"], (one, two)
    # strided blocks were discarded on the device under both choices (the restart code ran), more of them with the wider stride
    assert runs[ONE_SIDED][1]["restarts"] > 0 and runs[TWO_SIDED][1]["restarts"] > 0, (runs[ONE_SIDED][1], runs[TWO_SIDED][1])


@torch.no_grad()
def test_restart_at_a_blocks_first_sample_ends():
    """A forced slope bound far below the field's slope (L = 1e-3, as tests/test_gpu_sampler_stride.py's guard test forces it): every
    certainly positive sample now `certifies` 15 samples, so blocks are discarded at their first sample all the time and resume
    behind the previous block's last sample.  Results under a wrong bound are not the point (the guard rises, and the network's
    next call marches every sample and gives the stride-1 results): the march must end, and every restart is followed by a stride-1
    pass of its ray, so there are at least as many of those."""
    lib = _lib.load()
    net = HF.build("gen0").cuda()   # a handle of its own: its guards are raised here (parameters bit-identical to _net's)
    n_rays = _sampler_inputs("gen0")[0].shape[0]

    def sample(mode):
        return _sampler("gen0", mode, net)

    want, c0 = sample(OFF)
    assert not _status(net) & 16
    _lib.check(lib.iron_sampler_screen_debug(3, 1e-3))
    try:
        _, c1 = sample(TWO_SIDED)
    finally:
        _lib.check(lib.iron_sampler_screen_debug(3, 0.0))
    print("forced bound", c1, "stride 1", c0)
    assert c1["adaptive"] == 1 and c1["restarts"] > 0, c1
    assert c1["restarts"] <= c1["passes"] - c1["strided"], c1
    # an accepted pass moves its ray's last accepted sample at least 8 forward, and no ray restarts twice in a row
    assert c1["passes"] <= 2 * (HF.N_STEPS // 8) * n_rays, (c1, n_rays)
    assert _status(net) & 16                            # the stride-1 passes behind the restarts saw the slope
    got, c2 = sample(TWO_SIDED)                         # the next call: stride 1
    assert c2["adaptive"] == 0 and c2["strided"] == 0, c2
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    lib.iron_net_force_exact(net.hip_net().handle, 0)   # clears the status
