"""FusedAdam (iron_amd/optim.py over csrc/optim.hip: iron_adam_multi) against torch.optim.Adam.

The reference is torch.optim.Adam in fp64 on the CPU fed the same fp32 gradients (upcast).  The floor of a tensor is the largest
elementwise error of torch.optim.Adam in fp32 (CPU, same inputs) against that fp64 run; FusedAdam is allowed, element by element,
2 x that floor (an equally valid rounding order: FMA contraction, rsqrt against sqrt + divide) plus one fp32 ulp of the element's
own magnitude (the final rounding, where the floor of a tiny tensor happens to be small).  The same rule holds for exp_avg and
exp_avg_sq.  Shapes: the smallest at which chunking and vector ends can go wrong."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STEPS = 5
LR_A, LR_B = 1e-2, 1e-4
N_ONES = 300          # one-element tensors: more than any single launch table (IRON_ADAM_MAX_TENSORS)
N_OFFSET = 1031       # the parameter at storage offset 1: whole float4s and a tail on the scalar path


def _shapes():
    from iron_amd import _lib
    return [(1,), (3,), (63,), (64,), (65,), (257, 39), (256, 256), (_lib.IRON_ADAM_CHUNK + 1,), (N_OFFSET,)]


def _grad(shape, gen):
    """fp32 gradients of magnitude 1e-8 .. 1, either sign, about one in ten exactly zero."""
    mag = torch.pow(10.0, -8.0 * torch.rand(shape, generator=gen))
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    keep = (torch.rand(shape, generator=gen) >= 0.1).float()
    return (mag * sign * keep).float()


@pytest.fixture(scope="module")
def problem():
    gen = torch.Generator().manual_seed(11)
    shapes = _shapes() + [(1,)] * N_ONES
    p0 = [(0.1 * torch.randn(s, generator=gen)).float() for s in shapes]
    grads = [[_grad(s, gen) for s in shapes] for _ in range(STEPS + 1)]   # the last set is for the round-trip step
    flat = torch.cat([g.reshape(-1) for g in grads[0]]).abs()
    assert bool((flat == 0).any()) and float(flat[flat > 0].min()) < 1e-7 and float(flat.max()) > 0.5
    return {"shapes": shapes, "p0": p0, "grads": grads, "n_a": len(_shapes())}


def _groups(params, n_a):
    return [{"params": params[:n_a], "lr": LR_A}, {"params": params[n_a:], "lr": LR_B}]


def _device_params(problem):
    params = []
    for i, v in enumerate(problem["p0"]):
        if tuple(v.shape) == (N_OFFSET,):
            base = torch.zeros(N_OFFSET + 1, device=DEV)
            base[1:] = v.to(DEV)
            p = torch.nn.Parameter(base[1:])
            assert p.storage_offset() == 1 and p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(v.to(DEV).clone())
        params.append(p)
    return params


def _run_fused(problem, steps=STEPS, zero_grads=False):
    from iron_amd.optim import FusedAdam
    params = _device_params(problem)
    opt = FusedAdam(_groups(params, problem["n_a"]), zero_grads=zero_grads)
    for s in range(steps):
        for p, g in zip(params, problem["grads"][s]):
            p.grad = g.to(DEV)
        opt.step()
    torch.cuda.synchronize()
    return params, opt


def _run_torch(problem, dtype, steps=STEPS):
    params = [torch.nn.Parameter(v.to(dtype).clone()) for v in problem["p0"]]
    opt = torch.optim.Adam(_groups(params, problem["n_a"]))
    for s in range(steps):
        for p, g in zip(params, problem["grads"][s]):
            p.grad = g.to(dtype)
        opt.step()
    return params, opt


@pytest.fixture(scope="module")
def runs(problem):
    return {"fused": _run_fused(problem), "ref64": _run_torch(problem, torch.float64), "t32": _run_torch(problem, torch.float32)}


def _ulp(ref64):
    return torch.from_numpy(np.asarray(np.spacing(np.abs(ref64.detach().float().cpu().numpy())), dtype=np.float64))


def _check(name, ours, ref64, t32, report):
    """|ours - ref64| <= 2 max|t32 - ref64| + ulp(|ref64|), element by element."""
    ours, ref64, t32 = ours.detach().double().cpu(), ref64.detach().double(), t32.detach().double()
    floor = float((t32 - ref64).abs().max())
    err = (ours - ref64).abs()
    allow = 2.0 * floor + _ulp(ref64)
    scale = float(_ulp(ref64.abs().max()))
    report.append((name, floor / scale, float(err.max()) / scale))
    bad = err > allow
    assert not bool(bad.any()), "%s: %d elements beyond 2 x floor + 1 ulp (floor %.3e, worst error %.3e, allowance there %.3e)" % (
        name, int(bad.sum()), floor, float(err[bad].max()), float(allow[bad][err[bad].argmax()]))


def test_five_steps_within_twice_the_fp32_floor_of_torch_adam(problem, runs):
    (pf, of), (p64, o64), (p32, o32) = runs["fused"], runs["ref64"], runs["t32"]
    report = []
    for i, shape in enumerate(problem["shapes"]):
        tag = "x".join(map(str, shape)) + ("@1" if shape == (N_OFFSET,) else "")
        _check("param[%d] %s" % (i, tag), pf[i], p64[i], p32[i], report)
        for key in ("exp_avg", "exp_avg_sq"):
            _check("%s[%d] %s" % (key, i, tag), of.state[pf[i]][key], o64.state[p64[i]][key], o32.state[p32[i]][key], report)
        assert float(of.state[pf[i]]["step"]) == STEPS
    n_a = problem["n_a"]
    for name, floor, err in report[:3 * n_a]:
        print("%-28s floor %.3f ulp  FusedAdam %.3f ulp (of the tensor's largest element)" % (name, floor, err))
    ones = report[3 * n_a:]   # an element that ends next to zero has a tiny ulp of its own: count how often the runs differ instead
    print("%d one-element tensors x 3 quantities: FusedAdam differs from torch's fp32 run in %d, beyond 1 ulp of the element in %d" % (
        N_ONES, sum(abs(r[1] - r[2]) > 0 for r in ones), sum(abs(r[1] - r[2]) > 1.0 for r in ones)))
    v = of.state[pf[6]]["exp_avg_sq"].double().cpu()
    v64, v32 = o64.state[p64[6]]["exp_avg_sq"], o32.state[p32[6]]["exp_avg_sq"].double()
    nz = v64 > 0
    print("exp_avg_sq 256x256 relative to fp64: torch fp32 %.2e, FusedAdam %.2e" % (
        float(((v32 - v64).abs()[nz] / v64[nz]).max()), float(((v - v64).abs()[nz] / v64[nz]).max())))


def test_two_runs_are_bitwise_equal(problem, runs):
    pa, oa = runs["fused"]
    pb, ob = _run_fused(problem)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])


def test_in_kernel_zeroing_leaves_every_gradient_exactly_zero_and_the_same_update(problem, runs):
    from iron_amd.optim import FusedAdam
    params = _device_params(problem)
    opt = FusedAdam(_groups(params, problem["n_a"]), zero_grads=True)
    for p, g in zip(params, problem["grads"][0]):
        p.grad = g.to(DEV)
    opt.step()
    plain, _ = _run_fused(problem, steps=1)
    for p, q in zip(params, plain):
        assert p.grad is not None and int(torch.count_nonzero(p.grad)) == 0
        assert torch.equal(p, q)


def test_a_parameter_without_gradient_keeps_its_bits_and_its_step_and_versions_advance(problem):
    from iron_amd.optim import FusedAdam
    params = _device_params(problem)[:9]
    idle = torch.nn.Parameter(torch.randn(77, device=DEV))
    before = idle.detach().clone()
    opt = FusedAdam([{"params": params + [idle], "lr": LR_A}])
    for s in range(2):
        for p, g in zip(params, problem["grads"][s]):
            p.grad = g.to(DEV)
        versions = [p._version for p in params] + [idle._version]
        opt.step()
        assert all(p._version > v for p, v in zip(params, versions))
        assert idle._version == versions[-1]
    assert torch.equal(idle, before) and len(opt.state[idle]) == 0
    assert all(float(opt.state[p]["step"]) == 2 for p in params)
    # a gradient arrives later: this parameter's own count starts at 1 while the others go on to 3
    idle.grad = torch.full_like(idle, 0.5)
    for p, g in zip(params, problem["grads"][2]):
        p.grad = g.to(DEV)
    opt.step()
    assert float(opt.state[idle]["step"]) == 1 and float(opt.state[params[0]]["step"]) == 3
    want = before - LR_A * torch.sign(idle.grad)   # step 1 of Adam: m / sqrt(v) = sign(g) up to eps
    assert float((idle.detach() - want).abs().max()) < 1e-6


def test_state_dict_round_trips_through_torch_adam(problem, runs):
    """FusedAdam -> torch.optim.Adam and back, in torch's own layout; then one more step on each, held to the allowance."""
    from iron_amd.optim import FusedAdam
    pf, of = runs["fused"]
    sd = of.state_dict()
    n_a, extra = problem["n_a"], problem["grads"][STEPS]
    ref_keys = set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])
    assert set(sd["param_groups"][0]) == ref_keys and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}

    def clones():
        return [torch.nn.Parameter(p.detach().clone()) for p in pf]
    pt, pg = clones(), clones()
    torch_opt = torch.optim.Adam(_groups(pt, n_a))
    # load_state_dict keeps the tensors it is given (it copies only to cast or move them): hand every optimiser its own copies
    torch_opt.load_state_dict(copy.deepcopy(sd))                         # ours into torch's
    fused_opt = FusedAdam(_groups(pg, n_a))
    fused_opt.load_state_dict(copy.deepcopy(torch_opt.state_dict()))     # and torch's into ours
    assert [g["lr"] for g in fused_opt.param_groups] == [LR_A, LR_B]
    for params, opt in ((pt, torch_opt), (pg, fused_opt)):
        for p, g in zip(params, extra):
            p.grad = g.to(DEV)
        opt.step()
    torch.cuda.synchronize()
    # the sixth step of the fp64 and the fp32 CPU runs gives the reference and the floor
    p64, _ = _run_torch(problem, torch.float64, steps=STEPS + 1)
    p32, _ = _run_torch(problem, torch.float32, steps=STEPS + 1)
    report = []
    for i in range(len(pf)):
        assert float(fused_opt.state[pg[i]]["step"]) == STEPS + 1
        _check("round trip param[%d]" % i, pg[i], p64[i], p32[i], report)
        floor = float((p32[i].detach().double() - p64[i].detach()).abs().max())
        gap = (pg[i].detach().double() - pt[i].detach().double()).abs().cpu()
        assert bool((gap <= 2.0 * floor + _ulp(p64[i])).all()), i
    print("round trip: largest FusedAdam error %.3f ulp, largest floor %.3f ulp" % (max(r[2] for r in report), max(r[1] for r in report)))


def test_render_after_a_step_equals_fresh_networks_with_the_stepped_state():
    """The packed device copies (SDFNetwork.hip_net, the material handles) and host_light() follow the version counters FusedAdam
    bumps: no invalidate() call, and the render is the one of freshly built networks loaded with the stepped state_dict."""
    from iron_amd import scenes
    from iron_amd.optim import FusedAdam
    from iron_amd.raytracer import Camera, RayTracer, render_camera
    from iron_amd.renderer_ggx import GGXColocatedRenderer
    from iron_amd.rendering_func import make_render_fn
    fn = make_render_fn(GGXColocatedRenderer(use_cuda=True))
    K, W2C = scenes.fixture_camera_matrices(512, 512)
    cam = Camera(512, 512, K.to(DEV), W2C.to(DEV)).crop_region(24, 24, ul_corner=(244, 244))[0]

    def render(nets):
        with torch.no_grad():
            return render_camera(cam, nets["sdf_network"], RayTracer(), nets, fn, fill_holes=False, handle_edges=False, is_training=False)

    nets = {k: m.to(DEV) for k, m in scenes.build_networks("S0", seed=0).items()}
    first = render(nets)   # packs the device copies and reads the light
    assert bool(first["convergent_mask"].any())
    params = [p for m in nets.values() for p in m.parameters()]
    gen = torch.Generator(device=DEV).manual_seed(5)
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=gen)
    FusedAdam(params, lr=1e-3).step()
    stepped = render(nets)
    fresh = {k: m.to(DEV) for k, m in scenes.build_networks("S0", seed=3).items()}
    for k in fresh:
        fresh[k].load_state_dict(nets[k].state_dict())
    again = render(fresh)
    assert not torch.equal(stepped["color"], first["color"])
    assert torch.equal(stepped["convergent_mask"], again["convergent_mask"]) and torch.equal(stepped["color"], again["color"])
    assert nets["point_light_network"].host_light() == float(nets["point_light_network"].light.detach())


def test_bad_inputs_are_refused():
    from iron_amd import _lib
    from iron_amd.optim import FusedAdam
    lib = _lib.load_train()
    buf = torch.zeros(4, 8, device=DEV)
    for data in (torch.zeros(4), torch.zeros(4, device=DEV).double(), buf.t()):   # CPU, not fp32, not contiguous
        p = torch.nn.Parameter(data)
        p.grad = torch.zeros_like(p)
        with pytest.raises(_lib.IronError):
            FusedAdam([p]).step()
        assert int(torch.count_nonzero(p.detach())) == 0
    # torch refuses to attach most mismatched gradients to a leaf itself; the optimiser's own check is what step() runs on each pair
    p = torch.nn.Parameter(torch.ones(8, 4, device=DEV))
    FusedAdam._check_grad(p, torch.zeros(8, 4, device=DEV))
    for bad in (torch.zeros(4, 8, device=DEV), torch.zeros(8, 4, device=DEV).double(), torch.zeros(8, 4), buf.t()):
        with pytest.raises(_lib.IronError):
            FusedAdam._check_grad(p, bad)
    # the C entry, on the host: nothing is enqueued for a refused table
    t = (_lib.iron_adam_tensor * 1)()
    ok = torch.zeros(4, device=DEV)
    t[0].param = t[0].grad = t[0].exp_avg = t[0].exp_avg_sq = ok.data_ptr()
    t[0].numel, t[0].step, t[0].lr = 4, 1, 1e-3
    stream = _lib.stream_ptr(DEV)
    t[0].step = 0
    assert lib.iron_adam_multi(t, 1, 0.9, 0.999, 1e-8, 0, stream) == _lib.IRON_ERR_BAD_ARG
    t[0].step, t[0].numel = 1, -1
    assert lib.iron_adam_multi(t, 1, 0.9, 0.999, 1e-8, 0, stream) == _lib.IRON_ERR_BAD_ARG
    t[0].numel, t[0].grad = 4, None
    assert lib.iron_adam_multi(t, 1, 0.9, 0.999, 1e-8, 0, stream) == _lib.IRON_ERR_BAD_ARG
    assert lib.iron_adam_multi(None, 1, 0.9, 0.999, 1e-8, 0, stream) == _lib.IRON_ERR_BAD_ARG
    assert lib.iron_adam_multi(t, -1, 0.9, 0.999, 1e-8, 0, stream) == _lib.IRON_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ok)) == 0
