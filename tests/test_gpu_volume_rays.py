"""VolumeDataset's batches (iron_amd/dataset.py over csrc/volume.hip: iron_volume_rays, iron_volume_rays_grid) and the validation
tail (iron_volume_frame_u8) against the reference's expressions (models/dataset.py:271-300, 335-361; render_volume.py:696-729).

Rays: the reference's expressions are evaluated on the CPU in fp64 and in fp32 from the same fp32 matrices.  The allowance is the
project's fp32 floor: 4 x the error of the fp32 CPU evaluation against the fp64 one, and never less than 1 ulp of the
component compared.  The floor is measured once over ALL 35 pixels of the 7 x 5 picture, of which every case's pixels are a subset:
it is a property of the expressions on this camera, not of the pixels a case happened to draw (one ray's fp32 evaluation can land
on the fp64 value by luck).  Colour and mask are exact: u8 / 255 in fp32.

Frames: uint8 output against the reference's numpy expression on the same fp32 inputs; a pixel whose fp64 value lies within 1e-4 of
an integer boundary is flagged from the fp64 side and may differ by 1 (at most 2 % of the pixels are: asserted)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
H, W = 5, 7          # W != H: a swapped index shows
VIEW = 1             # two views, the last is used


def _cameras():
    """Two views: a pinhole with distinct focal lengths and an off-centre principal point; W2C = [R | t] with a generic rotation."""
    Ks, W2Cs = [], []
    for k in range(2):
        K = torch.eye(4, dtype=torch.float64)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 9.3 + k, 8.1 - 0.5 * k, 3.2 + 0.1 * k, 2.4 - 0.2 * k
        ang = torch.tensor([0.3 + 0.4 * k, -0.7 + 0.2 * k, 1.1 - 0.3 * k], dtype=torch.float64)
        cx, cy, cz = torch.cos(ang)
        sx, sy, sz = torch.sin(ang)
        Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
        Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
        Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3] = Rz @ Ry @ Rx
        M[:3, 3] = torch.tensor([0.1 - 0.2 * k, -0.15, 2.6 + 0.3 * k], dtype=torch.float64)
        Ks.append(K.float())
        W2Cs.append(M.float())
    return torch.stack(Ks), torch.stack(W2Cs)


def _dataset(channels=3, mask_channels=0):
    from iron_amd.dataset import VolumeDataset
    gen = torch.Generator().manual_seed(7)
    images = torch.randint(0, 256, (2, H, W, channels), generator=gen, dtype=torch.uint8)
    masks = None if mask_channels == 0 else torch.randint(0, 256, (2, H, W, mask_channels), generator=gen, dtype=torch.uint8)
    Ks, W2Cs = _cameras()
    return VolumeDataset(images=images, Ks=Ks, W2Cs=W2Cs, masks=masks, device=DEV), images, masks


def restated(kinv, pose, x, y, dtype):
    """models/dataset.py:294-299, 336-342 in `dtype` on the CPU: x, y pixel coordinates [n] -> rays_o, rays_d, near, far."""
    kinv, pose = kinv.to(dtype), pose.to(dtype)
    p = torch.stack([x, y, torch.ones_like(y)], dim=-1).to(dtype)
    p = torch.matmul(kinv[None, :3, :3], p[:, :, None]).squeeze(-1)
    rays_v = p / torch.linalg.norm(p, ord=2, dim=-1, keepdim=True)
    rays_v = torch.matmul(pose[None, :3, :3], rays_v[:, :, None]).squeeze(-1)
    rays_o = pose[None, :3, 3].expand(rays_v.shape)
    a = torch.sum(rays_v ** 2, dim=-1, keepdim=True)
    b = 2.0 * torch.sum(rays_o * rays_v, dim=-1, keepdim=True)
    mid = 0.5 * (-b) / a
    return rays_o, rays_v, mid - 1.0, mid + 1.0


_FLOOR = {}


def fp32_floor(kinv, pose):
    """max |fp32 CPU - fp64 CPU| of rays_d, near, far over every pixel of the picture; computed once and left unchanged."""
    if not _FLOOR:
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        x, y = xs.reshape(-1), ys.reshape(-1)
        r64, r32 = restated(kinv, pose, x, y, torch.float64), restated(kinv, pose, x, y, torch.float32)
        for name, a, b in zip(("rays_o", "rays_d", "near", "far"), r32, r64):
            _FLOOR[name] = float((a.double() - b).abs().max())
    return _FLOOR


def check(name, got, want64, floor, label):
    got, want64 = got.detach().cpu().double(), want64.double()
    assert got.shape == want64.shape, (label, name, got.shape, want64.shape)
    ulp = torch.from_numpy(np.spacing(want64.abs().numpy().astype(np.float32)).astype(np.float64))
    tol = torch.maximum(torch.full_like(want64, 4.0 * floor[name]), ulp)
    err = (got - want64).abs()
    print("%-28s %-7s max err %.2e  fp32 floor %.2e  tol %.2e .. %.2e" % (label, name, float(err.max()), floor[name], float(tol.min()),
                                                                           float(tol.max())))
    assert bool((err <= tol).all()), (label, name, float(err.max()))


@pytest.mark.parametrize("channels, mask_channels", [(3, 0), (4, 1), (3, 3)])
@pytest.mark.parametrize("batch", [1, 64, 65, 130])
def test_random_mode(batch, channels, mask_channels):
    ds, images, masks = _dataset(channels, mask_channels)
    assert (ds.n_images, ds.H, ds.W) == (2, H, W) and ds.images_u8.dtype == torch.uint8
    gen = torch.Generator().manual_seed(100 + batch)
    px = torch.cat([torch.tensor([0, W - 1, 0, W - 1]), torch.randint(0, W, (batch,), generator=gen)])
    py = torch.cat([torch.tensor([0, 0, H - 1, H - 1]), torch.randint(0, H, (batch,), generator=gen)])
    data, near, far = ds.rays_at_pixels(VIEW, px.to(DEV), py.to(DEV))
    torch.cuda.synchronize()
    n = batch + 4
    assert tuple(data.shape) == (n, 10) and tuple(near.shape) == (n, 1) and tuple(far.shape) == (n, 1)
    data = data.cpu()
    # colour and mask: exactly u8 / 255
    assert torch.equal(data[:, 6:9], images[VIEW][(py, px)][:, :3].to(torch.float32) / 255.0)
    want_mask = torch.ones(n) if masks is None else masks[VIEW][(py, px)][:, 0].to(torch.float32) / 255.0
    assert torch.equal(data[:, 9], want_mask)
    kinv, pose = ds.intrinsics_all_inv[VIEW].cpu(), ds.pose_all[VIEW].cpu()
    assert torch.allclose(kinv, torch.inverse(_cameras()[0][VIEW]), rtol=1e-5, atol=1e-7)
    floor = fp32_floor(kinv, pose)
    o64, d64, near64, far64 = restated(kinv, pose, px, py, torch.float64)
    label = "B=%d C=%d Cm=%d" % (batch, channels, mask_channels)
    assert torch.equal(data[:, :3], pose[None, :3, 3].expand(n, 3)), "rays_o is the pose's translation"
    check("rays_d", data[:, 3:6], d64, floor, label)
    check("near", near, near64, floor, label)
    check("far", far, far64, floor, label)
    # near_far_from_sphere on the batch's own rays: the same mid -+ 1
    near2, far2 = ds.near_far_from_sphere(data[:, :3].to(DEV), data[:, 3:6].to(DEV))
    check("near", near2, near64, floor, label + " (torch)")
    check("far", far2, far64, floor, label + " (torch)")


def test_random_rays_come_from_the_given_generator():
    ds, images, _ = _dataset()
    a = ds.gen_random_rays_at(VIEW, 65, generator=torch.Generator(device=DEV).manual_seed(3))
    g = torch.Generator(device=DEV).manual_seed(3)
    b = ds.gen_random_rays_at(torch.tensor(VIEW), 65, generator=g)       # image_perm[...] hands a 0-d tensor over
    c = ds.gen_random_rays_at(VIEW, 65, generator=g)
    assert tuple(a.shape) == (65, 10) and torch.equal(a, b) and not torch.equal(a, c)
    g = torch.Generator(device=DEV).manual_seed(3)
    px = torch.randint(low=0, high=W, size=[65], device=DEV, generator=g).cpu()
    py = torch.randint(low=0, high=H, size=[65], device=DEV, generator=g).cpu()
    assert torch.equal(a[:, 6:9].cpu(), images[VIEW][(py, px)].to(torch.float32) / 255.0)
    from iron_amd import _lib
    with pytest.raises(_lib.IronError):
        ds.gen_random_rays_at(2, 4)


def test_a_pixel_outside_the_picture_is_not_read():
    ds, _, _ = _dataset()
    data, near, far = ds.rays_at_pixels(0, torch.tensor([W, 1, -1], device=DEV), torch.tensor([0, H, 2], device=DEV))
    assert bool(torch.isnan(data[:, 6:]).all()) and bool(torch.isfinite(data[:, :6]).all()) and bool(torch.isfinite(near).all())


@pytest.mark.parametrize("level", [1, 2, 3])
def test_grid_mode(level):
    ds, _, _ = _dataset()
    rays_o, rays_d = ds.gen_rays_at(VIEW, resolution_level=level)
    torch.cuda.synchronize()
    rows, cols = H // level, W // level
    assert tuple(rays_o.shape) == (rows, cols, 3) and tuple(rays_d.shape) == (rows, cols, 3)     # the reference's transpose(0, 1)
    kinv, pose = ds.intrinsics_all_inv[VIEW].cpu(), ds.pose_all[VIEW].cpu()
    floor = fp32_floor(kinv, pose)
    tx, ty = torch.linspace(0, W - 1, cols), torch.linspace(0, H - 1, rows)                      # models/dataset.py:276-278
    pixels_x, pixels_y = torch.meshgrid(tx, ty, indexing="ij")                                   # [W', H']
    o64, d64, near64, far64 = restated(kinv, pose, pixels_x.reshape(-1).double(), pixels_y.reshape(-1).double(), torch.float64)
    d64 = d64.reshape(cols, rows, 3).transpose(0, 1)
    assert torch.equal(rays_o.cpu(), pose[None, None, :3, 3].expand(rows, cols, 3))
    check("rays_d", rays_d, d64, floor, "grid l=%d" % level)
    near, far = ds.near_far_from_sphere(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3))
    check("near", near, near64.reshape(cols, rows, 1).transpose(0, 1).reshape(-1, 1), floor, "grid l=%d" % level)
    check("far", far, far64.reshape(cols, rows, 1).transpose(0, 1).reshape(-1, 1), floor, "grid l=%d" % level)
    # the corner rays of the grid are the corner rays of the random mode
    if rows > 1:
        corner, _, _ = ds.rays_at_pixels(VIEW, torch.tensor([0, W - 1], device=DEV), torch.tensor([H - 1, 0], device=DEV))
        assert torch.equal(rays_d[rows - 1, 0], corner[0, 3:6]) and torch.equal(rays_d[0, cols - 1], corner[1, 3:6])


def test_image_at():
    ds, images, _ = _dataset(channels=4)
    full = ds.image_at(VIEW, 1)
    assert full.dtype == np.uint8 and np.array_equal(full, images[VIEW][:, :, :3].numpy())
    half = ds.image_at(VIEW, 2)
    assert half.dtype == np.uint8 and half.shape == (H // 2, W // 2, 3)
    assert list(ds.object_bbox_min) == [-1.01] * 3 and list(ds.object_bbox_max) == [1.01] * 3


# ---- iron_volume_frame_u8 -----------------------------------------------------------------------------------------------------------
N_RAYS, M, M_OUT, OFFSET, FRAME = 130, 5, 3, 37, 200


def _frame_inputs():
    gen = torch.Generator().manual_seed(23)
    color = torch.rand(N_RAYS, 3, generator=gen) * 1.2 - 0.1                       # some below 0 and above 1: both clips
    gradients = torch.randn(N_RAYS, M, 3, generator=gen)
    gradients = gradients / gradients.norm(dim=-1, keepdim=True) * (1.0 + 0.2 * torch.randn(N_RAYS, M, 1, generator=gen))
    weights = torch.rand(N_RAYS, M + M_OUT, generator=gen)
    weights = weights / weights.sum(dim=-1, keepdim=True) * torch.rand(N_RAYS, 1, generator=gen) * 1.3
    inside = (torch.rand(N_RAYS, M, generator=gen) < 0.7).to(torch.float32)        # partly 0
    rot = torch.linalg.inv(_cameras()[1][0][:3, :3])
    return color, gradients, weights, inside, rot.contiguous()


def _frame_reference(color, gradients, weights, inside, rot, dtype):
    """render_volume.py:700-703, 712, 722-729 in numpy; -> the two pictures before .clip(0, 255).astype('uint8'), [n, 3] each."""
    c, g, w, i, r = (t.numpy().astype(dtype) for t in (color, gradients, weights, inside, rot))
    normals = g * w[:, :M, None]
    normals = normals * i[..., None]
    normals = normals.sum(axis=1)
    img_fine = c * 256
    normal_img = np.matmul(r[None, :, :], normals[:, :, None]).reshape(-1, 3) * 128 + 128
    return img_fine, normal_img


@pytest.mark.parametrize("with_inside", [True, False])
def test_frame_u8(with_inside):
    from iron_amd import _lib
    color, gradients, weights, inside, rot = _frame_inputs()
    if not with_inside:
        inside = torch.ones_like(inside)
    assert 0.1 < float((inside == 0).float().mean()) < 0.5 or not with_inside
    rgb = torch.full((FRAME, 3), 77, dtype=torch.uint8, device=DEV)
    nrm = torch.full((FRAME, 3), 77, dtype=torch.uint8, device=DEV)
    dc, dg, dw, di, dr = (t.to(DEV).contiguous() for t in (color, gradients, weights, inside, rot))
    _lib.check(_lib.load().iron_volume_frame_u8(dc.data_ptr(), dg.data_ptr(), dw.data_ptr(), di.data_ptr() if with_inside else None,
                                                dr.data_ptr(), N_RAYS, M, M + M_OUT, OFFSET, FRAME, rgb.data_ptr(), nrm.data_ptr(),
                                                _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    rgb, nrm = rgb.cpu().numpy(), nrm.cpu().numpy()
    for frame in (rgb, nrm):   # written at the ray offset, and nowhere else
        assert (frame[:OFFSET] == 77).all() and (frame[OFFSET + N_RAYS:] == 77).all()
    img32, nrm32 = _frame_reference(color, gradients, weights, inside, rot, np.float32)
    img64, nrm64 = _frame_reference(color, gradients, weights, inside, rot, np.float64)
    for name, got, w32, w64 in (("colour", rgb[OFFSET:OFFSET + N_RAYS], img32, img64), ("normal", nrm[OFFSET:OFFSET + N_RAYS], nrm32, nrm64)):
        want = w32.clip(0, 255).astype("uint8")
        flagged = np.abs(w64 - np.rint(w64)) < 1e-4                      # within 1e-4 of an integer boundary, seen from fp64 (before the clip)
        share = float(flagged.mean())
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print("frame %-6s inside=%s: flagged %.2f %%, differing pixels %d (all flagged: %s)" % (name, with_inside, 100 * share, int((diff > 0).sum()),
                                                                                               bool(flagged[diff > 0].all())))
        assert share <= 0.02, (name, share)
        assert (diff[~flagged] == 0).all(), name
        assert (diff[flagged] <= 1).all(), name
    assert (img64 <= 0).any() and (img64 >= 255).any(), "the inputs reach both clips"
