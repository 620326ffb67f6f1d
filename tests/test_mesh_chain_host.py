"""CPU: the host side the mesh chain shares.  The workspace layouts (csrc/host_util.h's carver, csrc/pair_scan.h's levels) give the
sizes they gave before they were shared, and iron_amd/_args.py refuses and accepts what the modules' own helpers did.  Nothing here
launches a kernel."""
import ctypes

import numpy as np
import pytest
import torch

# recorded from a build of the commit before the layouts moved to the shared carver (and equal to its layout code evaluated by hand)
MC_BYTES = {(2, 2, 2): 1280, (33, 40, 47): 377088, (64, 64, 64): 1589504, (65, 64, 66): 1665536}
FACE_BYTES = {  # n_faces: (bake, bvh, uv)
    1: (2304, 1536, 1280),
    1024: (30720, 127232, 24832),
    1025: (32256, 127744, 25856),
    1048577: (30460672, 130024192, 25216256),
}


def test_workspace_sizes_are_unchanged():
    from iron_amd import _lib, build
    build.build()
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    for dims, want in MC_BYTES.items():
        assert lib.iron_mc_workspace_bytes(*dims, ctypes.byref(n)) == 0 and n.value == want, (dims, n.value)
    for faces, want in FACE_BYTES.items():
        for fn, w in zip((lib.iron_bake_workspace_bytes, lib.iron_bvh_workspace_bytes, lib.iron_uv_workspace_bytes), want):
            assert fn(faces, ctypes.byref(n)) == 0 and n.value == w, (fn.__name__, faces, n.value)


CPU = torch.device("cpu")


def test_device_array_checks_rank_and_trailing_shape_before_the_upload():
    from iron_amd import _args, _lib
    ok = _args.device_array(np.zeros((4, 3)), torch.float32, CPU, "vertices", (3,))
    assert ok.shape == (4, 3) and ok.dtype == torch.float32 and ok.is_contiguous()
    assert _args.device_array(np.zeros((0, 2), np.float32), torch.float32, CPU, "uv", (2,)).shape == (0, 2)
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((4, 3, 1)), np.zeros((3, 4))):
        for strict in (True, False):
            with pytest.raises(_lib.IronError, match=r"vertices must be \[n, 3\]"):
                _args.device_array(bad, torch.float32, torch.device("cuda"), "vertices", (3,), strict=strict)
    with pytest.raises(_lib.IronError, match=r"uv must be \[n, 2\], got \(5, 3\)"):
        _args.device_array(np.zeros((5, 3)), torch.float32, torch.device("cuda"), "uv", (2,))


def test_cpu_tensors_strict_and_lenient():
    from iron_amd import _args, _lib
    x = torch.arange(12.0, dtype=torch.float64).reshape(4, 3)
    with pytest.raises(_lib.IronError, match="^mesh render: CPU tensors"):
        _args.device_array(x, torch.float32, CPU, "vertices", (3,), what="mesh render")
    with pytest.raises(_lib.IronError, match="^mesh distance: CPU tensors"):
        _args.refuse_cpu("mesh distance", np.zeros(3), None, x)
    with pytest.raises(_lib.IronError, match="^mesh distance: CPU tensors"):
        _args.pick_device("mesh distance", np.zeros(3), x)
    _args.refuse_cpu("mesh distance", np.zeros(3), None, [1, 2])  # numpy, None and sequences pass
    # lenient (texture_bake): a CPU tensor is converted, never refused
    y = _args.device_array(x, torch.float32, CPU, "vertices", (3,), strict=False)
    assert y.dtype == torch.float32 and torch.equal(y, x.float())
    assert _args.device_array([[0, 1, 2]], torch.int32, CPU, "faces", (3,), strict=False).dtype == torch.int32
    if torch.cuda.is_available():
        assert _args.pick_device("texture bake", x, strict=False).type == "cuda"
        assert _args.pick_device("mesh distance", np.zeros(3)).type == "cuda"
    else:
        with pytest.raises(Exception) as e:  # torch's own complaint about the missing device, not a refusal of the tensor
            _args.pick_device("texture bake", x, strict=False)
        assert "CPU tensors" not in str(e.value)
        with pytest.raises(_lib.IronError, match="^mesh distance needs a GPU"):
            _args.pick_device("mesh distance", np.zeros(3))


def test_face_array_refuses_non_integer_faces_and_clamps_int64():
    from iron_amd import _args, _lib
    for bad in (np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float64), np.zeros((2, 3), bool)):
        with pytest.raises(_lib.IronError, match="integer vertex indices"):
            _args.face_array(bad, CPU)
    for bad in (np.zeros(3, np.int64), np.zeros((2, 4), np.int64), np.zeros((2, 3, 1), np.int32)):
        with pytest.raises(_lib.IronError, match=r"faces must be \[n, 3\]"):
            _args.face_array(bad, CPU)
    with pytest.raises(_lib.IronError, match="CPU tensors"):
        _args.face_array(torch.zeros((2, 3), dtype=torch.int64), CPU)
    f = _args.face_array(np.array([[0, 1 << 31, -5], [7, (1 << 31) - 1, -1]], dtype=np.int64), CPU)
    assert f.dtype == torch.int32 and f.is_contiguous()
    assert f.tolist() == [[0, (1 << 31) - 1, -1], [7, (1 << 31) - 1, -1]]  # beyond int32 stays out of range, never wraps
    assert _args.face_array(np.array([[0, 1, 2]], dtype=np.int16), CPU).tolist() == [[0, 1, 2]]
