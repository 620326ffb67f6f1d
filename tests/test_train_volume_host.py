"""Host-side checks of the stage-1 trainer (no GPU): the learning-rate schedule, the cosine annealing ratio, checkpoint names, the
command line, the agreement of both headers with the ctypes signatures of the entries csrc/volume.hip and csrc/volume_loss.hip
add, their argument checks, and write_ply_mesh."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ENTRIES = ("iron_volume_rays", "iron_volume_rays_grid", "iron_volume_frame_u8")
TRAIN_ENTRIES = ("iron_volume_loss_workspace_bytes", "iron_volume_loss", "iron_volume_loss_backward")


@pytest.mark.parametrize("step", [0, 2500, 5000, 52500, 100001])
def test_learning_rate_factor_against_the_formula_in_fp64(step):
    """render_volume.py:554-560 with womask_iron.conf's values."""
    import math
    from iron_amd.train_volume import learning_factor
    warm, end, alpha = 5000.0, 100001, 0.05
    if step < warm:
        want = step / warm
    else:
        want = (math.cos(math.pi * (step - warm) / (end - warm)) + 1.0) * 0.5 * (1 - alpha) + alpha
    got = learning_factor(step, warm, end, alpha)
    assert type(got) is float and abs(got - want) <= 4 * np.finfo(np.float64).eps * max(abs(want), 1.0), (step, got, want)
    assert {0: got == 0.0, 2500: got == 0.5, 5000: got == 1.0, 100001: abs(got - alpha) < 1e-15}.get(step, 0.05 < got < 1.0)


def test_learning_rate_without_warm_up_and_cos_anneal_ratio():
    from iron_amd.train_volume import cos_anneal_ratio, learning_factor
    assert learning_factor(0, 0.0, 100, 1.0) == 1.0 and learning_factor(57, 0.0, 100, 1.0) == 1.0   # alpha = 1: a constant rate
    assert learning_factor(0, 0.0, 100, 0.05) == 1.0
    assert cos_anneal_ratio(0, 50000.0) == 0.0 and cos_anneal_ratio(12500, 50000.0) == 0.25
    assert cos_anneal_ratio(50000, 50000.0) == 1.0 and cos_anneal_ratio(70000, 50000.0) == 1.0
    assert cos_anneal_ratio(0, 0.0) == 1.0 and cos_anneal_ratio(123, 0.0) == 1.0                  # anneal_end = 0: always 1
    assert type(cos_anneal_ratio(3, 7.0)) is float


def test_checkpoint_file_names(tmp_path):
    from iron_amd.train_volume import checkpoint_name, latest_checkpoint, state_name
    assert checkpoint_name(2) == "ckpt_000002.pth" and checkpoint_name(100000) == "ckpt_100000.pth" and checkpoint_name(1234567) == "ckpt_1234567.pth"
    assert state_name(10000) == "state_010000.pth"
    assert latest_checkpoint(str(tmp_path)) is None
    os.makedirs(tmp_path / "checkpoints")
    for name in ("ckpt_000002.pth", "ckpt_010000.pth", "ckpt_000500.pth", "state_010000.pth", "state_090000.pth", "notes.txt"):
        (tmp_path / "checkpoints" / name).write_bytes(b"")
    assert latest_checkpoint(str(tmp_path)) == "ckpt_010000.pth"


def test_argument_parsing_carries_the_reference_names_and_defaults():
    """render_volume.py:859-865."""
    from iron_amd.train_volume import config_parser
    a = config_parser().parse_args([])
    want = {"conf": "./confs/base.conf", "mode": "train", "mcube_threshold": 0.0, "is_continue": False, "gpu": 0, "case": "",
            "seed": 0, "optimizer": "fused", "tail": "hip"}
    for k, v in want.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    b = config_parser().parse_args("--conf C --mode validate_mesh --mcube_threshold 0.5 --is_continue --gpu 1 --case X --seed 3 "
                                   "--optimizer torch --tail torch".split())
    assert (b.conf, b.mode, b.mcube_threshold, b.is_continue, b.gpu, b.case, b.seed, b.optimizer, b.tail) == \
        ("C", "validate_mesh", 0.5, True, 1, "X", 3, "torch", "torch")
    for bad in (["--tail", "triton"], ["--optimizer", "sgd"], ["--mode", "interpolate_0_1"]):
        with pytest.raises(SystemExit):
            config_parser().parse_args(bad)


def _prototypes(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"^\s*(size_t|int)\s+(iron_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M | re.S):
        protos[name] = (ret, [" ".join(a.split()) for a in args.split(",")])
    return protos, hdr


def _ctype_of(decl):
    d = decl.replace("const ", "").strip()
    if "*" in d:
        return "struct" if d.split("*")[0].strip() == "iron_volume_loss_args" else C.c_void_p
    return {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "float": C.c_float, "size_t": C.c_size_t,
            "int": C.c_int}[d.rsplit(" ", 1)[0]]


def test_headers_and_ctypes_agree_on_the_new_entries():
    from iron_amd import _lib
    for header, table, names in (("iron_hip.h", _lib.SYMBOLS, HIP_ENTRIES), ("iron_train.h", _lib.TRAIN_SYMBOLS, TRAIN_ENTRIES)):
        protos, _ = _prototypes(header)
        for name in names:
            assert name in protos, "%s is not declared in include/%s" % (name, header)
            ret, args = protos[name]
            res, argtypes = table[name]
            assert res is {"int": C.c_int, "size_t": C.c_size_t}[ret], name
            assert len(args) == len(argtypes), (name, args)
            for decl, ct in zip(args, argtypes):
                want = _ctype_of(decl)
                assert ct is (C.POINTER(_lib.iron_volume_loss_args) if want == "struct" else want), (name, decl, ct)
    _, hdr = _prototypes("iron_train.h")
    body = re.search(r"typedef struct iron_volume_loss_args \{(.*?)\}\s*iron_volume_loss_args;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            first, *rest = decl.split(",")
            typ, n0 = first.rsplit(" ", 1)
            fields += [(typ + ("*" if n.startswith("*") else ""), n.lstrip("*")) for n in [n0] + [r.strip() for r in rest]]
    cfields = _lib.iron_volume_loss_args._fields_
    assert [n for _, n in fields] == [n for n, _ in cfields]
    for (typ, n), (_, ct) in zip(fields, cfields):
        assert ct is _ctype_of(typ if "*" in typ else typ + " x"), n
    assert C.sizeof(_lib.iron_volume_loss_args) == 96
    enum = re.search(r"enum \{\s*IRON_VL_LOSS(.*?)\};", hdr, flags=re.S).group(0)
    idx = {k: int(v) for k, v in re.findall(r"IRON_VL_([A-Z_]+) = (\d+)", enum)}
    assert idx["RECORD"] == len(_lib.VOLUME_LOSS_RECORD) == 8
    assert [idx[k] for k in ("LOSS", "COLOR", "EIKONAL", "MASK", "PSNR", "CDF", "WEIGHT_MAX", "MASK_SUM")] == list(range(8))
    assert _lib.VOLUME_LOSS_RECORD == ("loss", "color_fine_loss", "eikonal_loss", "mask_loss", "psnr", "cdf", "weight_max", "mask_sum")


def test_the_libraries_export_the_entries_and_refuse_bad_arguments_before_any_launch():
    from iron_amd import _lib, build
    build.build()
    assert "volume.hip" in build.SOURCES and "volume_loss.hip" in build.TRAIN_SOURCES
    lib, train = _lib.load(), _lib.load_train()
    for name in HIP_ENTRIES:
        assert hasattr(lib, name), name
    for name in TRAIN_ENTRIES:
        assert hasattr(train, name), name
    BAD = _lib.IRON_ERR_BAD_ARG
    one = 8   # a non-null address that is never dereferenced: the checks below all fail on the host
    # iron_volume_rays: null picture / matrices / outputs, c < 3, a negative count
    assert lib.iron_volume_rays(None, 5, 7, 3, None, 0, one, one, one, one, 4, one, one, one, None) == BAD
    assert lib.iron_volume_rays(one, 5, 7, 3, None, 0, None, one, one, one, 4, one, one, one, None) == BAD
    assert lib.iron_volume_rays(one, 5, 7, 3, None, 0, one, one, None, one, 4, one, one, one, None) == BAD
    assert lib.iron_volume_rays(one, 5, 7, 3, None, 0, one, one, one, one, 4, None, one, one, None) == BAD
    assert lib.iron_volume_rays(one, 5, 7, 2, None, 0, one, one, one, one, 4, one, one, one, None) == BAD
    assert lib.iron_volume_rays(one, 5, 7, 3, one, 0, one, one, one, one, 4, one, one, one, None) == BAD
    assert lib.iron_volume_rays(one, 5, 7, 3, None, 0, one, one, one, one, -1, one, one, one, None) == BAD
    assert lib.iron_volume_rays(one, 5, 7, 3, None, 0, one, one, None, None, 0, None, None, None, None) == 0       # an empty batch is a no-op
    assert lib.iron_volume_rays_grid(None, one, one, one, 2, 2, one, one, None) == BAD
    assert lib.iron_volume_rays_grid(one, one, None, one, 2, 2, one, one, None) == BAD
    assert lib.iron_volume_rays_grid(one, one, one, one, -1, 2, one, one, None) == BAD
    assert lib.iron_volume_rays_grid(one, one, one, one, 2, 2, None, one, None) == BAD
    # iron_volume_frame_u8: no frame at all, a null input of a requested frame, mw < m, a batch that leaves the frame
    assert lib.iron_volume_frame_u8(one, one, one, None, one, 4, 5, 8, 0, 4, None, None, None) == BAD
    assert lib.iron_volume_frame_u8(None, one, one, None, one, 4, 5, 8, 0, 4, one, None, None) == BAD
    assert lib.iron_volume_frame_u8(one, None, one, None, one, 4, 5, 8, 0, 4, None, one, None) == BAD
    assert lib.iron_volume_frame_u8(one, one, one, None, None, 4, 5, 8, 0, 4, None, one, None) == BAD
    assert lib.iron_volume_frame_u8(one, one, one, None, one, 4, 5, 4, 0, 4, one, one, None) == BAD
    assert lib.iron_volume_frame_u8(one, one, one, None, one, 4, 5, 8, 1, 4, one, one, None) == BAD
    assert lib.iron_volume_frame_u8(one, one, one, None, one, -4, 5, 8, 0, 4, one, one, None) == BAD
    # iron_volume_loss
    a = _lib.iron_volume_loss_args()
    assert train.iron_volume_loss(a, one, one, one, one, 1 << 20, None) == BAD                       # everything null, b = 0
    for k in ("color_fine", "true_rgb", "mask", "weight_sum", "weight_max", "cdf_fine", "gradient_error"):
        setattr(a, k, one)
    a.b, a.rgb_stride, a.mask_stride, a.cdf_stride, a.igr_weight, a.mask_weight = 4, 10, 10, 128, 0.1, 0.1
    assert train.iron_volume_loss(a, None, one, one, one, 1 << 20, None) == BAD
    assert train.iron_volume_loss(a, one, one, one, None, 1 << 20, None) == BAD
    assert train.iron_volume_loss(a, one, one, one, one, 8, None) == -5                             # IRON_ERR_WORKSPACE: 6 doubles needed
    assert train.iron_volume_loss_backward(a, None, one, one, one, one, None) == BAD
    for k, v in (("b", -1), ("b", 0), ("rgb_stride", 2), ("mask_stride", 0), ("cdf_stride", 0)):
        keep = getattr(a, k)
        setattr(a, k, v)
        assert train.iron_volume_loss(a, one, one, one, one, 1 << 20, None) == BAD, k
        assert train.iron_volume_loss_backward(a, one, one, one, one, one, None) == BAD, k
        setattr(a, k, keep)
    a.mask = None                                                                                  # allowed only with mask_weight = 0
    assert train.iron_volume_loss(a, one, one, one, one, 1 << 20, None) == BAD
    a.mask, a.weight_sum = one, None
    assert train.iron_volume_loss(a, one, one, one, one, 1 << 20, None) == BAD
    assert train.iron_volume_loss_workspace_bytes(1) == 48 and train.iron_volume_loss_workspace_bytes(2048) == 48
    assert train.iron_volume_loss_workspace_bytes(2049) == 96 and train.iron_volume_loss_workspace_bytes(-1) == 0


def _read_ply(path):
    """A binary little-endian PLY with float vertices and `list uchar int` faces -> (vertices, faces)."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert "property list uchar int vertex_indices" in lines
    verts = np.frombuffer(body, dtype="<f4", count=3 * nv).reshape(nv, 3)
    faces = [struct.unpack_from("<Biii", body, 12 * nv + 13 * k) for k in range(nf)]
    assert len(body) == 12 * nv + 13 * nf and all(f[0] == 3 for f in faces)
    return verts, np.array([f[1:] for f in faces], dtype=np.int64).reshape(nf, 3)


def test_write_ply_mesh_reads_back(tmp_path):
    from iron_amd.export_materials import write_ply_mesh
    rng = np.random.default_rng(0)
    verts = rng.standard_normal((7, 3))                  # float64, as extract_geometry returns them
    faces = rng.integers(0, 7, size=(5, 3))
    path = str(tmp_path / "m.ply")
    write_ply_mesh(path, verts, faces)
    v, f = _read_ply(path)
    assert np.array_equal(v, verts.astype(np.float32)) and np.array_equal(f, faces)
    write_ply_mesh(path, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    v, f = _read_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply_mesh(path, verts, np.array([[0, 1, 7]]))
