"""Host-side checks of the stage-2 trainer (no GPU): the command line, checkpoint ordering, the layout of FusedAdam's state and
the agreement of include/iron_train.h with the ctypes signatures of the entries csrc/optim.hip adds."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_parsing_carries_the_reference_names_and_defaults():
    """render_surface.py:42-95."""
    from iron_amd.train_surface import config_parser
    a = config_parser().parse_args([])
    want = {"data_dir": None, "out_dir": None, "folder_name": "image", "neus_ckpt_fpath": None, "num_iters": 100001, "patch_size": 128,
            "eik_weight": 0.1, "ssim_weight": 1.0, "roughrange_weight": 0.1, "no_edgesample": False, "inv_gamma_gt": False,
            "gamma_pred": False, "init_light_scale": 8.0, "export_all": False, "render_all": False, "gpu": 0,
            "seed": 0, "optimizer": "fused", "renderer_name": "comp"}
    for k, v in want.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    b = config_parser().parse_args("--data_dir D --out_dir O --patch_size 64 --no_edgesample --inv_gamma_gt --gamma_pred --eik_weight 0.2 "
                                   "--ssim_weight 0.5 --roughrange_weight 0.3 --init_light_scale 4 --neus_ckpt_fpath N --folder_name rgb "
                                   "--num_iters 7 --optimizer torch --renderer_name ggx --seed 3 --export_all".split())
    assert (b.data_dir, b.out_dir, b.patch_size, b.no_edgesample, b.inv_gamma_gt, b.gamma_pred) == ("D", "O", 64, True, True, True)
    assert (b.eik_weight, b.ssim_weight, b.roughrange_weight, b.init_light_scale) == (0.2, 0.5, 0.3, 4.0)
    assert (b.neus_ckpt_fpath, b.folder_name, b.num_iters, b.optimizer, b.renderer_name, b.seed, b.export_all) == ("N", "rgb", 7, "torch", "ggx", 3, True)
    with pytest.raises(SystemExit):
        config_parser().parse_args(["--optimizer", "sgd"])


def test_trainer_defaults_are_the_parser_defaults():
    import inspect
    from iron_amd.train_surface import SurfaceTrainer, config_parser
    sig = inspect.signature(SurfaceTrainer.__init__).parameters
    a = config_parser().parse_args([])
    for k in ("folder_name", "renderer_name", "patch_size", "eik_weight", "ssim_weight", "roughrange_weight", "init_light_scale", "inv_gamma_gt",
              "gamma_pred", "no_edgesample", "neus_ckpt_fpath", "seed", "optimizer", "data_dir", "out_dir"):
        assert sig[k].default == getattr(a, k), k


def test_checkpoint_paths_are_ordered_by_step_like_load_ckpt(tmp_path):
    """utils/ckpt_loader.py:8-19: by the integer between 'ckpt_' and '.pth', not by the string."""
    from iron_amd.train_surface import checkpoint_paths
    assert checkpoint_paths(str(tmp_path)) == []
    for step in (1000, 0, 20000, 3000):
        (tmp_path / ("ckpt_%d.pth" % step)).write_bytes(b"")
    (tmp_path / "state_20000.pth").write_bytes(b"")
    (tmp_path / "logim_100_0.png").write_bytes(b"")
    got = checkpoint_paths(str(tmp_path))
    assert [s for s, _ in got] == [0, 1000, 3000, 20000]
    assert [os.path.basename(p) for _, p in got] == ["ckpt_0.pth", "ckpt_1000.pth", "ckpt_3000.pth", "ckpt_20000.pth"]


def test_name_ordering_of_the_dataset_loader():
    """models/dataset.py:1409-1413: by the integer in front of the extension when every name has one, else by the string."""
    from iron_amd.dataset import ordered_names, to8b
    import numpy as np
    assert ordered_names(["10.png", "2.png", "0.jpg"]) == ["0.jpg", "2.png", "10.png"]
    assert ordered_names(["b_10.png", "a_2.png", "10.png"]) == ["10.png", "a_2.png", "b_10.png"]
    assert to8b(np.array([-0.5, 0.0, 0.5, 1.0, 2.0])).tolist() == [0, 0, 127, 255, 255]


def test_fused_adam_state_dict_has_torch_adams_layout():
    from iron_amd.optim import FusedAdam

    def params():
        torch.manual_seed(0)
        return [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(()))]

    def groups(ps):
        return [{"params": ps[:2], "lr": 1e-4}, {"params": ps[2:], "lr": 1e-2}]
    pt, pf = params(), params()
    adam, fused = torch.optim.Adam(groups(pt)), FusedAdam(groups(pf))
    assert isinstance(fused, torch.optim.Optimizer)
    a, f = adam.state_dict(), fused.state_dict()
    assert a["param_groups"] == f["param_groups"] and f["state"] == {}
    assert [g["lr"] for g in fused.param_groups] == [1e-4, 1e-2] and fused.defaults["betas"] == (0.9, 0.999) and fused.defaults["eps"] == 1e-8
    for p in pt:
        p.grad = torch.ones_like(p)
    adam.step()
    fused.load_state_dict(adam.state_dict())   # torch's state into ours ...
    f = fused.state_dict()
    assert sorted(f["state"]) == [0, 1, 2]
    for i in range(3):
        assert set(f["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(f["state"][i]["step"]) == 1.0 and not f["state"][i]["step"].is_cuda
        assert torch.equal(f["state"][i]["exp_avg"], adam.state_dict()["state"][i]["exp_avg"])
    again = torch.optim.Adam(groups(params()))
    again.load_state_dict(f)                    # ... and ours into torch's
    assert again.state_dict()["param_groups"] == a["param_groups"]
    fused.zero_grad()
    # no CPU path: stepping host parameters is refused, and nothing moves
    from iron_amd import _lib
    pf[0].grad = torch.ones_like(pf[0])
    with pytest.raises(_lib.IronError):
        fused.step()
    assert float(fused.state[pf[0]]["step"]) == 1.0


def _header_prototypes():
    hdr = open(os.path.join(ROOT, "include", "iron_train.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"^\s*(size_t|int)\s+(iron_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.M | re.S):
        protos[name] = (ret, [" ".join(a.split()) for a in args.split(",")])
    structs = {}
    for body, name in re.findall(r"typedef struct \w+ \{(.*?)\}\s*(\w+);", hdr, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            first, *rest = decl.split(",")
            typ, n0 = first.rsplit(" ", 1)
            for n in [n0] + [r.strip() for r in rest]:
                fields.append((typ + ("*" if n.startswith("*") else ""), n.lstrip("*")))
        structs[name] = fields
    return protos, structs, hdr


def _ctype_of(decl):
    """The ctypes type of one C parameter / field declaration of the two new entries."""
    d = decl.replace("const ", "").strip()
    if "*" in d:
        base = d.split("*")[0].strip()
        return {"iron_adam_tensor": "struct iron_adam_tensor", "iron_surface_reg_args": "struct iron_surface_reg_args"}.get(base, C.c_void_p)
    base = d.rsplit(" ", 1)[0] if " " in d else d
    return {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int}[base]


def test_header_and_ctypes_agree_on_the_new_entries():
    from iron_amd import _lib
    protos, structs, hdr = _header_prototypes()
    for name in ("iron_adam_multi", "iron_surface_reg_workspace_bytes", "iron_surface_reg", "iron_surface_reg_backward"):
        ret, args = protos[name]
        res, argtypes = _lib.TRAIN_SYMBOLS[name]
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[ret], name
        assert len(args) == len(argtypes), (name, args)
        for decl, ct in zip(args, argtypes):
            want = _ctype_of(decl)
            if isinstance(want, str):
                assert ct is C.POINTER(getattr(_lib, want.split()[1])), (name, decl)
            else:
                assert ct is want, (name, decl, ct)
    for sname in ("iron_adam_tensor", "iron_surface_reg_args"):
        cfields = getattr(_lib, sname)._fields_
        assert [n for _, n in structs[sname]] == [n for n, _ in cfields], sname
        for (typ, n), (_, ct) in zip(structs[sname], cfields):
            assert ct is _ctype_of(typ + " x" if "*" not in typ else typ), (sname, n)
    assert int(re.search(r"#define IRON_ADAM_CHUNK (\d+)", hdr).group(1)) == _lib.IRON_ADAM_CHUNK
    assert int(re.search(r"#define IRON_ADAM_MAX_TENSORS (\d+)", hdr).group(1)) == _lib.IRON_ADAM_MAX_TENSORS
    assert C.sizeof(_lib.iron_adam_tensor) == 56 and C.sizeof(_lib.iron_surface_reg_args) == 72
    # argument checks run on the host, before anything is enqueued
    from iron_amd import build
    build.build()
    lib = _lib.load_train()
    t = (_lib.iron_adam_tensor * 1)()
    t[0].numel, t[0].step = 4, 1
    assert lib.iron_adam_multi(t, 1, 0.9, 0.999, 1e-8, 0, None) == _lib.IRON_ERR_BAD_ARG      # null pointers
    t[0].numel, t[0].step = 0, 0
    assert lib.iron_adam_multi(t, 1, 0.9, 0.999, 1e-8, 0, None) == _lib.IRON_ERR_BAD_ARG      # t < 1
    t[0].numel, t[0].step = -1, 1
    assert lib.iron_adam_multi(t, 1, 0.9, 0.999, 1e-8, 0, None) == _lib.IRON_ERR_BAD_ARG      # negative size
    assert lib.iron_adam_multi(t, 0, 0.9, 0.999, 1e-8, 0, None) == 0                          # an empty table is a no-op
    assert lib.iron_surface_reg_workspace_bytes(4097, 0, 0) == 3 * 6 * 8
