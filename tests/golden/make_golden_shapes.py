"""Golden vectors G19 for the network-shape matrix (tests/_nets.py) -- BUILD CONTAINER ONLY (needs the reference).

Builds the reference's own SDFNetwork / RenderingNetwork / NeRF on CPU at every shape listed in tests/_nets.py that computes,
moves its parameters off the init with tests/_nets.generalise, and records per shape: the state hash (fp32 parameters), a few
input rows, and the reference's outputs in fp64 (the module cast to double): SDF forward columns, d sdf / dx of get_all,
material outputs, NeRF alpha / rgb.  tests/test_net_shapes_oracle.py pins oracle/iron_ref.py and neus_ref.py to them.

The archive is written with fixed zip timestamps, so a re-run reproduces g19_shapes.npz bit for bit.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_shapes.py
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (for _nets, _util)
import make_golden as MG  # noqa: E402,F401  (puts the reference and the repository on sys.path)

from models.fields import NeRF, RenderingNetwork, SDFNetwork  # noqa: E402  (reference)

import _nets as N  # noqa: E402
from _util import state_hash  # noqa: E402

OUT = os.path.join(HERE, "g19_shapes.npz")
ROWS = 24
SDF_COLS = (0, 1, 2, 128, 256)   # the distance and a few feature columns (d_out = 257)


def key(*parts) -> str:
    return "__".join(p.replace("/", ".") for p in parts)


def sdf_records(rec):
    for name in N.SDF_SHAPES:
        kw = N.sdf_kw(name)
        net = N.build(SDFNetwork, kw, name)
        rec[key("hash", "sdf", name)] = np.array(state_hash({"sdf_network": net}))
        x = N.sdf_inputs(ROWS, N.seed_of(name) + 2, kw["scale"]).double()
        net = net.double()
        xg = x.clone().requires_grad_(True)
        out = net(xg)
        (grad,) = torch.autograd.grad(out[:, :1], xg, torch.ones_like(out[:, :1]))
        cols = [c for c in SDF_COLS if c < kw["d_out"]]
        rec[key("sdf", name, "x")] = x.numpy()
        rec[key("sdf", name, "out")] = out[:, cols].detach().numpy()
        rec[key("sdf", name, "grad")] = grad.detach().numpy()


def render_records(rec):
    for name, kw in N.RENDER_SHAPES.items():
        net = N.build(RenderingNetwork, kw, name)
        rec[key("hash", "render", name)] = np.array(state_hash({"net": net}))
        pts, nrm, view, feat = (v.double() for v in N.render_inputs(ROWS, N.seed_of(name) + 2))
        use_view = kw["mode"] in ("idr", "no_normal")
        out = net.double()(pts, nrm, view if use_view else None, feat)
        rec[key("render", name, "out")] = out.detach().numpy()


def nerf_records(rec):
    for name in N.NERF_SHAPES:
        kw = N.nerf_kw(name)
        net = N.build(NeRF, kw, name)
        rec[key("hash", "nerf", name)] = np.array(state_hash({"net": net}))
        pts, views = (v.double() for v in N.nerf_inputs(ROWS, N.seed_of(name) + 2))
        alpha, rgb = net.double()(pts, views)
        rec[key("nerf", name, "alpha")] = alpha.detach().numpy()
        rec[key("nerf", name, "rgb")] = rgb.detach().numpy()


def save_deterministic(path, arrays):
    """np.savez_compressed, but with fixed member timestamps and order."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(8)
    rec = {}
    sdf_records(rec)
    render_records(rec)
    nerf_records(rec)
    save_deterministic(OUT, rec)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(rec), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
