"""Golden vectors G21 for the material texture bake -- BUILD CONTAINER ONLY (imports the reference's models/export_materials.py).

igl, trimesh and imageio are not installed: this script registers empty placeholders for them, which the recorded functions
(sample_surface, accumulate_splat_material) never touch.  The fixture mesh is not stored: it is rebuilt from the integer-only
recipe of tests/_bake_oracle.py (g21_mesh), and the archive keeps its SHA-256.

Recorded from the reference, with the module's `np` replaced by a proxy that passes every call through and keeps the outputs of
np.ceil, np.random.choice and np.random.rand:
- sample_surface on the fixture (np.random.seed(21), then 3000 samples; then 2000 more): points, uvs, the ceil counts, the drawn
  face indices and the r draws;
- accumulate_splat_material over three successive calls into 96 x 64 images (the first sampling, a grid of edge uvs, the second
  sampling), with values from g21_values; the images after the first and the third call;
- the .mtl text and the head of the rewritten OBJ of export_materials, and the module's inspect.signature's.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bake.py
"""
from __future__ import annotations

import inspect
import io
import json
import os
import re
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (for _bake_oracle)
import make_golden as MG  # noqa: E402,F401  (reference on sys.path)

import _bake_oracle as O  # noqa: E402

for _n in ("igl", "trimesh", "imageio"):
    sys.modules.setdefault(_n, types.ModuleType(_n))

import models.export_materials as EM  # noqa: E402  (reference)

OUT = os.path.join(HERE, "g21_bake.npz")


class _Rec:
    def __init__(self):
        self.log = {"ceil": [], "choice": [], "rand": []}


class _RandomProxy:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, k):
        return getattr(np.random, k)

    def choice(self, *a, **k):
        out = np.random.choice(*a, **k)
        self._rec.log["choice"].append(np.array(out))
        return out

    def rand(self, *a, **k):
        out = np.random.rand(*a, **k)
        self._rec.log["rand"].append(np.array(out))
        return out


class _NpProxy:
    def __init__(self, rec):
        self._rec = rec
        self.random = _RandomProxy(rec)

    def __getattr__(self, k):
        return getattr(np, k)

    def ceil(self, *a, **k):
        out = np.ceil(*a, **k)
        self._rec.log["ceil"].append(np.array(out))
        return out


def describe(fn):
    return [{"name": p.name, "kind": p.kind.name, "default": None if p.default is inspect._empty else repr(p.default)}
            for p in inspect.signature(fn).parameters.values()]


def main():
    rec = {}
    verts, faces, uvs, fuv = O.g21_mesh()
    rec["sha256__mesh"] = np.array(O.sha256(verts, faces, uvs, fuv))
    R = _Rec()
    EM.np = _NpProxy(R)
    np.random.seed(21)
    for k, n in enumerate((3000, 2000)):
        for v in R.log.values():
            v.clear()
        P, Q = EM.sample_surface(verts, faces, uvs, fuv, n)
        ceil_c = R.log["ceil"][0].astype(np.int64)
        drawn = R.log["choice"][0].astype(np.int64) if R.log["choice"] else np.zeros((0,), np.int64)
        r = R.log["rand"][0]
        counts = ceil_c.copy()
        counts[drawn] -= 1
        p = "sample%d__" % k
        rec[p + "n"] = np.int64(n)
        rec[p + "points"], rec[p + "uv"] = P, Q
        rec[p + "ceil_counts"], rec[p + "drawn"], rec[p + "counts"], rec[p + "r"] = ceil_c, drawn, counts, r
        print("sample %d: n %d total %d floor_num %d distinct %d" % (k, n, len(P), len(drawn), len(np.unique(drawn))))
    EM.np = np

    H, W = O.G21_HW
    xyz = np.zeros((H, W, 3), dtype=np.float32)
    mat = np.zeros((H, W, 7), dtype=np.float32)
    wgt = np.zeros((H, W), dtype=np.float32)
    edge_uv = O.g21_edge_uvs()
    calls = [(rec["sample0__points"], rec["sample0__uv"]),
             (O.g21_values(len(edge_uv), 3, 9) * 2.0 - 1.0, edge_uv),
             (rec["sample1__points"], rec["sample1__uv"])]
    for c, (pcd, uv) in enumerate(calls):
        m = O.g21_values(len(pcd), 7, c)
        rec["splat%d__pcd" % c], rec["splat%d__uv" % c], rec["splat%d__material" % c] = pcd, uv.copy(), m
        EM.accumulate_splat_material(xyz, mat, wgt, pcd.copy(), uv.copy(), m)
        if c in (0, 2):
            rec["splat_after%d__xyz" % c], rec["splat_after%d__material" % c], rec["splat_after%d__weight" % c] = (
                xyz.copy(), mat.copy(), wgt.copy())

    src = inspect.getsource(EM.export_materials)
    lines = [m for m in re.findall(r'"([^"\n]*\\n)"', src) if not m.startswith("usemtl")]
    rec["mtl_text"] = np.array("".join(lines).replace("\\n", "\n"))
    rec["usemtl_line"] = np.array("usemtl ./{}\n\n".format("mesh.obj"[:-4] + ".mtl"))
    sigs = {name: {"type": "function", "params": describe(getattr(EM, name))}
            for name in ("sample_surface", "accumulate_splat_material", "loadmesh_and_checkuv", "export_materials", "to8b")}
    sigs["Groupby"] = {"type": "class", "methods": {"__init__": describe(EM.Groupby.__init__), "apply": describe(EM.Groupby.apply)}}
    rec["signatures_json"] = np.array(json.dumps(sigs, sort_keys=True))

    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(rec[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
