"""evaluation/eval_mesh.py on the HIP kernels: the symmetric mean point-to-mesh distance between a predicted
and a target mesh, without igl.  The distances come from iron_amd.mesh_distance, the OBJ reader from iron_amd.export_materials.

    python -m iron_amd.eval_mesh PRED.obj TRGT.obj      prints the reference's line, '\\tChamfer_dist:  <value>'
"""
from __future__ import annotations

import sys

from .export_materials import read_obj
from .mesh_distance import chamfer_distance


def cal_mesh_err(va, fa, vb, fb):
    """0.5 * (mean distance of va to mesh (vb, fb) + mean distance of vb to mesh (va, fa)); evaluation/eval_mesh.py:6-12."""
    return chamfer_distance(va, fa, vb, fb)


def eval_obj_meshes(pred_mesh_fpath, trgt_mesh_fpath):
    v1, _, f1, _ = read_obj(pred_mesh_fpath)
    v4, _, f4, _ = read_obj(trgt_mesh_fpath)
    return cal_mesh_err(v1, f1, v4, f4)


def main(argv=None) -> None:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        raise SystemExit("usage: python -m iron_amd.eval_mesh PRED.obj TRGT.obj")
    dist_bidirectional = eval_obj_meshes(argv[0], argv[1])
    print('\tChamfer_dist: ', dist_bidirectional)


if __name__ == "__main__":
    main()
