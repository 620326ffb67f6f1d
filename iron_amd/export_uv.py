"""Drop-in for models/export_uv.py, the Blender script the stage-2 driver runs on the exported mesh
(`blender --background --python models/export_uv.py IN.obj OUT.obj`, render_surface.py:427): here
`python -m iron_amd.export_uv IN.obj OUT.obj`, which takes the last two arguments like the script, with the UV layout of
iron_amd.uv_unwrap.smart_uv_project (Smart UV project at Blender's default settings, on the HIP kernels).

The OBJ is read with export_materials.read_obj and written with export_materials.write_obj: the `v` lines and the face order are
kept, the file gains `vt` lines and `f a/b` indices.  IN and OUT may be the same file.

Deviations from the Blender export, on purpose:
- no `vn`, `o` or `s` lines (nothing downstream reads them: export_materials uses `v`, `vt` and `f`);
- coordinates are written round-trip exact for fp32 (`%.9g`) instead of Blender's six decimals;
- the layout follows the contract of iron_amd.uv_unwrap, not Blender's code bit for bit.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from . import _lib
from .export_materials import read_obj, write_obj
from .uv_unwrap import smart_uv_project


def export_uv(in_mesh_fpath, out_mesh_fpath):
    """Unwrap the mesh of `in_mesh_fpath` with smart_uv_project's defaults and write it with UVs to `out_mesh_fpath` (both .obj)."""
    assert in_mesh_fpath.endswith(".obj"), f"must use .obj format: {in_mesh_fpath}"
    assert out_mesh_fpath.endswith(".obj"), f"must use .obj format: {out_mesh_fpath}"
    vertices, _, faces, _ = read_obj(in_mesh_fpath)
    if not torch.cuda.is_available():
        raise _lib.IronError("export_uv needs a GPU (iron_amd has no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    uvs, face_uvs = smart_uv_project(torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev))
    write_obj(out_mesh_fpath, vertices, uvs.cpu().numpy(), faces, face_uvs.cpu().numpy().astype(np.int64))


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 3:
        raise SystemExit("usage: python -m iron_amd.export_uv IN.obj OUT.obj")
    export_uv(argv[-2], argv[-1])


if __name__ == "__main__":
    main()
