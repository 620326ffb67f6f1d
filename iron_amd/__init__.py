"""iron_amd -- MI355X (gfx950) implementation of IRON's stage-2 forward render path.

Module names mirror the reference's `models/` package for this path:
    iron_amd.raytracer      <- models/raytracer.py
    iron_amd.renderer_ggx   <- models/renderer_ggx.py
    iron_amd.rendering_func <- models/rendering_func.py
    iron_amd.fields         <- models/fields.py
    iron_amd.embedder       <- models/embedder.py
    iron_amd.image_losses   <- models/image_losses.py
    iron_amd.export_mesh    <- models/export_mesh.py
    iron_amd.tcnn_fields    <- models/tcnn_fields.py (TCNNSDF on iron_amd.hashgrid, the HIP hash-grid encoding; no tiny-cuda-nn)
    iron_amd.export_uv      <- models/export_uv.py (a Blender script: run as `python -m iron_amd.export_uv IN.obj OUT.obj`)
`install_as_models()` registers them under those names for `render_surface.py`-style callers.
"""
from __future__ import annotations

import sys
import types

__version__ = "0.1.0"


def install_as_models() -> None:
    """Make `from models.raytracer import ...` (and friends) resolve to this package.

    The mirrored modules are laid over the caller's own `models` package when there is one -- already imported, or importable from
    sys.path -- so that `models.dataset`, `models.helper` and whatever else it holds keep resolving to the caller's files.  Only
    when no `models` package exists is an empty one made up."""
    import importlib
    import importlib.util

    pkg = sys.modules.get("models")
    if pkg is None:
        try:
            found = importlib.util.find_spec("models") is not None
        except (ImportError, ValueError):
            found = False
        if found:
            pkg = importlib.import_module("models")
        else:
            pkg = types.ModuleType("models")
            pkg.__path__ = []  # mark as package
            sys.modules["models"] = pkg
    for name in ("raytracer", "renderer_ggx", "rendering_func", "fields", "embedder", "renderer", "network_conf", "image_losses",
                 "export_materials", "export_mesh", "tcnn_fields"):
        mod = importlib.import_module("iron_amd." + name)
        sys.modules["models." + name] = mod
        setattr(pkg, name, mod)
