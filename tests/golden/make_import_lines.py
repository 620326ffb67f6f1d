"""Import-line fixture (BUILD CONTAINER ONLY -- reads the reference's callers): every `from models.<module> import <names>` statement
of the reference's drivers, found with `ast` (no caller is imported or executed), module-level and nested ones alike.
Data only: caller file -> module -> sorted list of imported names -> tests/golden/reference_import_lines.json;
tests/test_dropin_imports.py replays the lines against iron_amd.install_as_models().

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_import_lines.py [reference root]
"""
from __future__ import annotations

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CALLERS = ["render_surface.py", "render_nir.py", "render_volume.py", "model_volume.py", "model_bed.py", "utils/process_routine.py"]


def import_lines(path: str) -> dict:
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level == 0 and node.module and node.module.startswith("models."):
            found.setdefault(node.module[len("models."):], set()).update(a.name for a in node.names)
    return {mod: sorted(names) for mod, names in sorted(found.items())}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {caller: import_lines(os.path.join(root, caller)) for caller in CALLERS}
    with open(os.path.join(HERE, "reference_import_lines.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print({k: sum(len(v) for v in m.values()) for k, m in out.items()})


if __name__ == "__main__":
    main()
