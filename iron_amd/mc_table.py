"""Marching-cubes case table, derived from the face rule below instead of copied from a published table.

Lattice conventions (shared by csrc/mcubes.hip, iron_amd/mesh.py and the test oracle):
  - corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) along (x, y, z) = (i, j, k) from the cell's min corner;
    bit c of the cube index is set when that corner is "above" (u > threshold).
  - edge e = 4 * axis + q runs from the corner at offset `EDGE_ORIGIN[e]` one step along `axis`; q enumerates the offsets on the
    two other axes (ascending axis order, lower one in bit 0).
  - the surface inside one cell is a set of closed loops through its crossed edges.  On every face, walked counter-clockwise
    about the outward normal, each crossing that enters an above corner is joined to the next crossing that leaves one.  On a face
    with two diagonal above corners this separates the above corners; the choice depends on the face's four signs only, so the
    two cells sharing a face pick the same segments (in opposite directions) and the mesh is watertight by construction.
  - each loop is fanned (L edges give L - 2 triangles) from its first vertex, in loop order from the smallest edge id, whose
    fan chords all run through the cell's interior: a chord joining two crossings of one face would lie in that face, where the
    neighbour's triangulation may draw it as well.  Right-hand normals point from the above corners toward the below ones.

`python -m iron_amd.mc_table` rewrites csrc/mc_table.h; tests/test_mc_table.py checks that the committed header matches.
"""
from __future__ import annotations

import os

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.h")

CORNERS = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]


def _edge_origin(e: int):
    axis, q = divmod(e, 4)
    others = [a for a in range(3) if a != axis]
    o = [0, 0, 0]
    o[others[0]], o[others[1]] = q & 1, (q >> 1) & 1
    return tuple(o)


EDGE_AXIS = [e // 4 for e in range(12)]
EDGE_ORIGIN = [_edge_origin(e) for e in range(12)]


def _corner(off) -> int:
    return off[0] | (off[1] << 1) | (off[2] << 2)


def _edge_between(ca: int, cb: int) -> int:
    a, b = CORNERS[ca], CORNERS[cb]
    diff = [i for i in range(3) if a[i] != b[i]]
    assert len(diff) == 1
    lo = a if a[diff[0]] == 0 else b
    return next(e for e in range(12) if EDGE_AXIS[e] == diff[0] and EDGE_ORIGIN[e] == lo)


def _faces():
    """6 faces, each as its 4 corners counter-clockwise about the outward normal."""
    faces = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3  # e_b x e_c = e_a
        for s in (0, 1):
            ring = [(0, 0), (1, 0), (1, 1), (0, 1)] if s == 1 else [(0, 0), (0, 1), (1, 1), (1, 0)]
            corners = []
            for pb, pc in ring:
                off = [0, 0, 0]
                off[a], off[b], off[c] = s, pb, pc
                corners.append(_corner(off))
            faces.append(corners)
    return faces


FACES = _faces()


def case_segments(case: int):
    """Directed segments (from edge, to edge) of one cube index, face by face."""
    above = [(case >> c) & 1 for c in range(8)]
    segs = []
    for ring in FACES:
        ups, downs = [], []  # positions along the ring of crossings entering / leaving an above corner
        for i in range(4):
            c0, c1 = ring[i], ring[(i + 1) % 4]
            if above[c0] != above[c1]:
                (ups if above[c1] else downs).append(i)
        for i in ups:
            j = min(downs, key=lambda d: (d - i) % 4)  # the next leaving crossing going forward
            segs.append((_edge_between(ring[i], ring[(i + 1) % 4]), _edge_between(ring[j], ring[(j + 1) % 4])))
    return segs


def case_loops(case: int):
    """Closed loops of edge ids, each starting at its smallest id, in order of that id."""
    nxt = {}
    for a, b in case_segments(case):
        assert a not in nxt, (case, a)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), case  # every crossed edge starts one segment and ends one
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3, (case, loop)
        loops.append(loop)
    return loops


def _edge_faces(e: int):
    """The two faces (indices into FACES) an edge lies on."""
    return {f for f, ring in enumerate(FACES) if any(_edge_between(ring[i], ring[(i + 1) % 4]) == e for i in range(4))}


_EDGE_FACES = [_edge_faces(e) for e in range(12)]


def _interior(a: int, b: int) -> bool:
    """Does the chord between the crossings on edges a and b run through the cell rather than along a face?  A chord on a face
    could be drawn by the neighbour across that face too, and the edge would then belong to four triangles."""
    return not (_EDGE_FACES[a] & _EDGE_FACES[b])


def _triangulate(loop):
    """Fan from the first loop position whose chords all run through the cell interior."""
    n = len(loop)
    for r in range(n):
        ring = loop[r:] + loop[:r]
        if all(_interior(ring[0], ring[i]) for i in range(2, n - 1)):
            return [(ring[0], ring[i], ring[i + 1]) for i in range(1, n - 1)]
    raise AssertionError("no fan of loop %s avoids the faces" % loop)


def case_triangles(case: int):
    tris = []
    for loop in case_loops(case):
        tris += _triangulate(loop)
    return tris


TABLE = [case_triangles(c) for c in range(256)]
MAX_TRIS = max(len(t) for t in TABLE)


def _check():
    for c in range(256):
        crossed = {e for e in range(12) if ((c >> _corner(EDGE_ORIGIN[e])) & 1)
                   != ((c >> _corner(tuple(o + (i == EDGE_AXIS[e]) for i, o in enumerate(EDGE_ORIGIN[e])))) & 1)}
        used = {e for t in TABLE[c] for e in t}
        assert used == crossed, c
        # single above (or below) corner: the one triangle's normal points from above to below
        if bin(c).count("1") in (1, 7):
            lone = [k for k in range(8) if ((c >> k) & 1) == (1 if bin(c).count("1") == 1 else 0)][0]
            mid = [[EDGE_ORIGIN[e][i] + 0.5 * (i == EDGE_AXIS[e]) for i in range(3)] for e in TABLE[c][0]]
            u = [mid[1][i] - mid[0][i] for i in range(3)]
            v = [mid[2][i] - mid[0][i] for i in range(3)]
            n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            out = [0.5 - CORNERS[lone][i] for i in range(3)]  # from the lone corner toward the cell centre
            dot = sum(n[i] * out[i] for i in range(3))
            assert (dot > 0) == (bin(c).count("1") == 1), c


_check()


def render_header() -> str:
    lines = [
        "// Marching-cubes case table -- GENERATED by iron_amd/mc_table.py (python -m iron_amd.mc_table); do not edit.",
        "// Conventions: see that module's docstring.  Corner c of a cell is at offset (c&1, (c>>1)&1, (c>>2)&1) along (x, y, z);",
        "// edge e runs from kMcEdgeOrigin[e] one step along axis e/4.  Row c of kMcTriEdges lists the edge ids of case c's",
        "// kMcTriCount[c] triangles (3 per triangle, right-hand normal from above toward below; unused slots -1).",
        "#pragma once",
        "#include <hip/hip_runtime.h>",
        "#include <stdint.h>",
        "",
        "namespace iron {",
        "",
        "constexpr int kMcMaxTris = %d;" % MAX_TRIS,
        "",
        "// (dx, dy, dz) of the lower end of each edge",
        "__constant__ int8_t kMcEdgeOrigin[12][3] = {%s};" % ", ".join("{%d, %d, %d}" % o for o in EDGE_ORIGIN),
        "",
        "__constant__ uint8_t kMcTriCount[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(TABLE[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("")
    lines.append("__constant__ int8_t kMcTriEdges[256][%d] = {" % (3 * MAX_TRIS))
    for c in range(256):
        flat = [e for t in TABLE[c] for e in t]
        flat += [-1] * (3 * MAX_TRIS - len(flat))
        lines.append("    {%s},  // %d" % (", ".join(str(e) for e in flat), c))
    lines.append("};")
    lines.append("")
    lines.append("}  // namespace iron")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(HEADER_PATH, "w") as f:
        f.write(render_header())
    print("wrote %s (max %d triangles per case)" % (HEADER_PATH, MAX_TRIS))
