"""Generates the marching-cubes case table csrc/hm_mc_table.h (the single source of truth for the topology).

    python scripts/gen_mc_table.py            # rewrite the header
    python scripts/gen_mc_table.py --check    # exit 1 if the checked-in header differs

For each of the 256 corner sign patterns (a corner is inside when its value is < level):
  - on each of the 6 cube faces the crossing edges are joined by segments.  A face has 0, 2 or 4 crossing edges; with
    4 (diagonal corners alike, the ambiguous face) every inside corner of the face is cut off on its own.  The rule
    depends on the face's four signs alone, so the two cells sharing a face cut it the same way and the mesh has no
    cracks;
  - each segment is oriented so that, seen from outside the cube, the inside corner lies on its right;
  - every crossing edge then ends exactly one segment and starts exactly one, so the segments close into directed
    loops; each loop is fan-triangulated from its first vertex (in loop order from the smallest edge) that has no
    diagonal to a vertex on a cube face it lies on (the neighbouring cell could use the same chord).  The triangle
    normal (v1-v0) x (v2-v0) points toward increasing values (outward for an SDF).
This differs from skimage's marching_cubes_lewiner inside ambiguous cells only (mesh extraction).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "hashmodnffbanks_idr_amd", "csrc", "hm_mc_table.h")
MAX_TRIS = 5


def corner_offset(c):
    """lattice offset (along volume axes 0, 1, 2) of cube corner c from the cell's lowest point"""
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


# edge e runs along axis e // 4 from EDGE_CORNER[e], the (e % 4)-th corner whose bit of that axis is 0
EDGE_CORNER = [c for a in range(3) for c in range(8) if not (c >> a) & 1]
EDGE_AXIS = [e // 4 for e in range(12)]


def _edge(u, w):
    """the cube edge between corners u and w (differing in one bit)"""
    a = (u ^ w).bit_length() - 1
    return EDGE_AXIS.index(a) + EDGE_CORNER[4 * a:4 * a + 4].index(min(u, w))


def _faces():
    """(outward normal, corners in cyclic order) of the 6 cube faces"""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for s in (0, 1):
            n = np.zeros(3)
            n[a] = 2 * s - 1
            cyc = [(s << a) | (p << b) | (q << c) for p, q in ((0, 0), (1, 0), (1, 1), (0, 1))]
            out.append((n, cyc))
    return out


def _mid(e):
    p = np.array(corner_offset(EDGE_CORNER[e]), dtype=float)
    p[EDGE_AXIS[e]] += 0.5
    return p


def face_segments(case, normal, cyc):
    """directed segments (edge_from, edge_to) of one face for a sign pattern"""
    inside = [(case >> c) & 1 for c in cyc]
    edges = [_edge(cyc[m], cyc[(m + 1) % 4]) for m in range(4)]  # edges[m] joins cyc[m] and cyc[m+1]
    crossing = [m for m in range(4) if inside[m] != inside[(m + 1) % 4]]
    if len(crossing) == 2:
        pairs = [(edges[crossing[0]], edges[crossing[1]])]
    elif len(crossing) == 4:
        pairs = [(edges[(m - 1) % 4], edges[m]) for m in range(4) if inside[m]]
    else:
        pairs = []
    segs = []
    for e1, e2 in pairs:
        p, q = _mid(e1), _mid(e2)
        c0 = EDGE_CORNER[e1]
        c_in = c0 if (case >> c0) & 1 else c0 | (1 << EDGE_AXIS[e1])
        left = np.dot(np.array(corner_offset(c_in), dtype=float) - p, np.cross(normal, q - p))
        assert left != 0.0
        segs.append((e1, e2) if left < 0 else (e2, e1))
    return segs


def _edge_faces(e):
    """the two cube faces (axis, side) edge e lies on"""
    c, a = EDGE_CORNER[e], EDGE_AXIS[e]
    return {(b, (c >> b) & 1) for b in range(3) if b != a}


def _fan_ok(loop, s):
    n = len(loop)
    return all(not (_edge_faces(loop[s]) & _edge_faces(loop[(s + d) % n])) for d in range(2, n - 1))


def case_triangles(case):
    succ = {}
    for n, cyc in _faces():
        for e1, e2 in face_segments(case, n, cyc):
            assert e1 not in succ, (case, e1)
            succ[e1] = e2
    assert sorted(succ) == sorted(succ.values()), case  # every crossing edge starts one segment and ends one
    tris, seen = [], set()
    for start in sorted(succ):
        if start in seen:
            continue
        loop = [start]
        while succ[loop[-1]] != start:
            loop.append(succ[loop[-1]])
        seen.update(loop)
        # fan from the first vertex (in loop order from the smallest edge) with no diagonal to a vertex on a cube face
        # it lies on: such a chord lies in that face, and the neighbouring cell may use the same chord (an edge in four
        # triangles).  Only an ambiguous face puts two non-adjacent loop vertices on one face.
        s = next(s for s in range(len(loop)) if _fan_ok(loop, s))
        loop = loop[s:] + loop[:s]
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    assert len(tris) <= MAX_TRIS, case
    return tris


def generate():
    """[256] lists of edge triples"""
    return [case_triangles(c) for c in range(256)]


def render(table=None):
    table = generate() if table is None else table
    lines = [
        "// hm_mc_table.h - marching-cubes case table, GENERATED by scripts/gen_mc_table.py (do not edit; the generator",
        "// states the rule; tests/test_mesh_cpu.py regenerates it and compares).",
        "//   corner c of a cell sits at lattice offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's lowest point;",
        "//   edge e runs along volume axis hm_mc_edge_axis[e] from corner hm_mc_edge_corner[e];",
        "//   case = sum of (1 << c) over the corners with value < level;",
        "//   hm_mc_tris[case] = {triangle count, then 3 edges per triangle, unused entries -1}; the triangle normal",
        "//   (v1-v0) x (v2-v0) points toward increasing values.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "constexpr int8_t hm_mc_edge_corner[12] = {" + ", ".join(map(str, EDGE_CORNER)) + "};",
        "constexpr int8_t hm_mc_edge_axis[12] = {" + ", ".join(map(str, EDGE_AXIS)) + "};",
        f"constexpr int hm_mc_max_tris = {MAX_TRIS};",
        "",
        f"constexpr int8_t hm_mc_tris[256][{1 + 3 * MAX_TRIS}] = {{",
    ]
    for c, tris in enumerate(table):
        row = [len(tris)] + [e for t in tris for e in t]
        row += [-1] * (1 + 3 * MAX_TRIS - len(row))
        lines.append("    {" + ", ".join(f"{v:2d}" for v in row) + f"}},  // {c}")
    lines += ["};", ""]
    return "\n".join(lines)


def table_array(table=None):
    """int8 [256, 1 + 3*MAX_TRIS] in the header's layout"""
    table = generate() if table is None else table
    out = np.full((256, 1 + 3 * MAX_TRIS), -1, np.int8)
    for c, tris in enumerate(table):
        out[c, 0] = len(tris)
        out[c, 1:1 + 3 * len(tris)] = np.asarray(tris, np.int8).reshape(-1)
    return out


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("hm_mc_table.h is " + ("up to date" if same else "STALE"))
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)
