"""Generate triplaneturbo_amd/csrc/tt_mc_tables.h: the marching-cubes case tables of tt_isosurface.hip.

The tables are derived, not transcribed (include/tt_abi.h, "marching cubes"):
  1. every cube face gets its segments from its own 4 inside/outside bits alone; on an ambiguous face (two diagonal
     inside corners) each inside corner is cut off by its own segment.  A face's segments therefore do not depend on
     the rest of the cell, two cells that share a face cut it the same way, and the mesh is watertight by construction;
  2. each segment is directed so that, seen from outside the cube, the inside corners lie on its right; the directed
     segments chain into disjoint closed loops (every crossing point has degree 2);
  3. each loop is fan-triangulated from its smallest edge id, so cross(v1 - v0, v2 - v0) points from the inside
     (level < iso) to the outside.

Conventions (shared with the kernels and tests/mc_reference.py):
  corner c = di | dj << 1 | dk << 2          offset (di, dj, dk) of the cell origin (i, j, k); k is the fastest axis
  case     = sum over corners of inside(c) << c
  edge e   = 4 * axis + the two other offset bits of its base corner, lower axis first
             (axis 0: dj + 2 dk, axis 1: di + 2 dk, axis 2: di + 2 dj); the edge runs from the base corner along +axis,
             so it is owned by grid point origin + base offset.

usage: python tools/gen_mc_tables.py [--check]   (writes the header, prints the largest triangle count per case;
       --check compares with the committed header instead and exits 1 on a difference)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "triplaneturbo_amd", "csrc", "tt_mc_tables.h")


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(off):
    return off[0] | (off[1] << 1) | (off[2] << 2)


def edge_id(axis, base):
    u, v = [a for a in range(3) if a != axis]
    return 4 * axis + base[u] + 2 * base[v]


def edge_corners(e):
    """(base corner, far corner) of edge e"""
    axis, r = divmod(e, 4)
    u, v = [a for a in range(3) if a != axis]
    base = [0, 0, 0]
    base[u], base[v] = r & 1, r >> 1
    far = list(base)
    far[axis] = 1
    return corner_id(base), corner_id(far)


def edge_axis_base(e):
    b, _ = edge_corners(e)
    return e // 4, corner_offset(b)


def edge_midpoint(e):
    a, b = edge_corners(e)
    pa, pb = corner_offset(a), corner_offset(b)
    return tuple((x + y) / 2.0 for x, y in zip(pa, pb))


def faces():
    """(axis, side, corners in a cycle around the face)"""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            cyc = []
            for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis], off[u], off[v] = side, cu, cv
                cyc.append(corner_id(off))
            out.append((axis, side, cyc))
    return out


def edge_between(c0, c1):
    p0, p1 = corner_offset(c0), corner_offset(c1)
    axis = [a for a in range(3) if p0[a] != p1[a]]
    assert len(axis) == 1
    base = p0 if p0[axis[0]] == 0 else p1
    return edge_id(axis[0], base)


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def face_segments(case, face):
    """Directed segments (edge_from, edge_to) of one face, from the face's 4 bits only.  The inside corner cut off by a
    segment lies on its right when the face is seen from outside the cube."""
    axis, side, cyc = face
    inside = [(case >> c) & 1 for c in cyc]
    n_in = sum(inside)
    if n_in in (0, 4):
        return []
    normal = [0.0, 0.0, 0.0]
    normal[axis] = 1.0 if side else -1.0
    segs = []
    if n_in == 2 and inside[0] == inside[2]:
        # ambiguous face: each inside corner cut off separately
        groups = [[i] for i in range(4) if inside[i]]
    else:
        # one connected run of inside corners (1, 2 adjacent or 3 of them) -> one segment
        groups = [[i for i in range(4) if inside[i]]]
    for g in groups:
        # the two crossing edges adjacent to the inside run
        ends = []
        for i in g:
            for j in ((i + 1) % 4, (i + 3) % 4):
                if not inside[j]:
                    ends.append(edge_between(cyc[i], cyc[j]))
        assert len(ends) == 2, (case, face, ends)
        a, b = ends
        pa, pb = edge_midpoint(a), edge_midpoint(b)
        ref = corner_offset(cyc[g[0]])
        # inside on the right seen from outside: cross(b - a, inside - a) . outward normal < 0
        if _dot(_cross(_sub(pb, pa), _sub(ref, pa)), normal) > 0:
            a, b = b, a
        segs.append((a, b))
    return segs


def case_loops(case):
    nxt = {}
    for f in faces():
        for a, b in face_segments(case, f):
            assert a not in nxt, (case, a)
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        loops.append(loop)
    return loops


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        m = loop.index(min(loop))
        loop = loop[m:] + loop[:m]
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def tables():
    return [case_triangles(c) for c in range(256)]


def render():
    tabs = tables()
    max_tris = max(len(t) for t in tabs)
    lines = [
        "// tt_mc_tables.h -- GENERATED by tools/gen_mc_tables.py; do not edit (tests/test_isosurface_tables.py checks it).",
        "// Marching-cubes case tables of tt_isosurface.hip: face-consistent segments (an ambiguous face cuts its two inside",
        "// corners off separately), loops directed with the inside on their right seen from outside, fan-triangulated from",
        "// the smallest edge id; cross(v1 - v0, v2 - v0) points from level < iso to level >= iso.",
        "// corner c = di | dj << 1 | dk << 2; case = sum inside(c) << c;",
        "// edge e = 4 * axis + other offset bits of its base corner (axis 0: dj + 2 dk, axis 1: di + 2 dk, axis 2: di + 2 dj).",
        "#pragma once",
        "",
        f"#define TT_MC_MAX_TRIS {max_tris}",
        "",
        "#ifndef TT_MC_TABLE",
        "#define TT_MC_TABLE static const",
        "#endif",
        "",
        "// triangles per case",
        "TT_MC_TABLE unsigned char tt_mc_tri_count[256] = {",
    ]
    counts = [len(t) for t in tabs]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(c) for c in counts[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// edge triplets per case, 255 = unused")
    lines.append(f"TT_MC_TABLE unsigned char tt_mc_tri_edges[256][{3 * max_tris}] = {{")
    for c, t in enumerate(tabs):
        flat = [e for tri in t for e in tri] + [255] * (3 * (max_tris - len(t)))
        lines.append("    {" + ", ".join(str(x) for x in flat) + f"}},  // {c}")
    lines.append("};")
    lines.append("")
    return "\n".join(lines), max_tris


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text, max_tris = render()
    if a.check:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("up to date" if same else f"{HEADER} differs from the generator")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(f"wrote {HEADER}: largest triangle count per case = {max_tris}")


if __name__ == "__main__":
    main()
