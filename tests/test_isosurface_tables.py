"""The marching-cubes case tables (triplaneturbo_amd/csrc/tt_mc_tables.h) are what tools/gen_mc_tables.py generates, and
they have the properties the generator claims, checked exhaustively over the 256 cases without the generator's code."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gen_mc_tables as G  # noqa: E402
from mc_reference import EDGE_AXIS, EDGE_BASE, load_tables  # noqa: E402

COUNT, EDGES = load_tables()
MAX_TRIS = EDGES.shape[1] // 3


def _corner(off):
    return off[0] | (off[1] << 1) | (off[2] << 2)


def _edge_ends(e):
    base = EDGE_BASE[e]
    far = base.copy()
    far[EDGE_AXIS[e]] = 1
    return _corner(base), _corner(far)


def _tris(case):
    return [tuple(EDGES[case, 3 * t:3 * t + 3]) for t in range(COUNT[case])]


def _directed(case):
    out = []
    for a, b, c in _tris(case):
        out += [(a, b), (b, c), (c, a)]
    return out


def _boundary(case):
    """directed triangle edges of the cell whose reverse the cell does not use"""
    d = _directed(case)
    return [e for e in d if (e[1], e[0]) not in d]


def _face_of(e0, e1):
    """(axis, side) of the cube face holding both cube edges, or None"""
    c = set(_edge_ends(e0)) | set(_edge_ends(e1))
    for axis in range(3):
        for side in (0, 1):
            if all(((x >> axis) & 1) == side for x in c):
                return axis, side
    return None


def test_committed_header_is_what_the_generator_writes():
    text, max_tris = G.render()
    assert open(G.HEADER).read() == text
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_tables.py"), "--check"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert max_tris == MAX_TRIS == COUNT.max()


def test_padding_and_counts():
    for case in range(256):
        n = COUNT[case]
        assert (EDGES[case, 3 * n:] == 255).all()
        assert (EDGES[case, :3 * n] < 12).all()
        for tri in _tris(case):
            assert len(set(tri)) == 3, (case, tri)
    assert COUNT[0] == COUNT[255] == 0


@pytest.mark.parametrize("case", range(256))
def test_case_uses_exactly_its_crossing_edges(case):
    inside = [(case >> c) & 1 for c in range(8)]
    crossing = {e for e in range(12) if inside[_edge_ends(e)[0]] != inside[_edge_ends(e)[1]]}
    used = {e for tri in _tris(case) for e in tri}
    assert used == crossing


@pytest.mark.parametrize("case", range(256))
def test_interior_edges_pair_up_and_boundary_edges_lie_on_faces(case):
    d = _directed(case)
    assert len(set(d)) == len(d), "a directed edge used twice inside one cell"
    for e in d:
        if (e[1], e[0]) in d:
            continue
        assert _face_of(*e) is not None, (case, e)
    # every crossing edge is an endpoint of exactly two boundary segments (one per face it lies on)
    b = _boundary(case)
    deg = {}
    for u, v in b:
        deg[u] = deg.get(u, 0) + 1
        deg[v] = deg.get(v, 0) + 1
    assert all(x == 2 for x in deg.values()), (case, deg)


def _face_segments(case, axis, side):
    return sorted(e for e in _boundary(case) if _face_of(*e) == (axis, side))


def _mirror_edge(e, axis):
    """the same cube edge seen from the neighbour cell across the face perpendicular to `axis` (on the face, so its
    base offset along `axis` flips 1 <-> 0)"""
    a = EDGE_AXIS[e]
    base = EDGE_BASE[e].copy()
    assert a != axis
    base[axis] = 1 - base[axis]
    u, v = [x for x in range(3) if x != a]
    return 4 * a + base[u] + 2 * base[v]


@pytest.mark.parametrize("axis", range(3))
def test_shared_faces_agree_between_neighbour_cells(axis):
    """The cell's face (axis, 1) is its +axis neighbour's face (axis, 0).  Whatever the rest of either cell, the two
    cut that face along the same segments, in opposite directions (the mesh is closed across cells)."""
    for case in range(256):
        segs = _face_segments(case, axis, 1)
        # the neighbour's corners on the shared face carry the same bits; its other four corners are free
        for rest in range(16):
            nb = 0
            for c in range(8):
                if (c >> axis) & 1:
                    continue
                nb |= ((case >> (c | (1 << axis))) & 1) << c
            free = [c for c in range(8) if (c >> axis) & 1]
            for i, c in enumerate(free):
                nb |= ((rest >> i) & 1) << c
            got = _face_segments(nb, axis, 0)
            want = sorted((_mirror_edge(v, axis), _mirror_edge(u, axis)) for u, v in segs)
            assert got == want, (axis, case, nb, segs, got)


def test_single_corner_triangle_faces_away_from_the_inside_corner():
    """orientation: case 1 (only corner 0 inside) -> one triangle whose normal points to +(1,1,1)"""
    (tri,) = _tris(1)
    mid = [(EDGE_BASE[e] + 0.5 * np.eye(3)[EDGE_AXIS[e]]) for e in tri]
    n = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    assert (n > 0).all()
