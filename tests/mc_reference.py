"""Test-only numpy oracle of the marching-cubes contract (include/tt_abi.h, "marching cubes").

It reads the case tables from the committed header (triplaneturbo_amd/csrc/tt_mc_tables.h, proven by
tests/test_isosurface_tables.py), so what it checks in the HIP kernels is the rest: the crossing masks, the vertex /
triangle scans, the interpolation, the edge -> (owner point, axis) -> vertex id mapping and the canonical order.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "triplaneturbo_amd", "csrc", "tt_mc_tables.h")


def load_tables(path=HEADER):
    """(tri_count (256,), tri_edges (256, 3 * max_tris)) from the header"""
    src = open(path).read()
    max_tris = int(re.search(r"#define\s+TT_MC_MAX_TRIS\s+(\d+)", src).group(1))
    body = re.search(r"tt_mc_tri_count\[256\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    count = np.array([int(x) for x in re.findall(r"\d+", body)], dtype=np.int64)
    body = re.search(r"tt_mc_tri_edges\[256\]\[\d+\]\s*=\s*\{(.*?)\n\};", src, re.S).group(1)
    rows = re.findall(r"\{([^}]*)\}", body)
    edges = np.array([[int(x) for x in r.split(",")] for r in rows], dtype=np.int64)
    assert count.shape == (256,) and edges.shape == (256, 3 * max_tris)
    return count, edges


# edge e -> (axis, base corner offset (di, dj, dk)): tools/gen_mc_tables.py
EDGE_AXIS = np.array([e // 4 for e in range(12)])
EDGE_BASE = np.zeros((12, 3), dtype=np.int64)
for _e in range(12):
    _a, _r = divmod(_e, 4)
    _u, _v = [x for x in range(3) if x != _a]
    EDGE_BASE[_e, _u], EDGE_BASE[_e, _v] = _r & 1, _r >> 1


class MC:
    """Result of marching_cubes(): v_pos (V,3) float32, t_pos_idx (T,3) int32, and per vertex the grid points of its
    edge (p0, p1: linear indices, axis) for re-implementations of the interpolation."""

    def __init__(self, v_pos, t_pos_idx, p0, p1, axis, res):
        self.v_pos, self.t_pos_idx, self.p0, self.p1, self.axis, self.res = v_pos, t_pos_idx, p0, p1, axis, res


def marching_cubes(level, deformation=None, isovalue=0.0, tables=None):
    level = np.ascontiguousarray(level, dtype=np.float32)
    R = level.shape[0]
    assert level.shape == (R, R, R) and R >= 2
    count, edges = tables if tables is not None else load_tables()
    iso = np.float32(isovalue)
    inside = level < iso
    cross = np.zeros((R, R, R, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    cross = cross.reshape(-1, 3)
    mask = (cross[:, 0] * 1 + cross[:, 1] * 2 + cross[:, 2] * 4).astype(np.int64)
    nv = cross.sum(1)
    vbase = np.concatenate([[0], np.cumsum(nv)[:-1]]).astype(np.int64)
    # vertices in (owner point, axis) order
    pt, ax = np.nonzero(cross)
    strides = np.array([R * R, R, 1])
    p1 = pt + strides[ax]
    flat = level.reshape(-1)
    s0, s1 = flat[pt], flat[p1]
    t = (iso - s0) / (s1 - s0)
    ijk = np.stack(np.unravel_index(pt, (R, R, R)), -1).astype(np.float32)
    ijk1 = ijk.copy()
    ijk1[np.arange(len(pt)), ax] += np.float32(1)
    if deformation is not None:
        d = np.ascontiguousarray(deformation, dtype=np.float32).reshape(-1, 3)
        a = ijk + d[pt]
        b = ijk1 + d[p1]
    else:
        a = ijk + np.float32(0)
        b = ijk1 + np.float32(0)
    v = (a + t[:, None] * (b - a)) / np.float32(R - 1)
    # triangles in (cell, table) order
    ins = inside.astype(np.int64)
    case = np.zeros((R - 1, R - 1, R - 1), dtype=np.int64)
    for c in range(8):
        di, dj, dk = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[di:R - 1 + di, dj:R - 1 + dj, dk:R - 1 + dk] << c
    cell_ijk = np.stack(np.meshgrid(*[np.arange(R - 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    case = case.reshape(-1)
    n = count[case]
    max_tris = edges.shape[1] // 3
    slot = np.arange(max_tris)[None, :] < n[:, None]
    cell, s = np.nonzero(slot)
    te = edges[case[cell]].reshape(-1, max_tris, 3)[np.arange(len(cell)), s]  # (T, 3) edge ids
    owner = cell_ijk[cell][:, None, :] + EDGE_BASE[te]
    own = (owner * strides).sum(-1)
    a = EDGE_AXIS[te]
    rank = np.zeros_like(a)
    rank += (a > 0) & ((mask[own] & 1) != 0)
    rank += (a > 1) & ((mask[own] & 2) != 0)
    tri = vbase[own] + rank
    return MC(v.astype(np.float32), tri.astype(np.int32), pt, p1, ax, R)


def vertex_positions_torch(mc, level, deformation, isovalue):
    """The interpolation of section 1 in torch (any dtype, autograd-connected to level / deformation) on the oracle's
    edges: the float64 arbiter of the gradient tests."""
    import torch
    R = mc.res
    flat = level.reshape(-1)
    p0 = torch.as_tensor(mc.p0, device=level.device)
    p1 = torch.as_tensor(mc.p1, device=level.device)
    s0, s1 = flat[p0], flat[p1]
    t = (isovalue - s0) / (s1 - s0)
    ijk = torch.as_tensor(np.stack(np.unravel_index(mc.p0, (R, R, R)), -1), dtype=level.dtype, device=level.device)
    ijk1 = ijk.clone()
    ijk1[torch.arange(len(p0)), torch.as_tensor(mc.axis)] += 1
    if deformation is not None:
        d = deformation.reshape(-1, 3)
        a, b = ijk + d[p0], ijk1 + d[p1]
    else:
        a, b = ijk, ijk1
    return (a + t[:, None] * (b - a)) / (R - 1)


# ---- mesh checks that do not use the table ----
def directed_edges(tri):
    tri = np.asarray(tri, dtype=np.int64)
    return np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])


def edge_key(e, n):
    return e[:, 0] * n + e[:, 1]


def euler_characteristic(v_pos, tri):
    d = directed_edges(tri)
    und = np.unique(np.sort(d, 1), axis=0)
    return len(v_pos) - len(und) + len(tri)


def unmatched_directed_edges(tri, n_vert):
    """directed edges (u, v) whose count differs from the count of (v, u)"""
    d = directed_edges(tri)
    keys, cnt = np.unique(edge_key(d, n_vert), return_counts=True)
    rev = np.unique(edge_key(d[:, ::-1], n_vert), return_counts=True)
    fwd = dict(zip(keys.tolist(), cnt.tolist()))
    bwd = dict(zip(rev[0].tolist(), rev[1].tolist()))
    return [k for k in fwd if fwd[k] != bwd.get(k, 0)]


def signed_volume(v_pos, tri):
    v = np.asarray(v_pos, dtype=np.float64)[np.asarray(tri, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def connected_components(n_vert, tri):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components as cc
    d = directed_edges(tri)
    g = sp.coo_matrix((np.ones(len(d)), (d[:, 0], d[:, 1])), shape=(n_vert, n_vert))
    return cc(g, directed=False)[0]
