"""Test-only numpy oracle of the marching-tetrahedra contract (include/tt_abi.h, "marching tetrahedra"; DESIGN.md
section 3b-mt): the static tables of a tet grid (unique sorted edges, each tet's rows in them, the vertex -> incident-edge
CSR) and the extraction on them (crossing edges in `edges` order, one-triangle tets before two-triangle tets, the
interpolation in fp32 in the written order).  tests/test_tets_host.py pins it to the reference's
MarchingTetrahedraHelper (tests/golden/reference_tets.npz); the GPU tests compare the HIP kernels with it."""
import numpy as np

BASE_EDGES = np.array([0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3])  # threestudio/models/isosurface.py:175
# isosurface.py:141-169, as data
TRI_TABLE = np.array([
    [-1, -1, -1, -1, -1, -1], [1, 0, 2, -1, -1, -1], [4, 0, 3, -1, -1, -1], [1, 4, 2, 1, 3, 4],
    [3, 1, 5, -1, -1, -1], [2, 3, 0, 2, 5, 3], [1, 4, 0, 1, 5, 4], [4, 2, 5, -1, -1, -1],
    [4, 5, 2, -1, -1, -1], [4, 1, 0, 4, 5, 1], [3, 2, 0, 3, 5, 2], [1, 3, 5, -1, -1, -1],
    [4, 1, 2, 4, 3, 1], [3, 0, 4, -1, -1, -1], [2, 0, 1, -1, -1, -1], [-1, -1, -1, -1, -1, -1]], dtype=np.int64)
TRI_COUNT = np.array([0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0], dtype=np.int64)


class Tables:
    """tet_tables' result: edges (Ne,2), tet_edge (Nt,6), vert_ptr (Nv+1), vert_col (2 Ne), all int64"""

    def __init__(self, edges, tet_edge, vert_ptr, vert_col):
        self.edges, self.tet_edge, self.vert_ptr, self.vert_col = edges, tet_edge, vert_ptr, vert_col


def tet_tables(indices, n_vertices):
    idx = np.asarray(indices, dtype=np.int64)
    pairs = np.sort(idx[:, BASE_EDGES].reshape(-1, 2), axis=1)
    uniq, inverse = np.unique(pairs[:, 0] * n_vertices + pairs[:, 1], return_inverse=True)
    edges = np.stack([uniq // n_vertices, uniq % n_vertices], axis=1)
    Ne = len(edges)
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    eid = np.concatenate([np.arange(Ne), np.arange(Ne)])
    order = np.lexsort((eid, src))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n_vertices))])
    return Tables(edges, inverse.reshape(-1, 6), ptr, eid[order])


class MT:
    """marching_tets' result: v_pos (V,3) float32, t_pos_idx (T,3) int32, the tables, and per vertex its row of
    `edges` (edge_id) for re-implementations of the interpolation"""

    def __init__(self, v_pos, t_pos_idx, tables, edge_id):
        self.v_pos, self.t_pos_idx, self.tables, self.edge_id = v_pos, t_pos_idx, tables, edge_id
        self.a, self.b = tables.edges[edge_id, 0], tables.edges[edge_id, 1]


def marching_tets(pos, level, indices, tables=None):
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    level = np.ascontiguousarray(level, dtype=np.float32).reshape(-1)
    idx = np.asarray(indices, dtype=np.int64)
    tb = tables if tables is not None else tet_tables(idx, len(pos))
    with np.errstate(invalid="ignore"):
        occ = level > 0  # a NaN level is unoccupied
    cross = occ[tb.edges[:, 0]] != occ[tb.edges[:, 1]]
    edge_id = np.nonzero(cross)[0]
    vid = np.cumsum(cross) - cross  # exclusive: the vertex of a crossing edge
    a, b = tb.edges[edge_id, 0], tb.edges[edge_id, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        sa, sb = level[a], level[b]
        den = sa - sb
        wa, wb = -sb / den, sa / den
        v = pos[a] * wa[:, None] + pos[b] * wb[:, None]
    case = (occ[idx] * (1 << np.arange(4))).sum(1)
    n = TRI_COUNT[case]
    one, two = np.nonzero(n == 1)[0], np.nonzero(n == 2)[0]
    f1 = vid[np.take_along_axis(tb.tet_edge[one], TRI_TABLE[case[one]][:, :3], axis=1)].reshape(-1, 3)
    f2 = vid[np.take_along_axis(tb.tet_edge[two], TRI_TABLE[case[two]][:, :6], axis=1)].reshape(-1, 3)
    return MT(v.astype(np.float32), np.concatenate([f1, f2]).astype(np.int32), tb, edge_id)


def vertex_positions_torch(mt, pos, level):
    """The interpolation in torch (any dtype, autograd-connected to pos / level) on the oracle's crossing edges: the
    float32 / float64 references of the gradient tests."""
    import torch
    a, b = torch.as_tensor(mt.a), torch.as_tensor(mt.b)
    flat = level.reshape(-1)
    sa, sb = flat[a], flat[b]
    den = sa - sb
    return pos[a] * (-sb / den)[:, None] + pos[b] * (sa / den)[:, None]


def backward(mt, pos, level, grad_v):
    """d sum(grad_v * v_pos) / d (level, pos) in float64, by the formulas of the contract"""
    pos, level, g = (np.asarray(x, dtype=np.float64) for x in (pos, level, grad_v))
    level = level.reshape(-1)
    a, b = mt.a, mt.b
    sa, sb = level[a], level[b]
    den = sa - sb
    gd = (g * (pos[b] - pos[a])).sum(1)
    g_level, g_pos = np.zeros_like(level), np.zeros_like(pos)
    np.add.at(g_level, a, gd * -sb / den ** 2)
    np.add.at(g_level, b, gd * sa / den ** 2)
    np.add.at(g_pos, a, g * (-sb / den)[:, None])
    np.add.at(g_pos, b, g * (sa / den)[:, None])
    return g_level, g_pos
