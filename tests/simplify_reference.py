"""Test-only numpy restatement of the mesh-simplification contract (include/tt_abi.h, "mesh simplification"): box,
cell keys and cell centres in float32 exactly as the contract writes them, everything after that (quadrics, member
means, the 3x3 solve, the clamp) in float64.  Returns what ops.mesh_simplify returns, as numpy arrays.  The project has
no other implementation to compare with (no CPU mesh library is installed), so this reading of the contract is the
oracle of tests/test_simplify_host.py and tests/test_gpu_simplify.py."""
import functools

import numpy as np

MAX_CLUSTERS = (1 << 21) - 1
F = np.float32


def _unchanged(v, tri, grid):
    return v, tri, {"grid": grid, "cell": 0.0, "n_clusters": len(v), "unchanged": True,
                    "vertex_map": np.arange(len(v), dtype=np.int32)}


def box(v, grid):
    """(lo (3,), h, inv_h) in float32"""
    lo = v.min(0)
    ext = (v.max(0) - lo).max()
    return lo, ext, (ext / F(grid) if ext != 0 else F(0)), (F(grid) / ext if ext != 0 else F(0))


def cell_keys(v, lo, inv_h, grid):
    """(cells (V,3) int64, key (V,) int64): subtract, then multiply, each rounded to float32"""
    t = ((v - lo[None, :]).astype(F) * inv_h).astype(F)
    c = np.clip(np.floor(t).astype(np.int64), 0, grid - 1)
    return c, (c[:, 0] * grid + c[:, 1]) * grid + c[:, 2]


def simplify(v_pos, t_pos_idx, grid, lam=1e-3):
    v = np.ascontiguousarray(v_pos, dtype=F).reshape(-1, 3)
    tri = np.asarray(t_pos_idx, dtype=np.int64).reshape(-1, 3)
    if not 2 <= grid <= 1024:
        raise ValueError("grid out of range")
    if len(v) == 0 or len(tri) == 0:
        return _unchanged(v, tri.astype(np.int32), grid)
    lo, ext, h, inv_h = box(v, grid)
    if ext == 0:
        return _unchanged(v, tri.astype(np.int32), grid)
    _, key = cell_keys(v, lo, inv_h, grid)
    ckey, rank = np.unique(key, return_inverse=True)  # ascending key
    rank = rank.reshape(-1)
    C = len(ckey)
    if C > MAX_CLUSTERS:
        raise ValueError("too many clusters")
    cc = np.stack([ckey // (grid * grid), (ckey // grid) % grid, ckey % grid], 1)
    centre32 = (lo[None, :] + ((cc.astype(F) + F(0.5)) * h).astype(F)).astype(F)
    centre = centre32.astype(np.float64)
    vd = v.astype(np.float64)
    # quadrics: a face counts once per distinct cluster it touches
    r = rank[tri]
    p0, p1, p2 = vd[tri[:, 0]], vd[tri[:, 1]], vd[tri[:, 2]]
    n = np.cross(p1 - p0, p2 - p0)
    l = np.sqrt((n * n).sum(1))
    good = l > 0
    nh = n / np.where(good, l, 1.0)[:, None]
    area = 0.5 * l
    A = np.zeros((C, 3, 3))
    b = np.zeros((C, 3))
    w = np.zeros(C)
    use = [np.ones(len(tri), bool), r[:, 1] != r[:, 0], (r[:, 2] != r[:, 0]) & (r[:, 2] != r[:, 1])]
    for k in range(3):
        sel = use[k] & good
        cl = r[sel, k]
        d = -(nh[sel] * (p0[sel] - centre[cl])).sum(1)
        np.add.at(A, cl, area[sel, None, None] * nh[sel, :, None] * nh[sel, None, :])
        np.add.at(b, cl, (area[sel] * d)[:, None] * nh[sel])
        np.add.at(w, cl, area[sel])
    # member mean
    m = np.zeros((C, 3))
    np.add.at(m, rank, vd - centre[rank])
    m /= np.bincount(rank, minlength=C)[:, None]
    x = m.copy()
    pos = w > 0
    M = A[pos] + (lam * w[pos])[:, None, None] * np.eye(3)[None]
    rhs = lam * w[pos][:, None] * m[pos] - b[pos]
    x[pos] = np.linalg.solve(M, rhs[..., None])[..., 0]
    half = 0.5 * float(h)
    x = np.clip(x, -half, half)
    cpos = (centre + x).astype(F)
    # faces
    distinct = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 2] != r[:, 0])
    s = np.argmin(r, axis=1)
    rot = np.stack([r[np.arange(len(r)), (s + j) % 3] for j in range(3)], 1)
    fkey = (rot[:, 0] << 42) | (rot[:, 1] << 21) | rot[:, 2]
    idx = np.nonzero(distinct)[0]
    _, first = np.unique(fkey[idx], return_index=True)  # first occurrence = smallest original index
    keep = np.sort(idx[first])
    faces = rot[keep]
    cmark = np.zeros(C, bool)
    cmark[faces.reshape(-1)] = True
    new_id = np.cumsum(cmark) - 1
    vertex_map = np.where(cmark[rank], new_id[rank], -1).astype(np.int32)
    info = {"grid": grid, "cell": float(h), "n_clusters": C, "vertex_map": vertex_map, "unchanged": False,
            "centre": centre32[cmark], "rank": rank}
    return cpos[cmark], new_id[faces].astype(np.int32).reshape(-1, 3), info


def dedupe_case():
    """Box [0,3]^3, G = 3: two vertices each in the cells A = (0,0,0), B = (2,0,0), C = (0,2,0), plus the corners
    (0,0,0) and (3,3,3) that make the box exact.  Faces (a0,b0,c0), (b1,c1,a1), (a1,c0,b1): the second is a rotation
    of the first in cluster numbering (dropped), the third has the opposite orientation (kept)."""
    v = np.array([[0.2, 0.3, 0.4], [0.6, 0.5, 0.7],   # a0, a1
                  [2.2, 0.3, 0.4], [2.6, 0.5, 0.2],   # b0, b1
                  [0.2, 2.3, 0.4], [0.6, 2.5, 0.3],   # c0, c1
                  [0.0, 0.0, 0.0], [3.0, 3.0, 3.0]], dtype=F)
    tri = np.array([[0, 2, 4], [3, 5, 1], [1, 4, 3]], dtype=np.int32)
    return v, tri


def single_triangle():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 1.0, 0.3]], dtype=F)
    return v, np.array([[0, 1, 2]], dtype=np.int32)


# the cases of tests/test_gpu_simplify.py (tools/time_simplify.py records the GPU's deviation on the same ones)
CASES = [("sphere24", 4), ("sphere24", 8), ("sphere24", 12),
         ("sphere32", 2),  # segments of ~456 pairs: 8 strides per wave
         ("torus32", 12),
         ("blobs32", 8),  # clusters that lose every face: the vertex compaction path
         ("hand", 2), ("hand", 3), ("hand", 5),  # a degenerate face, a non-manifold edge, an unreferenced vertex
         ("dedupe", 3), ("triangle", 2)]


@functools.lru_cache(maxsize=None)
def source_mesh(name):
    """(v_pos float32, t_pos_idx) of a case, computed once: marching-cubes meshes mapped to [-1, 1]"""
    import mc_reference as MC
    import mesh_reference as M
    if name == "hand":
        return M.hand_mesh()
    if name == "dedupe":
        return dedupe_case()
    if name == "triangle":
        return single_triangle()
    field = {"sphere24": lambda: M.sphere_field(24), "sphere32": lambda: M.sphere_field(32),
             "torus32": lambda: M.torus_field(32), "blobs32": lambda: M.blobs_field(32)}[name]()
    mc = MC.marching_cubes(field)
    return mc.v_pos * 2 - 1, mc.t_pos_idx
