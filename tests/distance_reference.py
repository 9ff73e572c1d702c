"""float64 restatement of the point-to-mesh distance contract (include/tt_abi.h, "point-to-mesh distance"), written
independently of the kernel's Voronoi-region code: project onto the plane and test inside, else the minimum over the
three edge segments (which is also what a degenerate triangle is).  CPU torch, chunked.  Besides: Ericson's formulation
in float64 (a second opinion), a Python mirror of the kernel's binning, ring search and stopping rule, the sampler's
restatement, and the hand-built meshes and the point set of tests/test_gpu_mesh_distance.py."""
import numpy as np
import torch

F64 = torch.float64


def _dot(x, y):
    return (x * y).sum(-1)


def _segment_t(P, X, Y):
    e = Y - X
    ee = _dot(e, e)
    t = _dot(P - X, e) / torch.where(ee > 0, ee, torch.ones_like(ee))
    return torch.where(ee > 0, t.clamp(0, 1), torch.zeros_like(t))


def closest_point(P, A, B, C):
    """Closest point on the triangles (A, B, C) to P, all (..., 3) float64 and broadcastable: (d2, bary (..., 3)).
    Differentiable (every division has a safe denominator)."""
    P, A, B, C = torch.broadcast_tensors(P, A, B, C)
    ab, ac, ap = B - A, C - A, P - A
    n = torch.linalg.cross(ab, ac)
    nn = _dot(n, n)
    safe = torch.where(nn > 0, nn, torch.ones_like(nn))
    v = _dot(torch.linalg.cross(ap, ac), n) / safe
    w = _dot(torch.linalg.cross(ab, ap), n) / safe
    u = 1 - v - w
    inside = (nn > 0) & (u >= 0) & (v >= 0) & (w >= 0)
    zero = torch.zeros_like(u)
    t1, t2, t3 = _segment_t(P, A, B), _segment_t(P, B, C), _segment_t(P, C, A)
    cands = [torch.stack([1 - t1, t1, zero], -1), torch.stack([zero, 1 - t2, t2], -1), torch.stack([t3, zero, 1 - t3], -1)]

    def d2_of(b):
        c = b[..., 0:1] * A + b[..., 1:2] * B + b[..., 2:3] * C
        return _dot(P - c, P - c)

    bary, best = cands[0], d2_of(cands[0])
    for b in cands[1:]:
        d = d2_of(b)
        take = d < best
        bary, best = torch.where(take[..., None], b, bary), torch.where(take, d, best)
    face_b = torch.stack([u, v, w], -1)
    bary = torch.where(inside[..., None], face_b, bary)
    return d2_of(bary), bary


def ericson(P, A, B, C):
    """Real-Time Collision Detection 5.1.5 in float64 (numpy, elementwise over equal-shaped (..., 3) arrays): d2.
    For triangles with area only."""
    P, A, B, C = (np.asarray(x, np.float64) for x in (P, A, B, C))
    ab, ac, ap, bp, cp = B - A, C - A, P - A, P - B, P - C
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        den = va + vb + vc
        v, w = vb / den, vc / den  # the face region, then overwritten in reverse priority
        m = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = np.where(m, 1 - t, v), np.where(m, t, w)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = np.where(m, 0.0, v), np.where(m, d2 / (d2 - d6), w)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = np.where(m, d1 / (d1 - d3), v), np.where(m, 0.0, w)
        m = (d6 >= 0) & (d5 <= d6)
        v, w = np.where(m, 0.0, v), np.where(m, 1.0, w)
        m = (d3 >= 0) & (d4 <= d3)
        v, w = np.where(m, 1.0, v), np.where(m, 0.0, w)
        m = (d1 <= 0) & (d2 <= 0)
        v, w = np.where(m, 0.0, v), np.where(m, 0.0, w)
    c = A + v[..., None] * ab + w[..., None] * ac
    return dot(P - c, P - c)


def corners(v_pos, t_pos_idx):
    v = torch.as_tensor(np.asarray(v_pos), dtype=F64)
    t = torch.as_tensor(np.asarray(t_pos_idx), dtype=torch.int64)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def pair_matrix(points, v_pos, t_pos_idx, max_pairs=250_000):
    """d2 of every (point, triangle) pair, (N, T) float64, in chunks of points."""
    P = torch.as_tensor(np.asarray(points), dtype=F64)
    A, B, C = corners(v_pos, t_pos_idx)
    step = max(1, max_pairs // max(len(A), 1))
    return torch.cat([closest_point(P[i:i + step, None, :], A[None], B[None], C[None])[0]
                      for i in range(0, len(P), step)]) if len(P) else torch.zeros(0, len(A), dtype=F64)


def distance_to_faces(points, v_pos, t_pos_idx, faces):
    """float64 distance of point i to face faces[i] alone."""
    P = torch.as_tensor(np.asarray(points), dtype=F64)
    A, B, C = corners(v_pos, np.asarray(t_pos_idx)[np.asarray(faces)])
    return closest_point(P, A, B, C)[0].sqrt().numpy()


# ---------------------------------------------------------------------------------------------------------------
# the kernel's grid, ring search and stopping rule, mirrored
def default_grid(n_faces):
    return int(min(max(int(np.ceil(np.sqrt(float(n_faces)) / 8.0)), 1), 256))


def box(v_pos, G):
    v = np.asarray(v_pos, np.float32)
    lo = v.min(0)
    ext = (v.max(0) - lo).max()
    h = ext / np.float32(G)
    inv_h = np.float32(G) / ext if ext > 0 else np.float32(0)
    return lo, ext, np.float32(h), np.float32(inv_h)


def cell(x, lo, inv_h, G):
    c = np.floor((np.asarray(x, np.float32) - lo) * inv_h).astype(np.int64)
    return np.clip(c, 0, G - 1)


def grid_search(points, v_pos, t_pos_idx, G, D=None):
    """The query as the kernel runs it: triangles binned by the cells of their boxes' corners, Chebyshev rings around
    the cell of the clamped point, stop when the best d2 is STRICTLY below (1 - 2^-16) |p - q|^2 + (max(r - 1/64, 0) h)^2.
    Pair distances from D (N, T) (default: pair_matrix); returns (d2 (N,), face (N,)), the lexicographic minimum."""
    points = np.asarray(points, np.float32)
    v, tri = np.asarray(v_pos, np.float32), np.asarray(t_pos_idx)
    D = pair_matrix(points, v, tri).numpy() if D is None else np.asarray(D)
    lo, ext, h, inv_h = box(v, G)
    p3 = v[tri]
    c0, c1 = cell(p3.min(1), lo, inv_h, G), cell(p3.max(1), lo, inv_h, G)
    cells = {}
    for f in range(len(tri)):
        for z in range(c0[f, 0], c1[f, 0] + 1):
            for y in range(c0[f, 1], c1[f, 1] + 1):
                for x in range(c0[f, 2], c1[f, 2] + 1):
                    cells.setdefault((z, y, x), []).append(f)
    out_d2, out_f = np.full(len(points), np.inf), np.full(len(points), -1, np.int64)
    for i, p in enumerate(points):
        q = np.minimum(np.maximum(p, lo), lo + ext)
        c = cell(q, lo, inv_h, G)
        pq2 = float(((p.astype(np.float64) - q.astype(np.float64)) ** 2).sum())
        best, bf = np.inf, np.iinfo(np.int64).max
        rmax = int(max(c.max(), (G - 1 - c).max()))
        for r in range(rmax + 1):
            for z in range(max(c[0] - r, 0), min(c[0] + r, G - 1) + 1):
                for y in range(max(c[1] - r, 0), min(c[1] + r, G - 1) + 1):
                    for x in range(max(c[2] - r, 0), min(c[2] + r, G - 1) + 1):
                        if max(abs(z - c[0]), abs(y - c[1]), abs(x - c[2])) != r:
                            continue
                        for f in cells.get((z, y, x), ()):
                            if D[i, f] < best or (D[i, f] == best and f < bf):
                                best, bf = D[i, f], f
            rr = max(r - 1.0 / 64.0, 0.0) * float(h)
            if best < pq2 * (1.0 - 2.0 ** -16) + rr * rr:
                break
        out_d2[i], out_f[i] = best, bf
    return out_d2, out_f


# ---------------------------------------------------------------------------------------------------------------
# the sampler
def face_k(v_pos, t_pos_idx, spacing):
    """(k (T,) int64, L / spacing (T,) float64): k = max(1, ceil(L / spacing)) with L the fp32 longest edge, every
    operation rounded to fp32."""
    v = np.asarray(v_pos, np.float32)[np.asarray(t_pos_idx)]
    l2 = np.zeros(len(v), np.float32)
    for e in range(3):
        d = v[:, (e + 1) % 3] - v[:, e]
        sq = d * d
        l2 = np.maximum(l2, (sq[:, 0] + sq[:, 1]) + sq[:, 2])
    L = np.sqrt(l2)
    ratio = L / np.float32(spacing)
    return np.maximum(np.ceil(ratio), 1).astype(np.int64), ratio.astype(np.float64)


def surface_samples(v_pos, t_pos_idx, spacing):
    """(points (S,3) float64, face (S,)): a + (i/k)(b - a) + (j/k)(c - a), face-major, then i, then j."""
    v = np.asarray(v_pos, np.float64)[np.asarray(t_pos_idx)]
    ks, _ = face_k(v_pos, t_pos_idx, spacing)
    pts, faces = [], []
    for f, k in enumerate(ks):
        i, j = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij")
        keep = i + j <= k
        i, j = i[keep], j[keep]  # row-major: ascending i, then j
        a, b, c = v[f]
        pts.append(a + (i / k)[:, None] * (b - a) + (j / k)[:, None] * (c - a))
        faces.append(np.full(len(i), f, np.int64))
    return np.concatenate(pts), np.concatenate(faces)


# ---------------------------------------------------------------------------------------------------------------
# meshes and points of the GPU tests
def _cluster(centre, rng, n=8, size=0.15):
    v = centre + rng.uniform(-size, size, (3 * n, 3))
    return v.astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def two_clusters():
    """Two clusters of 8 small triangles, 1.8 apart along x."""
    rng = np.random.default_rng(11)
    va, ta = _cluster(np.array([-0.9, 0.0, 0.0]), rng)
    vb, tb = _cluster(np.array([0.9, 0.0, 0.0]), rng)
    return np.concatenate([va, vb]), np.concatenate([ta, tb + len(va)]).astype(np.int32)


def spanning():
    """40 small triangles in [-1, 1]^3 and, in the middle of the face list, one triangle that spans the whole cube."""
    rng = np.random.default_rng(12)
    parts = [_cluster(rng.uniform(-0.8, 0.8, 3), rng, n=4, size=0.1) for _ in range(10)]
    v = np.concatenate([p[0] for p in parts] + [np.array([[-1, -1, -1], [1, 1, -1], [0, 1, 1]], np.float32)])
    t = np.concatenate([p[1] + 12 * i for i, p in enumerate(parts)])
    big = np.array([[len(v) - 3, len(v) - 2, len(v) - 1]], np.int32)
    return v, np.concatenate([t[:20], big, t[20:]]).astype(np.int32)


def one_octant():
    """Every triangle in one octant, plus one far vertex (unreferenced) that stretches the cube: at G = 2 one cell holds
    every triangle."""
    rng = np.random.default_rng(13)
    v, t = _cluster(np.array([0.25, 0.25, 0.25]), rng, n=12, size=0.2)
    return np.concatenate([v, np.array([[1.9, 1.9, 1.9]], np.float32)]), t


def query_points(v_pos, t_pos_idx, seed=0):
    """The point set of the GPU tests: 1 500 uniform points in [-1.5, 1.5]^3, up to 200 vertices, centroids and edge
    midpoints (exact zeros and ties), the same scaled by 1.001, one point at distance 1e3; float32.  The NaN and inf
    rows are appended by the tests that want them."""
    rng = np.random.default_rng(seed)
    v, tri = np.asarray(v_pos, np.float32), np.asarray(t_pos_idx)
    pv = v[rng.permutation(len(v))[:200]]
    f = rng.permutation(len(tri))[:200]
    cen = v[tri[f]].mean(1)
    mid = 0.5 * (v[tri[f, 0]] + v[tri[f, 1]])
    on = np.concatenate([pv, cen, mid]).astype(np.float32)
    far = np.array([[600.0, -700.0, 400.0]], np.float32)
    return np.concatenate([rng.uniform(-1.5, 1.5, (1500, 3)).astype(np.float32), on, on * np.float32(1.001), far])
