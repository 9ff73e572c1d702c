"""float64 restatement of the winding-number contract (include/tt_abi.h, "winding number"): the pair, the exact sum,
the tree (keys, sorted order, node table), the (l, m) walk as a pure-Python model, a level-by-level evaluation of the
same tree that also reports every point's smallest decision margin, the MeshOBJ / ce_pq_loss / ShapeLoss formulas, and
the meshes and point sets of tests/test_gpu_winding.py.  numpy throughout; `dtype=np.float32` restates the pair in fp32
(the running sum stays a double, as in the kernel).  Only the keys mirror the kernel's fp32 arithmetic operation by
operation: a face must land in the same leaf on both sides."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as D  # noqa: E402
import simplify_reference as S  # noqa: E402

F32 = np.float32
FOUR_PI = 4.0 * np.pi


# ---------------------------------------------------------------------------------------------------------------
# the pair and the exact sum
def solid_angle(P, A, B, C, dtype=np.float64):
    """Omega of the triangles (A, B, C) seen from P, all (..., 3) and broadcastable (Van Oosterom-Strackee); num == 0
    gives exactly 0."""
    P, A, B, C = (np.asarray(x, dtype) for x in (P, A, B, C))
    a, b, c = A - P, B - P, C - P
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    num = dot(a, np.cross(b, c))
    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
    return np.where(num == 0, dtype(0), dtype(2) * np.arctan2(num, den))


def atan2_f32(y, x):
    """The kernel's own atan2 (wind_atan2, csrc/tt_wind.hip) operation by operation in numpy float32 (without the
    compiler's FMA contraction): t = (mn - b mx) / (b mn + mx) with b = [mn > tan(pi/8) mx], Cephes' atanf polynomial,
    then the octant.  For y != 0."""
    y, x = np.asarray(y, F32), np.asarray(x, F32)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    b = (mn > F32(0.41421356) * mx).astype(F32)
    t = (mn - b * mx) / (b * mn + mx)
    z = t * t
    poly = ((F32(8.05374449538e-2) * z - F32(1.38776856032e-1)) * z + F32(1.99777106478e-1)) * z - F32(3.33329491539e-1)
    a = b * F32(0.78539816) + (t + t * z * poly)
    a = np.where(ay > ax, F32(1.57079633) - a, a)
    a = np.where(x < 0, F32(3.14159265) - a, a)
    return np.copysign(a, y).astype(F32)


def exact(points, v_pos, t_pos_idx, dtype=np.float64, max_pairs=1_000_000):
    """w (N,) float64: the sum over every face, in chunks of points; the pairs in `dtype`, the sum in float64."""
    P = np.asarray(points, dtype)
    v = np.asarray(v_pos, dtype)[np.asarray(t_pos_idx)]
    step = max(1, max_pairs // max(len(v), 1))
    out = [solid_angle(P[i:i + step, None, :], v[None, :, 0], v[None, :, 1], v[None, :, 2], dtype).astype(np.float64).sum(1)
           for i in range(0, len(P), step)]
    return (np.concatenate(out) if out else np.zeros(0)) / FOUR_PI


# ---------------------------------------------------------------------------------------------------------------
# the tree
def default_levels(n_faces):
    return next((L for L in range(6) if 6 * 4 ** L >= n_faces), 6)  # the smallest L with 6 * 4^L >= T, at most 6


def box(v_pos, L):
    v = np.asarray(v_pos, F32)
    lo = v.min(0)
    ext = (v.max(0) - lo).max()
    inv_h = F32(1 << L) / ext if ext > 0 else F32(0)
    return lo, ext, F32(inv_h)


def morton(cells, L):
    """Bit b of (c_x, c_y, c_z) at bits 3b+2, 3b+1, 3b."""
    cells = np.asarray(cells, np.int64)
    key = np.zeros(len(cells), np.int64)
    for b in range(L):
        key |= (((cells[:, 0] >> b) & 1) << 2 | ((cells[:, 1] >> b) & 1) << 1 | ((cells[:, 2] >> b) & 1)) << (3 * b)
    return key


def face_keys(v_pos, t_pos_idx, L):
    """Morton key of the leaf cell of every face's centroid, with the kernel's fp32 operations: ((a + b) + c) * (1/3)."""
    v = np.asarray(v_pos, F32)[np.asarray(t_pos_idx)]
    lo, ext, inv_h = box(v_pos, L)
    cen = ((v[:, 0] + v[:, 1]) + v[:, 2]) * F32(0.33333334)
    return morton(D.cell(cen, lo, inv_h, 1 << L), L)


def point_keys(points, v_pos, L):
    lo, ext, inv_h = box(v_pos, L)
    q = np.minimum(np.maximum(np.asarray(points, F32), lo), lo + ext)
    return morton(D.cell(q, lo, inv_h, 1 << L), L)


class Tree:
    """order (T,): the face of every sorted row; leaf_ptr (8^L + 1); per level l the arrays N (8^l,3), c (8^l,3),
    r (8^l,) (-1: empty), A (8^l,), begin / end (8^l,) and n_bar / len_sum (the fp32 bars of tests (c): see bars())."""

    def __init__(self, v_pos, t_pos_idx, L):
        self.L = L
        self.v32 = np.asarray(v_pos, F32)
        self.tri = np.asarray(t_pos_idx, np.int64)
        self.ext = float(box(v_pos, L)[1])
        keys = face_keys(v_pos, t_pos_idx, L)
        self.order = np.argsort(keys, kind="stable")
        self.leaf_ptr = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=8 ** L))]).astype(np.int64)
        corners = self.v32.astype(np.float64)[self.tri[self.order]]  # sorted rows
        self.corners = corners
        e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
        n = 0.5 * np.cross(e1, e2)
        area = np.linalg.norm(n, axis=1)
        cen = corners.mean(1)
        edge_len = np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)
        n_leaf = 8 ** L
        leaf_of = np.repeat(np.arange(n_leaf), np.diff(self.leaf_ptr))
        lv = {"N": np.zeros((n_leaf, 3)), "c": np.zeros((n_leaf, 3)), "r": np.full(n_leaf, -1.0), "A": np.zeros(n_leaf),
              "begin": self.leaf_ptr[:-1].copy(), "end": self.leaf_ptr[1:].copy(), "len_sum": np.zeros(n_leaf)}
        np.add.at(lv["N"], leaf_of, n)
        np.add.at(lv["A"], leaf_of, area)
        np.add.at(lv["len_sum"], leaf_of, edge_len)
        S_, M_ = np.zeros((n_leaf, 3)), np.zeros((n_leaf, 3))
        np.add.at(S_, leaf_of, area[:, None] * cen)
        np.add.at(M_, leaf_of, cen)
        count = np.diff(self.leaf_ptr)
        occ = count > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            lv["c"] = np.where((lv["A"] > 0)[:, None], S_ / lv["A"][:, None], M_ / np.maximum(count, 1)[:, None])
        lv["c"][~occ] = 0
        dist = np.linalg.norm(corners - lv["c"][leaf_of][:, None, :], axis=2).max(1) if len(corners) else np.zeros(0)
        np.maximum.at(lv["r"], leaf_of, dist)
        self.levels = {L: lv}
        for l in range(L - 1, -1, -1):
            ch = self.levels[l + 1]
            n_l = 8 ** l
            occ_k = (ch["r"] >= 0).reshape(n_l, 8)
            A_k, c_k, r_k = ch["A"].reshape(n_l, 8), ch["c"].reshape(n_l, 8, 3), ch["r"].reshape(n_l, 8)
            A = (A_k * occ_k).sum(1)
            n_occ = occ_k.sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                c = np.where((A > 0)[:, None], ((A_k * occ_k)[:, :, None] * c_k).sum(1) / A[:, None],
                             (c_k * occ_k[:, :, None]).sum(1) / np.maximum(n_occ, 1)[:, None])
            c[n_occ == 0] = 0
            reach = np.where(occ_k, np.linalg.norm(c[:, None, :] - c_k, axis=2) + r_k, -1.0)
            self.levels[l] = {"N": ch["N"].reshape(n_l, 8, 3).sum(1), "c": c, "r": reach.max(1), "A": A,
                              "begin": ch["begin"].reshape(n_l, 8)[:, 0], "end": ch["end"].reshape(n_l, 8)[:, 7],
                              "len_sum": ch["len_sum"].reshape(n_l, 8).sum(1)}

    def bars(self, l):
        """fp32 bars of a level's (N, c, r) against this float64 table, from the number format alone (eps = 2^-23,
        Lm = the mesh's largest |coordinate|): a face's area vector is a difference of products of fp32 edge
        components, each product within eps |e1||e2| <= 2 eps Lm (|e1| + |e2|) / 2 and each edge within eps Lm of its
        exact value, so |dN| <= 8 eps Lm sum_f (|e1| + |e2|) with room for the stored rounding; c is a weighted mean of
        fp32 centroids (each within 4 eps Lm) with weights within a few eps, rounded to fp32 once per level:
        16 eps Lm (L + 1); r adds the rounding of c, of one distance and of one sum per level: 32 eps Lm (L + 1)."""
        eps, Lm = 2.0 ** -23, float(np.abs(self.v32).max())
        lv = self.levels[l]
        return 8 * eps * Lm * lv["len_sum"], 16 * eps * Lm * (self.L + 1), 32 * eps * Lm * (self.L + 1)


def walk(L, is_near):
    """The (l, m) rule of the kernel as a generator: yields every visited node (l, m); is_near(l, m) says whether the
    node is opened (an inner node is then descended, a leaf summed) -- empty and far nodes return False."""
    l, m = 0, 0
    while True:
        yield l, m
        if is_near(l, m) and l < L:
            l, m = l + 1, 8 * m
            continue
        while l > 0 and (m & 7) == 7:
            m >>= 3
            l -= 1
        if l == 0:
            return
        m += 1


def fast_one(tree, p, beta):
    """w of ONE point by the pure-Python walk, float64."""
    p = np.asarray(p, np.float64)
    acc = 0.0

    def is_near(l, m):
        lv = tree.levels[l]
        if lv["r"][m] < 0:
            return False
        d = np.linalg.norm(lv["c"][m] - p)
        return not d > beta * lv["r"][m]

    for l, m in walk(tree.L, is_near):
        lv = tree.levels[l]
        if lv["r"][m] < 0:
            continue
        dvec = lv["c"][m] - p
        d = np.linalg.norm(dvec)
        if d > beta * lv["r"][m]:
            t = lv["N"][m] @ dvec
            acc += 0.0 if t == 0 else t / d ** 3
        elif l == tree.L:
            rows = tree.corners[lv["begin"][m]:lv["end"][m]]
            acc += solid_angle(p, rows[:, 0], rows[:, 1], rows[:, 2]).sum()
    return acc / FOUR_PI


def fast(tree, points, beta):
    """(w (N,) float64, margin (N,)): the same tree evaluated level by level over all points at once (float64 does not
    care about the order of the sum); margin = the smallest | |c - p| - beta r | / ext over the nodes a point tested."""
    P = np.asarray(points, np.float64)
    acc, margin = np.zeros(len(P)), np.full(len(P), np.inf)
    pi, mi = np.arange(len(P)), np.zeros(len(P), np.int64)
    ext = tree.ext if tree.ext > 0 else 1.0
    for l in range(tree.L + 1):
        lv = tree.levels[l]
        keep = lv["r"][mi] >= 0
        pi, mi = pi[keep], mi[keep]
        dvec = lv["c"][mi] - P[pi]
        d = np.linalg.norm(dvec, axis=1)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            br = beta * lv["r"][mi]
            far = d > br  # NaN (inf * 0): near
            if np.isfinite(beta):
                np.minimum.at(margin, pi, np.abs(d - br) / ext)
            t = (lv["N"][mi] * dvec).sum(1)
            np.add.at(acc, pi[far], np.where(t[far] == 0, 0.0, t[far] / d[far] ** 3))
        pi, mi = pi[~far], mi[~far]
        if l < tree.L:
            pi, mi = np.repeat(pi, 8), (mi[:, None] * 8 + np.arange(8)).reshape(-1)
        else:
            cnt = lv["end"][mi] - lv["begin"][mi]
            rows = np.repeat(lv["begin"][mi], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
            pp = np.repeat(pi, cnt)
            tri = tree.corners[rows]
            np.add.at(acc, pp, solid_angle(P[pp], tri[:, 0], tri[:, 1], tri[:, 2]))
    return acc / FOUR_PI, margin


# ---------------------------------------------------------------------------------------------------------------
# the drop-ins (threestudio/utils/ops.py:482-584), float64
def normalize(v, target_scale):
    v = np.asarray(v, np.float64)
    v = v - v.mean(0)
    return v / np.linalg.norm(v, axis=1).max() * target_scale


def shape_loss_mesh(v, mesh_scale=0.7):
    rx = np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    ry = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    return (rx @ ry @ normalize(v, mesh_scale).T).T


def gaussian_weight(d2, sigma):
    return np.exp(-d2 / (2 * sigma ** 2))


def ce_pq(p, q, weight=None):
    """(loss, d loss / d p) with q, 1 - q clamped to [1e-4, 1 - 1e-4]."""
    lq, l1q = np.log(np.clip(q, 1e-4, 1 - 1e-4)), np.log(np.clip(1 - q, 1e-4, 1 - 1e-4))
    w = 1.0 if weight is None else weight
    return float((-(p * lq + (1 - p) * l1q) * w).sum()), -(lq - l1q) * w


def shape_loss(indicator, d2, sigmas, keep=None, delta=0.2, proximal=0.3):
    """(loss, d loss / d sigmas) of ShapeLoss.forward from the float64 indicator (w > 0.5) and squared distance; rows
    with keep == False are left out of the sum."""
    sig = np.asarray(sigmas, np.float64)
    occ_raw = 1 - np.exp(-delta * sig)
    occ = np.clip(occ_raw, 0, 1.1)
    weight = 1 - gaussian_weight(d2, proximal)
    if keep is not None:
        weight = weight * keep
    loss, dp = ce_pq(occ, indicator.astype(np.float64), weight)
    return loss, dp * ((occ_raw >= 0) & (occ_raw <= 1.1)) * delta * np.exp(-delta * sig)


# ---------------------------------------------------------------------------------------------------------------
# meshes and points of the tests
MESHES = ["sphere24", "torus32", "hand", "triangle", "two_clusters", "spanning"]
NEAR_SURFACE = 1e-3  # extents: closer points are left out of the comparisons against float64


@functools.lru_cache(maxsize=None)
def mesh(name):
    hand_built = {"two_clusters": D.two_clusters, "spanning": D.spanning}
    v, t = hand_built[name]() if name in hand_built else S.source_mesh(name)
    return np.ascontiguousarray(v, dtype=F32), np.ascontiguousarray(t, dtype=np.int32)


def query_points(v_pos, t_pos_idx, seed=0, n_uniform=1400, n_surface=(150, 50)):
    """n_uniform points uniform in 1.4x the bounding cube and points of the surface (a random face with area, uniform
    barycentrics) moved along the face normal: n_surface[0] for each of +-0.02 extents, n_surface[1] for each of
    +-0.002 extents (fewer: on the open triangle soups a point that close to one face is often closer than NEAR_SURFACE
    to another, and those points may be at most 1 % of a case)."""
    rng = np.random.default_rng(seed)
    v, tri = np.asarray(v_pos, np.float64), np.asarray(t_pos_idx)
    lo, ext, _ = box(v_pos, 0)
    centre = lo.astype(np.float64) + 0.5 * float(ext)
    pts = [centre + rng.uniform(-0.7, 0.7, (n_uniform, 3)) * float(ext)]
    c = v[tri]
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    nn = np.linalg.norm(n, axis=1)
    good = np.flatnonzero(nn > 1e-12 * float(ext) ** 2)
    for off, count in ((0.02, n_surface[0]), (-0.02, n_surface[0]), (0.002, n_surface[1]), (-0.002, n_surface[1])):
        f = good[rng.integers(0, len(good), count)]
        b = rng.dirichlet([1, 1, 1], count)
        pts.append((b[:, :, None] * c[f]).sum(1) + off * float(ext) * n[f] / nn[f, None])
    return np.concatenate(pts).astype(F32)


def surface_d2(points, v_pos, t_pos_idx):
    """float64 squared distance of every point to the mesh (distance_reference.closest_point), evaluated only on the
    pairs that can hold the minimum: a face's centroid is a point of the surface (an upper bound of the distance) and
    no point of a face is closer than the distance to its centroid minus the face's radius about it."""
    import torch
    P = np.asarray(points, np.float64)
    c = np.asarray(v_pos, np.float64)[np.asarray(t_pos_idx)]
    cen = c.mean(1)
    rad = np.linalg.norm(c - cen[:, None], axis=2).max(1)
    to_cen = np.linalg.norm(P[:, None, :] - cen[None], axis=2)
    pi, fi = np.nonzero(to_cen - rad[None] <= to_cen.min(1)[:, None])
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    d2 = D.closest_point(T(P[pi]), T(c[fi, 0]), T(c[fi, 1]), T(c[fi, 2]))[0].numpy()
    out = np.full(len(P), np.inf)
    np.minimum.at(out, pi, d2)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(points float32, exact w float64, away (N,) bool: at least NEAR_SURFACE extents from the surface, d2 float64)."""
    v, t = mesh(name)
    pts = query_points(v, t)
    d2 = surface_d2(pts, v, t)
    away = np.sqrt(d2) >= NEAR_SURFACE * float(box(v, 0)[1])
    return pts, exact(pts, v, t), away, d2


@functools.lru_cache(maxsize=None)
def tree(name, L):
    v, t = mesh(name)
    return Tree(v, t, default_levels(len(t)) if L is None else L)


@functools.lru_cache(maxsize=None)
def fast_case(name, L, beta):
    """(w_fast float64, margin, method error = max |fast - exact| over the points away from the surface)."""
    pts, w, away, _ = case(name)
    wf, margin = fast(tree(name, L), pts, beta)
    return wf, margin, float(np.abs(wf - w)[away].max())
