"""numpy restatement of the UV-atlas and texture-fill contract (include/tt_abi.h, "UV atlas and texture fill") for small
meshes: face pairs, labels + smoothing, charts, chart boxes, shelf packing, UVs, texel-centre coverage and the nearest
fill.  float64 where the contract computes in double, numpy float32 where it computes in fp32 (the UVs), plain Python
for the packing (double, every probe rounded to float, as tt_uv_pack)."""
import math

import numpy as np

AXES = [(1, 2), (2, 1), (2, 0), (0, 2), (0, 1), (1, 0)]  # (u, v) coordinates of labels +x -x +y -y +z -z
REL_PREC = 1e-4  # TT_UV_PACK_REL_PREC


def face_pairs(tri):
    """the two faces of every edge that exactly two face edges use (ops.MeshTopology.face_pairs, same order)"""
    tri = np.asarray(tri, np.int64)
    V = int(tri.max()) + 1 if len(tri) else 1
    a, b = tri, tri[:, [1, 2, 0]]
    key = (np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1)
    perm = np.argsort(key, kind="stable")
    skey = key[perm]
    _, starts, counts = np.unique(skey, return_index=True, return_counts=True)
    two = starts[counts == 2]
    return np.stack([perm[two] // 3, perm[two + 1] // 3], axis=1).astype(np.int64)


def labels(v, tri, pairs, rounds=8, tau=0.3):
    v = np.asarray(v, np.float32).astype(np.float64)
    tri = np.asarray(tri, np.int64)
    T = len(tri)
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    s = np.stack([n[:, 0], -n[:, 0], n[:, 1], -n[:, 1], n[:, 2], -n[:, 2]], axis=1)
    lab = np.argmax(s, axis=1)
    t = float(np.float32(tau))
    adm = np.copysign(s * s, s) >= (t * t) * nn[:, None]
    live = nn > 0
    adm[~live] = False
    lab[~live] = 0
    nbr = [[] for _ in range(T)]
    for a, b in pairs:
        if a != b:
            nbr[a].append(b)
            nbr[b].append(a)
    nb = np.full((T, 3), -1, np.int64)
    for f in range(T):
        nb[f, :len(nbr[f][:3])] = nbr[f][:3]
    has = nb >= 0
    for _ in range(rounds):
        nl = np.where(has, lab[np.maximum(nb, 0)], 6)
        cnt = np.stack([(lab == l).astype(np.int64) + (nl == l).sum(1) for l in range(6)], axis=1)
        best, bc = lab.copy(), cnt[np.arange(T), lab]
        for l in range(6):
            c = np.where(adm[:, l], cnt[:, l], -1)
            best = np.where(c > bc, l, best)
            bc = np.maximum(c, bc)
        nmin = nl.min(1)
        lab = np.where(adm.any(1), best, np.where(nmin < 6, nmin, 0))
    return lab


def charts(tri, pairs, lab, singleton=None):
    """dense chart ids in order of each chart's smallest face"""
    T = len(tri)
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    single = np.zeros(T, bool) if singleton is None else np.asarray(singleton, bool)
    for a, b in pairs:
        if lab[a] == lab[b] and not single[a] and not single[b]:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    comp = np.array([find(f) for f in range(T)])
    roots = np.unique(comp)
    return np.searchsorted(roots, comp)


def chart_boxes(v, tri, lab, chart):
    v = np.asarray(v, np.float32)
    C = int(chart.max()) + 1
    box = np.zeros((C, 4), np.float32)
    box[:, :2], box[:, 2:] = np.inf, -np.inf
    for f in range(len(tri)):
        cu, cv = AXES[lab[f]]
        for k in range(3):
            p = v[tri[f, k]]
            c = chart[f]
            box[c, 0], box[c, 1] = min(box[c, 0], p[cu]), min(box[c, 1], p[cv])
            box[c, 2], box[c, 3] = max(box[c, 2], p[cu]), max(box[c, 3], p[cv])
    return box


def _shelf(w, h, s, N, pad):
    bw = [math.ceil(x * s) + 2 * pad + 1 for x in w]
    bh = [math.ceil(x * s) + 2 * pad + 1 for x in h]
    order = sorted(range(len(w)), key=lambda c: (-bh[c], -bw[c], c))
    x = y = shelf = 0
    off = np.zeros((len(w), 2), np.int64)
    for c in order:
        if bw[c] > N or bh[c] > N:
            return None
        if x + bw[c] > N:
            y, x, shelf = y + shelf, 0, 0
        if shelf == 0:
            shelf = bh[c]
        if y + shelf > N:
            return None
        off[c] = (x, y)
        x += bw[c]
    return off


def f32(x):
    return float(np.float32(x))


def pack(box, N, pad):
    """(offsets (C,2), s) exactly as tt_uv_pack"""
    box = np.asarray(box, np.float32).astype(np.float64)
    w, h = list(box[:, 2] - box[:, 0]), list(box[:, 3] - box[:, 1])
    m = max(max(w), max(h))
    if m == 0.0:
        return _shelf(w, h, 1.0, N, pad), 1.0
    lo, hi = 0.0, f32((N - 2.0 * pad) / m)
    for _ in range(200):
        if not hi - lo > REL_PREC * hi:
            break
        mid = f32(0.5 * (lo + hi))
        if not (lo < mid < hi):
            break
        if _shelf(w, h, mid, N, pad) is not None:
            lo = mid
        else:
            hi = mid
    return _shelf(w, h, lo, N, pad), lo


def emit(v, tri, lab, chart, box, off, s, N, pad):
    """(v_tex (Vt,2) float32, t_tex_idx (T,3)) with UV vertices numbered by the first corner of each (chart, vertex)"""
    v = np.asarray(v, np.float32)
    ids, v_tex, t_tex = {}, [], np.zeros(tri.shape, np.int64)
    sf, half, Nf = np.float32(s), np.float32(0.5), np.float32(N)
    for q in range(tri.size):
        f, k = divmod(q, 3)
        key = (int(chart[f]), int(tri[f, k]))
        if key not in ids:
            ids[key] = len(v_tex)
            c = chart[f]
            cu, cv = AXES[lab[f]]
            p = v[tri[f, k]]
            U = (np.float32(off[c, 0] + pad) + half) + (p[cu] - box[c, 0]) * sf
            W = (np.float32(off[c, 1] + pad) + half) + (p[cv] - box[c, 1]) * sf
            v_tex.append((U / Nf, W / Nf))
        t_tex[f, k] = ids[key]
    return np.array(v_tex, np.float32), t_tex


def coverage(v_tex, t_tex, N):
    """(count (N,N) of UV triangles whose interior holds each texel centre, ambiguous (N,N) bool: a centre within 1e-7
    texels of an edge line, where float rounding may decide differently) in float64 with the top-left tie rule"""
    uv = np.asarray(v_tex, np.float64) * N
    cnt = np.zeros((N, N), np.int64)
    amb = np.zeros((N, N), bool)
    for t in t_tex:
        P = uv[t]
        area = (P[1, 0] - P[0, 0]) * (P[2, 1] - P[0, 1]) - (P[1, 1] - P[0, 1]) * (P[2, 0] - P[0, 0])
        if area == 0 or len(set(t.tolist())) < 3:
            continue
        sg = 1.0 if area > 0 else -1.0
        x0, x1 = int(max(math.floor(P[:, 0].min()) - 1, 0)), int(min(math.ceil(P[:, 0].max()) + 1, N - 1))
        y0, y1 = int(max(math.floor(P[:, 1].min()) - 1, 0)), int(min(math.ceil(P[:, 1].max()) + 1, N - 1))
        if x1 < x0 or y1 < y0:
            continue
        X, Y = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        inside = np.ones(X.shape, bool)
        for k in range(3):
            a, b = P[(k + 1) % 3], P[(k + 2) % 3]
            e = sg * ((a[0] - X) * (b[1] - Y) - (a[1] - Y) * (b[0] - X))
            L = math.hypot(b[0] - a[0], b[1] - a[1])
            amb[y0:y1 + 1, x0:x1 + 1] |= np.abs(e) <= 1e-7 * max(L, 1e-30)
            gx, gy = sg * (a[1] - b[1]), sg * (b[0] - a[0])
            owns = gx > 0 or (gx == 0 and gy > 0)
            inside &= (e > 0) | ((e == 0) & owns)
        cnt[y0:y1 + 1, x0:x1 + 1] += inside
    return cnt, amb


def nearest_sq_dist(mask):
    """(H,W) squared distance of every texel to the nearest True texel (brute force; inf without one)"""
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return np.full((H, W), np.inf)
    gy, gx = np.mgrid[0:H, 0:W]
    best = np.full((H, W), np.inf)
    for i in range(0, len(ys), 256):
        d = (gy[..., None] - ys[None, None, i:i + 256]) ** 2 + (gx[..., None] - xs[None, None, i:i + 256]) ** 2
        best = np.minimum(best, d.min(-1))
    return best
