"""Restatements of the ray-casting contract (include/tt_abi.h, "ray casting") for tests/test_ray_host.py and
tests/test_gpu_ray.py, numpy on the CPU:
  * moller_trumbore: a float64 brute force written independently of the kernel's pair (Moeller-Trumbore, not the
    sheared edge functions), the matrix of plane parameters and smallest barycentrics of every (ray, face) pair;
  * classify: the nearest hit of that reference and which rays are "unclean" (its answer hangs on a margin below eta);
  * pair_f32: the kernel's ray_pair operation by operation in numpy float32 (the double retry included);
  * walk_f32: the kernel's slice walk over the distance grid, reading the pairs of pair_f32; brute_f32: its answer
    without a grid;
  * ao_rays_f32 / ao_reference: the rays of the ambient-occlusion kernel in fp32, and their float64 hit count;
  * the hand-built meshes and the ray sets of the tests."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as D  # noqa: E402  (box, cell: the grid the triangles are binned with)
import simplify_reference as S  # noqa: E402

F32 = np.float32
ETA = 1e-4
T_BAR = 1e-6  # the bar on t, in units of s = (L + |o|_inf) / |d|
INF32 = F32(np.inf)


# ---------------------------------------------------------------------------------------------------------------
# meshes
def tetra():
    v = np.array([[0.9, 0.1, -0.2], [-0.5, 0.8, -0.3], [-0.4, -0.7, -0.5], [0.05, 0.1, 0.85]], F32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)


def quad(size=1.0, z=0.0):
    """Two faces sharing the edge from vertex 0 to vertex 2, in the plane z."""
    s = size
    v = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], F32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def cube(half=0.5):
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(tri, np.int32)


def lattice(n=3):
    """Every axis-aligned face of an n x n x n block of cells, coordinates k / n - 0.5: faces ON cell boundaries of the
    grids that divide n."""
    m = n + 1
    idx = lambda i, j, k: (i * m + j) * m + k  # noqa: E731
    v = np.array([[F32(i) / F32(n) - F32(0.5), F32(j) / F32(n) - F32(0.5), F32(k) / F32(n) - F32(0.5)]
                  for i in range(m) for j in range(m) for k in range(m)], F32)
    tri = []
    for axis in range(3):
        for p in range(m):
            for a in range(n):
                for b in range(n):
                    def at(da, db):
                        c = [0, 0, 0]
                        c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = p, a + da, b + db
                        return idx(*c)
                    q = (at(0, 0), at(1, 0), at(1, 1), at(0, 1))
                    tri += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return v, np.array(tri, np.int32)


def degenerate():
    """Faces without area only: equal vertices (all three, two of three) and collinear ones, axis-aligned and oblique."""
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.25, 0.5, -0.25], [-0.5, -0.25, 0.75], [-0.125, 0.125, 0.25],
                  [0.5, 0.5, 0.5]], F32)  # 3, 4, 5: 5 is the midpoint of 3 and 4, exact in fp32
    tri = np.array([[0, 0, 0], [6, 6, 6], [0, 1, 1], [3, 4, 4], [0, 1, 2], [2, 0, 1], [3, 5, 4], [5, 3, 4]], np.int32)
    return v, tri


def point_mesh():
    """A mesh without extent: every vertex the same point."""
    v = np.full((3, 3), 0.25, F32)
    return v, np.array([[0, 1, 2], [2, 1, 0]], np.int32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "sphere24":
        v, tri = S.source_mesh("sphere24")
        return np.ascontiguousarray(v, F32), np.ascontiguousarray(tri, np.int32)
    return {"tetra": tetra, "quad": quad, "cube": cube, "lattice": lattice, "degenerate": degenerate,
            "point": point_mesh}[name]()


def edges(tri):
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0)


# ---------------------------------------------------------------------------------------------------------------
# ray sets
def random_rays(n, seed):
    """Origins uniform in [-1, 1]^3, Gaussian directions (any length)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, 3)).astype(F32), rng.normal(size=(n, 3)).astype(F32)


def aimed_rays(v, tri, origins, max_targets=None, seed=0):
    """From every origin, one ray at every vertex and one at every edge midpoint, target and direction in fp32."""
    v = np.asarray(v, F32)
    e = edges(np.asarray(tri))
    targets = np.concatenate([v, (v[e[:, 0]] + v[e[:, 1]]) * F32(0.5)]).astype(F32)
    if max_targets is not None and len(targets) > max_targets:
        targets = targets[np.random.default_rng(seed).choice(len(targets), max_targets, replace=False)]
    o = np.repeat(np.asarray(origins, F32), len(targets), 0)
    d = (np.tile(targets, (len(origins), 1)) - o).astype(F32)
    keep = np.abs(d).max(1) > 0
    return o[keep], d[keep]


SIXTH_ORIGINS = np.array([[-1, -1, -1], [1, 0.5, -5 / 6], [-1 / 6, 1 / 6, 1 / 3], [0, 0, 0], [2 / 3, -1, 1 / 6]], F32)


def axis_rays(n=3):
    """Axis-parallel rays lying in the face planes of lattice(n): through face interiors, along edges, both senses."""
    o, d = [], []
    planes = [F32(k) / F32(n) - F32(0.5) for k in range(n + 1)]
    for axis in range(3):
        for s in (1.0, -1.0):
            for p in planes:
                for q in (planes[1], F32(0.1), F32(-0.45)):
                    x = np.zeros(3, F32)
                    x[axis], x[(axis + 1) % 3], x[(axis + 2) % 3] = -s, p, q
                    e = np.zeros(3, F32)
                    e[axis] = s * 0.75
                    o.append(x)
                    d.append(e)
    return np.array(o, F32), np.array(d, F32)


@functools.lru_cache(maxsize=None)
def special_rays(name):
    """The aimed and axis-parallel sets of a mesh, about 700 rays."""
    v, tri = mesh(name)
    o1, d1 = aimed_rays(v, tri, SIXTH_ORIGINS, max_targets=120)
    o2, d2 = axis_rays()
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


# ---------------------------------------------------------------------------------------------------------------
# float64 reference
def moller_trumbore(o, d, v, tri, max_pairs=4_000_000):
    """(t (N,T), bmin (N,T)) in float64: the parameter at which ray i meets the plane of face f and the smallest of the
    three barycentrics there; NaN for a ray parallel to the plane or a face without area."""
    o, d, v = (np.asarray(x, np.float64) for x in (o, d, v))
    a, b, c = (v[np.asarray(tri)[:, k]] for k in range(3))
    e1, e2 = b - a, c - a
    N, T = len(o), len(a)
    t, bmin = np.empty((N, T)), np.empty((N, T))
    step = max(1, max_pairs // max(T, 1))
    cross = lambda x, y: (x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0])  # noqa: E731
    dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]  # noqa: E731
    E1, E2 = [e1[None, :, k] for k in range(3)], [e2[None, :, k] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i0 in range(0, N, step):
            dd = [d[i0:i0 + step, k, None] for k in range(3)]
            s = [o[i0:i0 + step, k, None] - a[None, :, k] for k in range(3)]
            p = cross(dd, E2)
            det = dot(E1, p)
            det = np.where(det == 0, np.nan, det)
            u = dot(s, p) / det
            q = cross(s, E1)
            w = dot(dd, q) / det
            t[i0:i0 + step] = dot(E2, q) / det
            bmin[i0:i0 + step] = np.minimum(np.minimum(u, w), 1 - u - w)
    return t, bmin


def scale(o, d, v):
    """s = (L + |o|_inf) / |d| per ray, L the mesh's largest absolute coordinate."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    return (np.abs(np.asarray(v, np.float64)).max() + np.abs(o).max(1)) / np.linalg.norm(d, axis=1)


def classify(o, d, v, tri, t_max=np.inf, eta=ETA):
    """The float64 answer and its margins: dict(t, face: nearest hit with 0 <= t <= t_max and barycentrics >= 0 (inf, -1
    for none); unclean (N,) bool; s; T, B: the matrices of moller_trumbore).  A ray is unclean when
      (a) some face's plane is met at -eta s <= t <= min(t_nearest, t_max) + eta s with the smallest barycentric within
          eta of 0 (an edge or a vertex decides), or
      (b) the two nearest hits are closer than eta s, or a hit whose barycentrics are >= -eta lies within eta s of 0 or of
          t_max (the nearest one included)."""
    T, B = moller_trumbore(o, d, v, tri)
    s = scale(o, d, v)
    with np.errstate(invalid="ignore"):
        valid = (B >= 0) & (T >= 0) & (T <= t_max)
        tv = np.where(valid, T, np.inf)
        face = np.where(valid.any(1), tv.argmin(1), -1)
        tn = tv.min(1)
        es = eta * s
        upper = np.minimum(tn, t_max) + es
        a = ((np.abs(B) <= eta) & (T >= -es[:, None]) & (T <= upper[:, None])).any(1)
        two = np.sort(tv, 1)[:, :2] if tv.shape[1] > 1 else np.concatenate([tv, np.full_like(tv, np.inf)], 1)
        near = np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] < es)
        inner = B >= -eta
        ends = (inner & (np.abs(T) <= es[:, None])).any(1)
        if np.isfinite(t_max):
            ends |= (inner & (np.abs(T - t_max) <= es[:, None])).any(1)
    return {"t": tn, "face": face, "unclean": a | near | ends, "s": s, "T": T, "B": B}


def any_reference(o, d, v, tri, t_max=np.inf, eta=ETA):
    """(hit (N,) bool, unclean (N,) bool) of the any-hit question in float64: unclean when an edge or a vertex (smallest
    barycentric within eta of 0) or an end of [0, t_max] (within eta s) decides whether some face counts."""
    T, B = moller_trumbore(o, d, v, tri)
    es = (eta * scale(o, d, v))[:, None]
    with np.errstate(invalid="ignore"):
        hit = ((B >= 0) & (T >= 0) & (T <= t_max)).any(1)
        un = ((np.abs(B) <= eta) & (T >= -es) & (T <= t_max + es)).any(1)
        inner = B >= -eta
        un |= (inner & (np.abs(T) <= es)).any(1)
        if np.isfinite(t_max):
            un |= (inner & (np.abs(T - t_max) <= es)).any(1)
    return hit, un


# ---------------------------------------------------------------------------------------------------------------
# the kernel's pair in numpy float32, every operation rounded on its own
def major_axis(d):
    """argmax |d| per row, the lowest index at equal magnitude."""
    return np.argmax(np.abs(d), axis=1)


def pair_f32(o, d, v, tri, t_max=np.inf):
    """ray_pair for every (ray, face): (hit (N,T) bool, t (N,T) float32 (inf where no hit), bary (N,T,3) float32)."""
    o, d, v = np.asarray(o, F32), np.asarray(d, F32), np.asarray(v, F32)
    tri = np.asarray(tri)
    N = len(o)
    rows = np.arange(N)
    kz = major_axis(d)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = d[rows, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        dz = d[rows, kz]
        Sx, Sy, Sz = (d[rows, kx] / dz)[:, None], (d[rows, ky] / dz)[:, None], (F32(1) / dz)[:, None]
        P = []
        for k in range(3):
            A = v[tri[:, k]][None] - o[:, None]  # (N,T,3) float32
            Az = A[rows, :, kz]
            P.append((A[rows, :, kx] - Sx * Az, A[rows, :, ky] - Sy * Az, Az))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = P
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        z = (U == 0) | (V == 0) | (W == 0)
        if z.any():
            f = lambda p, q, r, s: (p[z].astype(np.float64) * q[z] - r[z].astype(np.float64) * s[z]).astype(F32)  # noqa: E731
            U[z], V[z], W[z] = f(Cx, By, Cy, Bx), f(Ax, Cy, Ay, Cx), f(Bx, Ay, By, Ax)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        num = (U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)
        t = num / det
        hit = ~mixed & (det != 0) & np.isfinite(det) & (t >= 0) & (t <= F32(t_max))
        e1 = (v[tri[:, 1]] - v[tri[:, 0]]).astype(np.float64)  # the fp32 edge vectors; their products exact in double
        e2 = (v[tri[:, 2]] - v[tri[:, 0]]).astype(np.float64)
        flat = ((e1[:, 1] * e2[:, 2] == e1[:, 2] * e2[:, 1]) & (e1[:, 2] * e2[:, 0] == e1[:, 0] * e2[:, 2]) &
                (e1[:, 0] * e2[:, 1] == e1[:, 1] * e2[:, 0]))
        hit &= ~flat[None]
        bary = np.stack([U / det, V / det, W / det], -1)
    return hit, np.where(hit, t, INF32).astype(F32), np.where(hit[..., None], bary, F32(0)).astype(F32)


def brute_f32(hit, t):
    """The contract's answer from pair_f32's matrices: (t (N,) float32, face (N,)), the lexicographic minimum of
    (t, face) over all faces; (inf, -1) for a miss."""
    face = np.where(hit.any(1), t.argmin(1), -1)  # argmin: the first, hence smallest, face at equal t
    return t.min(1), face


# ---------------------------------------------------------------------------------------------------------------
# the kernel's walk
REL = F32(2.0 ** -16)


class Grid:
    """The distance grid of a mesh as the kernel bins it (distance_reference.box / cell): cells[(c0, c1, c2)] = faces."""

    def __init__(self, v, tri, G):
        self.v, self.tri, self.G = np.asarray(v, F32), np.asarray(tri), G
        self.lo, self.ext, self.h, self.inv_h = D.box(self.v, G)
        p3 = self.v[self.tri]
        c0, c1 = D.cell(p3.min(1), self.lo, self.inv_h, G), D.cell(p3.max(1), self.lo, self.inv_h, G)
        self.cells = {}
        for f in range(len(self.tri)):
            for x in range(c0[f, 0], c1[f, 0] + 1):
                for y in range(c0[f, 1], c1[f, 1] + 1):
                    for z in range(c0[f, 2], c1[f, 2] + 1):
                        self.cells.setdefault((x, y, z), []).append(f)

    def cell(self, x, axis):
        with np.errstate(all="ignore"):
            c = np.floor((F32(x) - self.lo[axis]) * self.inv_h)
        c = np.fmin(np.fmax(c, F32(0)), F32(self.G - 1))  # fmax / fmin drop a NaN, as fmaxf / fminf do
        return int(c)


def _below(x, pad):
    return x - (np.abs(x) * REL + pad)


def _above(x, pad):
    return x + (np.abs(x) * REL + pad)


def walk_f32(o, d, grid, hit, t, t_max=np.inf, any_hit=False, count=None):
    """The slice walk of one thread per ray, in float32, reading the pairs from pair_f32's (hit, t): (t (N,), face (N,)),
    or the any-hit flags (N,) bool.  count (a list), if given, receives the number of cells each ray visited."""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    G, lo, ext, h = grid.G, grid.lo, grid.ext, grid.h
    out_t, out_f = np.full(len(o), INF32), np.full(len(o), -1, np.int64)
    out_any = np.zeros(len(o), bool)
    cen = lo + F32(0.5) * ext
    with np.errstate(all="ignore"):
        for i in range(len(o)):
            oi, di = o[i], d[i]
            tol = REL * (ext + np.abs(oi - cen).max() + np.abs(cen).max())
            t_lo, t_hi, outside = F32(0), F32(t_max), False
            for a in range(3):
                p0, p1 = lo[a] - tol, (lo[a] + ext) + tol
                if di[a] == 0:
                    outside |= bool(oi[a] < p0 or oi[a] > p1)
                else:
                    t0, t1 = (p0 - oi[a]) / di[a], (p1 - oi[a]) / di[a]
                    t_lo = np.fmax(t_lo, _below(np.fmin(t0, t1), F32(0)))
                    t_hi = np.fmin(t_hi, _above(np.fmax(t0, t1), F32(0)))
            visited = 0
            if outside or not t_lo <= t_hi:
                if count is not None:
                    count.append(0)
                continue
            ka = int(np.argmax(np.abs(di)))
            ku, kv = (1 if ka == 0 else 0), (1 if ka == 2 else 2)
            tol_t = tol / np.abs(di[ka])
            up = di[ka] > 0
            best, bf = INF32, np.iinfo(np.int64).max
            for j in range(G):
                k = j if up else G - 1 - j
                q0, q1 = lo[ka] + F32(k) * h, lo[ka] + F32(k + 1) * h
                tq0, tq1 = (q0 - oi[ka]) / di[ka], (q1 - oi[ka]) / di[ka]
                s, e = _below(tq0 if up else tq1, tol_t), _above(tq1 if up else tq0, tol_t)
                if j == 0:
                    s = -INF32
                if j == G - 1:
                    e = INF32
                if s > t_hi:
                    break
                t0, t1 = np.fmax(s, t_lo), np.fmin(e, t_hi)
                if t0 <= t1:
                    rng = []
                    for b in (ku, kv):
                        x0 = oi[b] if di[b] == 0 else oi[b] + t0 * di[b]
                        x1 = oi[b] if di[b] == 0 else oi[b] + t1 * di[b]
                        c0 = grid.cell(np.fmin(x0, x1) - tol, b)
                        rng.append((c0, max(c0, grid.cell(np.fmax(x0, x1) + tol, b))))
                    for iu in range(rng[0][0], rng[0][1] + 1):
                        for iv in range(rng[1][0], rng[1][1] + 1):
                            c = [0, 0, 0]
                            c[ka], c[ku], c[kv] = k, iu, iv
                            visited += 1
                            for f in grid.cells.get(tuple(c), ()):
                                if not hit[i, f]:
                                    continue
                                out_any[i] = True
                                if t[i, f] < best or (t[i, f] == best and f < bf):
                                    best, bf = t[i, f], f
                            if any_hit and out_any[i]:
                                break
                        if any_hit and out_any[i]:
                            break
                if (any_hit and out_any[i]) or best < s:
                    break
            if bf != np.iinfo(np.int64).max:
                out_t[i], out_f[i] = best, bf
            if count is not None:
                count.append(visited)
    return out_any if any_hit else (out_t, out_f)


# ---------------------------------------------------------------------------------------------------------------
# ambient occlusion
def ao_directions(K):
    """ops.ao_directions restated: float64, rounded once."""
    k = np.arange(K, dtype=np.float64)
    u1 = (k + 0.5) / K
    u2 = np.zeros(K)
    f, n = 0.5, np.arange(K)
    while n.any():
        u2 += f * (n & 1)
        n >>= 1
        f *= 0.5
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - u1)], 1).astype(F32)


def ao_rays_f32(points, normals, dirs_local, bias):
    """The rays of tt_ray_ao in numpy float32, operation by operation: (origins (N,K,3), dirs (N,K,3))."""
    p, n, dl = np.asarray(points, F32), np.asarray(normals, F32), np.asarray(dirs_local, F32)
    bias = F32(bias)
    n = n / np.abs(n).max(1, keepdims=True)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    n = n / ln[:, None]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sg = np.copysign(F32(1), nz)
    a = F32(-1) / (sg + nz)
    b = (nx * ny) * a
    Tv = np.stack([F32(1) + ((sg * nx) * nx) * a, sg * b, (-sg) * nx], 1)
    Bv = np.stack([b, sg + (ny * ny) * a, -ny], 1)
    x, y, z = dl[None, :, 0, None], dl[None, :, 1, None], dl[None, :, 2, None]
    dirs = (x * Tv[:, None] + y * Bv[:, None]) + z * n[:, None]
    orig = p + bias * n
    return np.broadcast_to(orig[:, None], dirs.shape).astype(F32), dirs.astype(F32)


def ao_reference(points, normals, dirs_local, bias, max_distance, v, tri):
    """(hits (N,) int, unclean (N,) int: how many of a point's rays the reference calls unclean) of the float64 any-hit
    answer on the rays of ao_rays_f32 (their fp32 rounding is far inside the unclean margins)."""
    o, d = ao_rays_f32(points, normals, dirs_local, bias)
    N, K = o.shape[:2]
    hit, un = any_reference(o.reshape(-1, 3), d.reshape(-1, 3), v, tri, t_max=max_distance)
    return hit.reshape(N, K).sum(1), un.reshape(N, K).sum(1)


def surface_points(v, tri, n, seed):
    """n points on the surface with their face normals (unnormalised cross products): random faces of non-zero area,
    barycentrics away from the edges."""
    v, tri = np.asarray(v, np.float64), np.asarray(tri)
    rng = np.random.default_rng(seed)
    f = rng.integers(0, len(tri), n)
    b = rng.dirichlet((2.0, 2.0, 2.0), n)
    a, bb, c = (v[tri[f, k]] for k in range(3))
    return ((b[:, 0:1] * a + b[:, 1:2] * bb + b[:, 2:3] * c).astype(F32),
            np.cross(bb - a, c - a).astype(F32))


# ---------------------------------------------------------------------------------------------------------------
# the committed ray sets of the tests, with their float64 classification, computed once
CASE_SEEDS = {"tetra": 11, "cube": 12, "lattice": 13, "sphere24": 14}


@functools.lru_cache(maxsize=None)
def case(name, n=2000):
    """(origins, dirs, classify(...)) of the seeded random set of a mesh."""
    v, tri = mesh(name)
    o, d = random_rays(n, CASE_SEEDS[name])
    return o, d, classify(o, d, v, tri)


def point_residual(o, d, v, tri, t, face, bary):
    """|sum_k b_k v_k - (o + t d)|_inf / (L + |o|_inf) of an answer, evaluated in float64; rows with face < 0 give 0."""
    o, d, v = (np.asarray(x, np.float64) for x in (o, d, v))
    f = np.maximum(np.asarray(face), 0)
    p = (np.asarray(bary, np.float64)[:, :, None] * v[np.asarray(tri)[f]]).sum(1)
    with np.errstate(invalid="ignore"):
        r = np.abs(p - (o + np.asarray(t, np.float64)[:, None] * d)).max(1) / (np.abs(v).max() + np.abs(o).max(1))
    return np.where(np.asarray(face) >= 0, r, 0.0)


@functools.lru_cache(maxsize=None)
def restated(name, n=2000):
    """(t, face, bary) of the fp32 restatement (pair_f32 + brute_f32) on case(name)."""
    v, tri = mesh(name)
    o, d, _ = case(name, n)
    hit, t, bary = pair_f32(o, d, v, tri)
    bt, bf = brute_f32(hit, t)
    return bt, bf, bary[np.arange(len(o)), np.maximum(bf, 0)] * (bf >= 0)[:, None]
