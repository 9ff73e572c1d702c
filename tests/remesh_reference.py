"""Test-only numpy restatement of the isotropic remeshing contract (include/tt_abi.h, "isotropic remeshing") and a
checker of the traces ops.mesh_remesh returns.  Written from the contract text, on tests/decimate_reference.py (the
topology of a round, the link condition, the flip test of a collapse, the hashed independent set) and
tests/distance_reference.py (the float64 closest point).

  restatement   thresholds, len2 (fp32 squared lengths), split_pass (vectorised), collapse_ok / collapse_round,
                flip_ok / flip_round (sequential), relax / project / fold_guard, remesh (the whole loop, with its trace)
  checker       check_trace(v, tri, L, trace, final): replays a trace record by record and asserts what the contract
                says of every traced operation
  metrics       quality(v, tri, L): the figures the issue's table reports

Lengths are compared as the contract compares them: fp32 squared lengths, every product and sum rounded to fp32,
(dx dx + dy dy) + dz dz.  The checker allows a relative slack of 1e-6 at every threshold (decimation's), the
restatement none."""
import numpy as np

import decimate_reference as D

MAX_ROUNDS = 1024
MAX_SPLIT_PASSES = 32
SLACK = 1e-6


# ---------------------------------------------------------------------------------------------------------------
# inputs
def bumpy_sphere_level(R):
    """r - 0.3 - 0.04 sin(9x) cos(7y) sin(8z + 1) on the R^3 lattice of [0,1]^3, r the distance to (0.5, 0.5, 0.5)."""
    g = np.linspace(0.0, 1.0, R)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    r = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    return (r - 0.3 - 0.04 * np.sin(9 * x) * np.cos(7 * y) * np.sin(8 * z + 1)).astype(np.float32)


def mean_edge(v, tri):
    e = np.unique(np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64), 1), axis=0)
    p = np.asarray(v, np.float64)
    return float(np.linalg.norm(p[e[:, 0]] - p[e[:, 1]], axis=1).mean())


# ---------------------------------------------------------------------------------------------------------------
# thresholds and lengths
def thresholds(L):
    """(hi2, lo2) fp32: the squares of fl32(4/3 L) and fl32(4/5 L), the products taken in double and rounded once."""
    h, l = np.float32((4.0 / 3.0) * float(L)), np.float32(0.8 * float(L))
    return np.float32(h * h), np.float32(l * l)


def len2(p, q):
    d = np.asarray(q, np.float32) - np.asarray(p, np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def midpoint(p, q):
    return np.float32(0.5) * (np.asarray(p, np.float32) + np.asarray(q, np.float32))


def edge_table(tri, V):
    """(edges (E,2) a <= b lexicographic, counts (E), fe2e (3T): the unique edge of face edge 3f + k, order (3T): the
    face edges grouped by unique edge, ascending inside a group, starts (E))"""
    tri = np.asarray(tri, np.int64)
    a, b = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)
    key = np.minimum(a, b) * V + np.maximum(a, b)
    uniq, fe2e, counts = np.unique(key, return_inverse=True, return_counts=True)
    order = np.argsort(key, kind="stable")
    return np.stack([uniq // V, uniq % V], 1), counts, fe2e.reshape(-1), order, np.cumsum(counts) - counts


# ---------------------------------------------------------------------------------------------------------------
# split
def split_pass(v, tri, hi2):
    """One split pass: (v', tri', marked edges (k,2) int32 in ascending unique-edge order)."""
    v, tri = np.asarray(v, np.float32), np.asarray(tri, np.int64)
    V, T = len(v), len(tri)
    edges, _, fe2e, _, _ = edge_table(tri, V)
    mark = (len2(v[edges[:, 0]], v[edges[:, 1]]) > hi2) & (edges[:, 0] != edges[:, 1])
    rank = np.cumsum(mark) - mark
    v2 = np.concatenate([v, midpoint(v[edges[mark, 0]], v[edges[mark, 1]])])
    mid = np.where(mark, V + rank, -1)[fe2e].reshape(T, 3)
    n = (mid >= 0).sum(1)
    child = np.full((T, 4, 3), -1, np.int64)
    rot = lambda arr, k, j: np.take_along_axis(arr, ((k + j) % 3)[:, None], 1)[:, 0]
    s = n == 0
    child[s, 0] = tri[s]
    s = np.flatnonzero(n == 1)
    k = np.argmax(mid[s] >= 0, 1)
    a, b, c, m = rot(tri[s], k, 0), rot(tri[s], k, 1), rot(tri[s], k, 2), rot(mid[s], k, 0)
    child[s, 0], child[s, 1] = np.stack([a, m, c], 1), np.stack([m, b, c], 1)
    s = np.flatnonzero(n == 2)
    k = np.argmin(mid[s] >= 0, 1)  # the unmarked edge (a, b); c is cut off
    a, b, c = rot(tri[s], k, 0), rot(tri[s], k, 1), rot(tri[s], k, 2)
    mb, ma = rot(mid[s], k, 1), rot(mid[s], k, 2)
    da, db = len2(v2[a], v2[mb]), len2(v2[b], v2[ma])
    from_a = (da < db) | ((da == db) & (a < b))
    child[s, 0] = np.stack([mb, c, ma], 1)
    child[s, 1] = np.where(from_a[:, None], np.stack([a, b, mb], 1), np.stack([a, b, ma], 1))
    child[s, 2] = np.where(from_a[:, None], np.stack([a, mb, ma], 1), np.stack([b, mb, ma], 1))
    s = n == 3
    i, m = tri[s], mid[s]
    child[s, 0] = np.stack([i[:, 0], m[:, 0], m[:, 2]], 1)
    child[s, 1] = np.stack([i[:, 1], m[:, 1], m[:, 0]], 1)
    child[s, 2] = np.stack([i[:, 2], m[:, 2], m[:, 1]], 1)
    child[s, 3] = m
    keep = np.arange(4)[None, :] <= n[:, None]
    return v2, child[keep], edges[mark].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# collapse
def ring_ok(topo, v, a, b, x32, hi2, slack=0.0):
    ring = np.setdiff1d(np.union1d(topo.N(a), topo.N(b)), [a, b])
    return bool((len2(v[ring], x32[None, :]) <= hi2 * np.float32(1.0 + slack)).all())


def collapse_ok(topo, v, a, b, hi2, lo2, slack=0.0):
    """The reason edge (a, b) is no collapse candidate, or None; the point is the fp32 midpoint."""
    why = D.link_ok(topo, a, b)
    if why is not None:
        return why
    if not len2(v[a], v[b]) < lo2 * np.float32(1.0 + slack):
        return "length"
    x = midpoint(v[a], v[b])
    if not ring_ok(topo, v, a, b, x, hi2, slack):
        return "ring"
    if not D.flip_ok(topo, v, a, b, x, slack=slack):
        return "flip"
    return None


def collapse_round(v, tri, hi2, lo2, rnd):
    """(kept edges (k,2) in ascending edge index, their midpoints (k,3) fp32) of one collapse round."""
    topo = D.Topology(tri, len(v))
    e = topo.edges
    pre = np.flatnonzero((len2(v[e[:, 0]], v[e[:, 1]]) < lo2) & ~topo.locked[e[:, 0]] & ~topo.locked[e[:, 1]])
    cost_bits = np.full(len(e), D.INVALID, np.int64)
    for i in pre:
        if collapse_ok(topo, v, int(e[i, 0]), int(e[i, 1]), hi2, lo2) is None:
            cost_bits[i] = 0
    kept = D.select(topo, cost_bits, rnd, 1 << 60, passes=1)
    return e[kept].astype(np.int32), midpoint(v[e[kept, 0]], v[e[kept, 1]])


def apply_collapses(v, tri, edges, xopt):
    v, remap = np.array(v, np.float32), np.arange(len(v))
    for (a, b), x in zip(np.asarray(edges, np.int64), np.asarray(xopt, np.float32)):
        v[a], remap[b] = x, a
    t = remap[np.asarray(tri, np.int64)]
    return v, t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])]


# ---------------------------------------------------------------------------------------------------------------
# flip
def flip_faces(tri, order, starts, counts, e, a, b):
    """(f0, c, f1, d): the face that runs a -> b with its opposite corner and the face that runs b -> a with its, or
    None when the edge has not exactly two faces of opposite direction."""
    if counts[e] != 2:
        return None
    out = {}
    for fe in order[starts[e]:starts[e] + 2]:
        f, k = int(fe) // 3, int(fe) % 3
        out[(int(tri[f, k]), int(tri[f, (k + 1) % 3]))] = (f, int(tri[f, (k + 2) % 3]))
    if (a, b) not in out or (b, a) not in out:
        return None
    return out[(a, b)] + out[(b, a)]


def flip_ok(topo, v, a, b, c, d, hi2, slack=0.0):
    """The reason the flip of edge (a, b) with opposite corners c, d is no candidate, or None."""
    if topo.locked[a] or topo.locked[b]:
        return "locked"
    if c == d or (min(c, d), max(c, d)) in topo.edge_index:
        return "edge exists"
    val = lambda w: len(topo.N(w))
    tgt = lambda w: 4 if topo.locked[w] else 6
    before = sum(abs(val(w) - tgt(w)) for w in (a, b, c, d))
    after = sum(abs(val(w) - 1 - tgt(w)) for w in (a, b)) + sum(abs(val(w) + 1 - tgt(w)) for w in (c, d))
    if not after < before:
        return "valence"
    if not len2(v[c], v[d]) <= hi2 * np.float32(1.0 + slack):
        return "length"
    p = np.asarray(v, np.float64)
    old = [np.cross(p[b] - p[a], p[c] - p[a]), np.cross(p[a] - p[b], p[d] - p[b])]
    new = [np.cross(p[d] - p[a], p[c] - p[a]), np.cross(p[b] - p[d], p[c] - p[d])]
    for m in new:
        for n in old:
            if not m @ n > -slack * np.sqrt((m @ m) * (n @ n)):
                return "normal"
    return None


def flip_round(v, tri, hi2, rnd):
    """(flipped edges (k,2) int32 in ascending edge index, their (c, d) (k,2) int32) of one flip round."""
    topo = D.Topology(tri, len(v))
    _, counts, _, order, starts = edge_table(tri, len(v))
    cand = {}
    for e, (a, b) in enumerate(topo.edges):
        a, b = int(a), int(b)
        if topo.locked[a] or topo.locked[b]:
            continue
        q = flip_faces(topo.tri, order, starts, counts, e, a, b)
        if q is not None and flip_ok(topo, v, a, b, q[1], q[3], hi2) is None:
            cand[e] = (a, b, q[1], q[3])
    key = {e: (D.hash32(q[0], q[1], rnd) << 32) | e for e, q in cand.items()}
    owner = {}
    for e, q in cand.items():
        for w in q:
            owner[w] = min(owner.get(w, 1 << 64), key[e])
    won = sorted(e for e, q in cand.items() if all(owner[w] == key[e] for w in q))
    return (np.asarray([cand[e][:2] for e in won], np.int32).reshape(-1, 2),
            np.asarray([cand[e][2:] for e in won], np.int32).reshape(-1, 2))


def apply_flips(tri, edges, cd):
    tri = np.array(tri, np.int64)
    V = int(tri.max()) + 1
    all_edges, counts, _, order, starts = edge_table(tri, V)
    index = {(int(a), int(b)): i for i, (a, b) in enumerate(all_edges)}
    src = tri.copy()
    for (a, b), (c, d) in zip(np.asarray(edges, np.int64), np.asarray(cd, np.int64)):
        f0, c0, f1, d0 = flip_faces(src, order, starts, counts, index[(int(a), int(b))], int(a), int(b))
        assert (c0, d0) == (int(c), int(d)), f"flip ({a},{b}): corners {(c0, d0)}, traced {(int(c), int(d))}"
        tri[f0], tri[f1] = (a, d, c), (d, b, c)
    return tri


# ---------------------------------------------------------------------------------------------------------------
# move
def relax(v, tri):
    """(q (V,3) float64: p + (g - p) - ((g - p) . n) n for the movable vertices, p for the others; movable (V) bool: the
    unlocked vertices a face references)"""
    topo = D.Topology(tri, len(v))
    p = np.asarray(v, np.float64)
    movable = np.zeros(len(v), bool)
    movable[topo.tri.reshape(-1)] = True
    movable &= ~topo.locked
    row = np.repeat(np.arange(len(v)), np.diff(topo.nbr_ptr))
    g = np.zeros_like(p)
    np.add.at(g, row, p[topo.nbr_col])
    g /= np.maximum(np.diff(topo.nbr_ptr), 1)[:, None]
    fn = np.cross(p[topo.tri[:, 1]] - p[topo.tri[:, 0]], p[topo.tri[:, 2]] - p[topo.tri[:, 0]])
    n = np.zeros_like(p)
    corner = np.argsort(topo.tri.reshape(-1), kind="stable")
    np.add.at(n, topo.tri.reshape(-1)[corner], fn[corner // 3])
    l = np.linalg.norm(n, axis=1)
    n = np.where((l > 0)[:, None], n / np.where(l > 0, l, 1.0)[:, None], 0.0)
    d = g - p
    q = p + d - (d * n).sum(1)[:, None] * n
    return np.where(movable[:, None], q, p), movable


def project(points, v0, t0, chunk=256):
    """The closest point of the mesh (v0, t0) to every point, float64 (distance_reference.closest_point, brute force)."""
    import torch

    import distance_reference as DR
    A, B, C = DR.corners(v0, t0)
    out = np.empty((len(points), 3))
    P = torch.as_tensor(np.asarray(points, np.float64))
    for s in range(0, len(P), chunk):
        d2, bary = DR.closest_point(P[s:s + chunk, None, :], A[None], B[None], C[None])
        f = d2.argmin(1)
        b = bary[torch.arange(len(f)), f]
        out[s:s + chunk] = (b[:, 0:1] * A[f] + b[:, 1:2] * B[f] + b[:, 2:3] * C[f]).numpy()
    return out


def tied_points(point, v0, t0, slack):
    """The closest points, per face, of every face whose squared distance to `point` is within a relative `slack` of
    the smallest: more than one point where the closest point is a tie (a point on a symmetry plane over a valley
    edge), which rounding then decides."""
    import torch

    import distance_reference as DR
    A, B, C = DR.corners(v0, t0)
    d2, b = DR.closest_point(torch.as_tensor(np.asarray(point, np.float64))[None, :], A, B, C)
    near = d2 <= d2.min() * (1.0 + slack)
    return (b[near, 0:1] * A[near] + b[near, 1:2] * B[near] + b[near, 2:3] * C[near]).numpy()


def folded(old, new, tri):
    """(T) bool: the faces whose old normal is non-zero and whose new normal has a non-positive dot product with it"""
    o, n = np.asarray(old, np.float64)[tri], np.asarray(new, np.float64)[tri]
    no = np.cross(o[:, 1] - o[:, 0], o[:, 2] - o[:, 0])
    nn = np.cross(n[:, 1] - n[:, 0], n[:, 2] - n[:, 0])
    return ((no * no).sum(1) > 0) & ~((no * nn).sum(1) > 0)


def fold_guard(old, new, tri):
    """(positions (V,3) fp32, reverted (V) bool): the Jacobi fixed point of the guard"""
    old, new, tri = np.asarray(old, np.float32), np.asarray(new, np.float32), np.asarray(tri, np.int64)
    rev = np.zeros(len(old), bool)
    while True:
        cur = np.where(rev[:, None], old, new)
        bad = folded(old, cur, tri)
        if not bad.any():
            return cur, rev
        rev[tri[bad].reshape(-1)] = True


def move(v, tri, v0, t0):
    q, movable = relax(v, tri)
    new = np.array(v, np.float32)
    if movable.any():
        new[movable] = project(q[movable].astype(np.float32), v0, t0).astype(np.float32)
    return fold_guard(v, new, tri)


# ---------------------------------------------------------------------------------------------------------------
# the whole loop
def emit(v, tri):
    used = np.zeros(len(v), bool)
    used[tri.reshape(-1)] = True
    return np.asarray(v, np.float32)[used], (np.cumsum(used) - 1)[tri].astype(np.int32)


def split_phase(v, tri, hi2, trace):
    n, capped = 0, False
    for p in range(MAX_SPLIT_PASSES + 1):
        if not (lambda e: (len2(v[e[:, 0]], v[e[:, 1]]) > hi2).any())(edge_table(tri, len(v))[0]):
            break
        if p == MAX_SPLIT_PASSES:
            capped = True
            break
        v, tri, edges = split_pass(v, tri, hi2)
        trace.append(("split", edges))
        n += len(edges)
    return v, tri, n, capped


def remesh(v, tri, L, iterations=5):
    """(v', t', info) as ops.mesh_remesh's, numpy, the trace always; info["rounds"] lists (phase, rounds) pairs."""
    v, tri = np.asarray(v, np.float32), np.asarray(tri, np.int64)
    v0, t0 = v.copy(), tri.copy()
    hi2, lo2 = thresholds(L)
    info = {"edge_length": float(L), "iterations": iterations, "n_split": [], "n_collapsed": [], "n_flipped": [],
            "n_reverted": [], "split_capped": False, "rounds_capped": False, "rounds": [],
            "n_locked": int(D.Topology(tri, len(v)).locked.sum()) if len(tri) else 0}
    trace = []
    for _ in range(iterations):
        v, tri, n, capped = split_phase(v, tri, hi2, trace)
        info["n_split"].append(n)
        info["split_capped"] |= capped
        n = 0
        for rnd in range(MAX_ROUNDS + 1):
            edges, x = collapse_round(v, tri, hi2, lo2, rnd)
            if not len(edges):
                break
            if rnd == MAX_ROUNDS:
                info["rounds_capped"] = True
                break
            trace.append(("collapse", edges, x))
            v, tri = apply_collapses(v, tri, edges, x)
            n += len(edges)
        info["n_collapsed"].append(n)
        info["rounds"].append(("collapse", rnd))
        n = 0
        for rnd in range(MAX_ROUNDS + 1):
            edges, cd = flip_round(v, tri, hi2, rnd)
            if not len(edges):
                break
            if rnd == MAX_ROUNDS:
                info["rounds_capped"] = True
                break
            trace.append(("flip", edges, cd))
            tri = apply_flips(tri, edges, cd)
            n += len(edges)
        info["n_flipped"].append(n)
        info["rounds"].append(("flip", rnd))
        v, rev = move(v, tri, v0, t0)
        trace.append(("move", v.copy(), rev.astype(np.uint8)))
        info["n_reverted"].append(int(rev.sum()))
    v, tri, n, capped = split_phase(v, tri, hi2, trace)
    info["n_split"].append(n)
    info["split_capped"] |= capped
    info["trace"] = trace
    v_out, t_out = emit(v, tri)
    return v_out, t_out, info


# ---------------------------------------------------------------------------------------------------------------
# checker
def check_trace(v, tri, L, trace, final=None, move_tol=1e-5):
    """Replays `trace` (ops.mesh_remesh's records, numpy) on the input mesh and asserts, per record:
      split     the marked edges are exactly the edges with len2 > hi2, in ascending edge order (fp32 arithmetic the
                restatement repeats bit for bit: no slack); the replay is this module's split_pass
      collapse  every edge is an edge of the current mesh and a candidate by the restated rules (slack 1e-6), its point
                is the exact fp32 midpoint, the closed neighbourhoods are pairwise disjoint
      flip      every edge is a candidate by the restated rules, its traced corners are the mesh's, the vertex sets
                {a, b, c, d} are pairwise disjoint
      move      vertices that are not movable keep their bits; reverted vertices hold their old position; every other
                one lies within move_tol x the bounding-box diagonal of the float64 restatement (relax, then the
                closest point; where faces tie for the closest point within a relative 1e-6 of the squared distance,
                as on the symmetry planes of the torus, the closest point of any of them); no face is folded
    With final = (v_pos, t_pos_idx) the replay must reproduce them exactly.  Returns the replay's (v_pos, t_pos_idx)
    and its state before the compaction (v_pos with every vertex ever made, the live faces)."""
    v, tri = np.asarray(v, np.float32), np.asarray(tri, np.int64)
    v0, t0 = v.copy(), tri.copy()
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0).astype(np.float64)))
    hi2, lo2 = thresholds(L)
    for i, rec in enumerate(trace):
        kind = rec[0]
        if kind == "split":
            edges = np.asarray(rec[1], np.int64)
            v2, tri2, mine = split_pass(v, tri, hi2)
            assert len(edges) >= 1 and np.array_equal(mine, edges), f"record {i}: the split marks differ from the fp32 rule"
            v, tri = v2, tri2
        elif kind == "collapse":
            edges, x = np.asarray(rec[1], np.int64), np.asarray(rec[2], np.float32)
            assert len(edges) >= 1
            topo, seen = D.Topology(tri, len(v)), set()
            for (a, b), x32 in zip(edges, x):
                a, b = int(a), int(b)
                assert (a, b) in topo.edge_index, f"record {i}: ({a},{b}) is no edge of the mesh"
                assert topo.counts[topo.edge_index[(a, b)]] == 2
                why = collapse_ok(topo, v, a, b, hi2, lo2, slack=SLACK)
                assert why is None, f"record {i}: collapse ({a},{b}) breaks the {why} rule"
                assert np.array_equal(x32.view(np.uint32), midpoint(v[a], v[b]).view(np.uint32)), \
                    f"record {i}: collapse ({a},{b}) point {x32} is not the fp32 midpoint"
                hood = topo.closed(a, b)
                assert not (hood & seen), f"record {i}: the neighbourhood of ({a},{b}) meets another collapse's"
                seen |= hood
            v, tri = apply_collapses(v, tri, edges, x)
        elif kind == "flip":
            edges, cd = np.asarray(rec[1], np.int64), np.asarray(rec[2], np.int64)
            assert len(edges) >= 1
            topo, seen = D.Topology(tri, len(v)), set()
            _, counts, _, order, starts = edge_table(tri, len(v))
            for (a, b), (c, d) in zip(edges, cd):
                a, b, c, d = int(a), int(b), int(c), int(d)
                assert (a, b) in topo.edge_index, f"record {i}: ({a},{b}) is no edge of the mesh"
                q = flip_faces(topo.tri, order, starts, counts, topo.edge_index[(a, b)], a, b)
                assert q is not None and (q[1], q[3]) == (c, d), f"record {i}: flip ({a},{b}) corners {(c, d)}: {q}"
                why = flip_ok(topo, v, a, b, c, d, hi2, slack=SLACK)
                assert why is None, f"record {i}: flip ({a},{b}) breaks the {why} rule"
                assert not ({a, b, c, d} & seen), f"record {i}: flip ({a},{b}) shares a vertex with another flip"
                seen |= {a, b, c, d}
            tri = apply_flips(tri, edges, cd)
        elif kind == "move":
            pos, rev = np.asarray(rec[1], np.float32), np.asarray(rec[2]).astype(bool)
            assert pos.shape == v.shape and rev.shape == (len(v),)
            q, movable = relax(v, tri)
            fixed = ~movable | rev
            assert np.array_equal(pos[fixed].view(np.uint32), v[fixed].view(np.uint32)), \
                f"record {i}: a locked, unreferenced or reverted vertex moved"
            assert not (rev & ~movable).any(), f"record {i}: a vertex that cannot move is marked reverted"
            m = movable & ~rev
            if m.any():
                q32 = q[m].astype(np.float32)
                err = np.linalg.norm(pos[m].astype(np.float64) - project(q32, v0, t0), axis=1)
                for j in np.flatnonzero(err > move_tol * diag):  # a tie between faces, decided by rounding?
                    err[j] = np.linalg.norm(tied_points(q32[j], v0, t0, SLACK) - pos[m][j].astype(np.float64), axis=1).min()
                assert err.max() <= move_tol * diag, \
                    f"record {i}: move off the restatement by {err.max():.3e} (diag {diag:.3e})"
            assert not folded(v, pos, tri).any(), f"record {i}: the move folds a face"
            v = pos.copy()
        else:
            raise AssertionError(f"record {i}: unknown kind {kind!r}")
    out = emit(v, tri)
    if final is not None:
        fv, ft = (np.asarray(x) for x in final)
        assert fv.shape == out[0].shape and np.array_equal(fv.view(np.uint32), out[0].view(np.uint32)), "v_pos differs"
        assert np.array_equal(ft.astype(np.int64), out[1].astype(np.int64)), "t_pos_idx differs"
    return out + (v, tri)


# ---------------------------------------------------------------------------------------------------------------
# metrics
def quality(v, tri, L):
    """The figures of the issue's table: share of edges shorter than 0.8 L, edges with len2 > hi2, mean and 5th
    percentile of the faces' minimum angle (degrees), mean |valence - 6| over the referenced vertices."""
    v, tri = np.asarray(v, np.float32), np.asarray(tri, np.int64)
    e = edge_table(tri, len(v))[0]
    p = v.astype(np.float64)
    length = np.linalg.norm(p[e[:, 0]] - p[e[:, 1]], axis=1)
    c = p[tri]
    ang = []
    for k in range(3):
        x, y = c[:, (k + 1) % 3] - c[:, k], c[:, (k + 2) % 3] - c[:, k]
        cos = (x * y).sum(1) / np.maximum(np.linalg.norm(x, axis=1) * np.linalg.norm(y, axis=1), 1e-300)
        ang.append(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))))
    amin = np.min(ang, 0)
    val = np.bincount(e.reshape(-1), minlength=len(v))
    return {"faces": len(tri), "short_share": float((length < 0.8 * L).mean()),
            "n_long": int((len2(v[e[:, 0]], v[e[:, 1]]) > thresholds(L)[0]).sum()),
            "min_angle_mean": float(amin.mean()), "min_angle_p5": float(np.percentile(amin, 5)),
            "valence_dev": float(np.abs(val[val > 0] - 6).mean())}
