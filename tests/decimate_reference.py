"""Test-only numpy restatement of the mesh decimation contract (include/tt_abi.h, "mesh decimation") and a checker
of the traces ops.mesh_decimate returns.  Everything is sequential fp64 numpy, written from the contract text.

  restatement   Topology (edges, counts, locks, the two CSR tables), vertex_quadrics, solve_edge, edge_valid,
                round_edges (cost and validity of every edge), select (threshold, hashed priorities, passes, budget),
                apply_round, emit, decimate (the whole loop)
  checker       check_trace(v, tri, trace, ...): replays a trace round by round and asserts what the contract
                guarantees of every kept collapse

Two places of the contract are decided by comparing fp64 numbers that rounding can move: the choice between the solve
and the three-candidate fallback (|det| against 1e-9 (trace/3)^3) and the choice among the three candidates (ties on
a flat neighbourhood are ties of rounding noise).  The checker therefore accepts, for a kept edge, the optimal point of
either branch when |det| is within 1e-6 (relative) of the threshold, and in the fallback any candidate whose restated
cost is within the cost tolerance of the cheapest.  Everywhere else a kept edge's point must be within 1e-5 x the
bounding-box diagonal of the restatement's and its cost within rel 1e-3 + abs 1e-12 diag^2."""
import numpy as np

INVALID = 0xFFFFFFFF
QUANTILE = 0.25
PASSES = 2
FLIP_COS = 0.2
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------
# meshes
def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    t = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, t


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    t = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, t


def icosphere(n, noise=0.0, seed=0):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p],
         [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]]
    t = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(n):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        t = nt
    v = np.asarray(v, np.float64)
    if noise:
        v = v * (1.0 + noise * np.random.default_rng(seed).uniform(-1.0, 1.0, (len(v), 1)))
    return v.astype(np.float32), np.asarray(t, np.int32)


def torus(nu=32, nv=16, R=1.0, r=0.4):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32), t.astype(np.int32)


def height_field(n, amp=0.05, fx=7.0, fy=5.0):
    x, y = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    v = np.stack([x, y, amp * np.sin(fx * x) * np.cos(fy * y)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.astype(np.float32), t.astype(np.int32)


def two_tetrahedra_sharing_an_edge():
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [0.5, 1, 0.5], [-1, 0, 0.5], [-0.5, -1, 0.5]], np.float32)
    t = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2], [0, 1, 4], [0, 5, 1], [0, 4, 5], [1, 5, 4]], np.int32)
    return v, t


def manifold_stats(tri):
    """(every edge has exactly two faces, Euler characteristic V - E + F over the referenced vertices, components)"""
    tri = np.asarray(tri, np.int64)
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), 1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    verts = np.unique(tri)
    parent = {int(x): int(x) for x in verts}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in ue:
        parent[find(int(a))] = find(int(b))
    comps = len({find(int(x)) for x in verts})
    return bool((cnt == 2).all()), int(len(verts) - len(ue) + len(tri)), comps


# ---------------------------------------------------------------------------------------------------------------
# restatement
def hash32(a, b, rnd):
    h = ((a * 0x9E3779B1) & M32) ^ (((b + 0x7F4A7C15) & M32) * 0x85EBCA77 & M32) ^ (((rnd + 1) * 0xC2B2AE3D) & M32)
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


class Topology:
    """Step 1 and 2 of a round: unique edges (a <= b, lexicographic) with their face-edge counts, the vertex ->
    neighbour CSR (ascending rows), the vertex -> face-corner CSR (ascending) and the locked vertices."""

    def __init__(self, tri, V):
        tri = np.asarray(tri, np.int64)
        self.tri, self.V = tri, V
        a, b = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)
        key, self.counts = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
        self.edges = np.stack([key // V, key % V], 1)
        self.edge_index = {(int(x), int(y)): i for i, (x, y) in enumerate(self.edges)}
        row = np.concatenate([self.edges[:, 0], self.edges[:, 1]])
        col = np.concatenate([self.edges[:, 1], self.edges[:, 0]])
        o = np.lexsort((col, row))
        self.nbr_col = col[o]
        self.nbr_ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=V))])
        self.vf_col = np.argsort(tri.reshape(-1), kind="stable")
        self.vf_ptr = np.concatenate([[0], np.cumsum(np.bincount(tri.reshape(-1), minlength=V))])
        self.locked = np.zeros(V, bool)
        bad = (self.counts != 2) | (self.edges[:, 0] == self.edges[:, 1])
        self.locked[self.edges[bad].reshape(-1)] = True

    def N(self, v):
        return self.nbr_col[self.nbr_ptr[v]:self.nbr_ptr[v + 1]]

    def faces(self, v):
        return self.vf_col[self.vf_ptr[v]:self.vf_ptr[v + 1]] // 3

    def closed(self, a, b):
        return set(self.N(a).tolist()) | set(self.N(b).tolist()) | {int(a), int(b)}


def vertex_quadrics(v, tri):
    """(V,10) fp64: a00 a01 a02 a11 a12 a22 b0 b1 b2 c of every vertex, from its faces in ascending face order."""
    p = np.asarray(v, np.float64)[np.asarray(tri, np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    l = np.sqrt((n * n).sum(1))
    ok = l > 0
    nh = n / np.where(ok, l, 1.0)[:, None]
    area, d = 0.5 * l, -(nh * p[:, 0]).sum(1)
    k = np.stack([nh[:, 0] * nh[:, 0], nh[:, 0] * nh[:, 1], nh[:, 0] * nh[:, 2], nh[:, 1] * nh[:, 1],
                  nh[:, 1] * nh[:, 2], nh[:, 2] * nh[:, 2], d * nh[:, 0], d * nh[:, 1], d * nh[:, 2], d * d], 1)
    k = np.where(ok[:, None], k * area[:, None], 0.0)
    Q = np.zeros((len(v), 10))
    order = np.argsort(np.asarray(tri, np.int64).reshape(-1), kind="stable")  # corners by vertex, ascending face
    np.add.at(Q, np.asarray(tri, np.int64).reshape(-1)[order], k[order // 3])
    return Q


def qcost(q, x):
    A = np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
    return float(x @ A @ x + 2.0 * (q[6:9] @ x) + q[9])


def solve_edge(q, va, vb):
    """The contract's optimal point of a quadric q = Qa + Qb: (x fp64, cost fp64, alternatives) where alternatives
    lists every (x, cost) the checker accepts (see the module docstring)."""
    c00, c01, c02 = q[3] * q[5] - q[4] * q[4], q[2] * q[4] - q[1] * q[5], q[1] * q[4] - q[2] * q[3]
    c11, c12, c22 = q[0] * q[5] - q[2] * q[2], q[1] * q[2] - q[0] * q[4], q[0] * q[3] - q[1] * q[1]
    det, tr = q[0] * c00 + q[1] * c01 + q[2] * c02, (q[0] + q[3] + q[5]) / 3.0
    thr = 1e-9 * tr * tr * tr
    va, vb = np.asarray(va, np.float64), np.asarray(vb, np.float64)
    cands = [(c, qcost(q, c)) for c in (va, vb, 0.5 * (va + vb))]
    best = cands[0]
    for c in cands[1:]:
        if c[1] < best[1]:
            best = c
    solved = None
    if det != 0.0:
        b = q[6:9]
        x = -np.array([c00 * b[0] + c01 * b[1] + c02 * b[2], c01 * b[0] + c11 * b[1] + c12 * b[2],
                       c02 * b[0] + c12 * b[1] + c22 * b[2]]) / det
        solved = (x, qcost(q, x))
    use_solve = abs(det) > thr
    ambiguous = abs(abs(det) - thr) <= 1e-6 * abs(thr)
    alts = []
    if (use_solve or ambiguous) and solved is not None:
        alts.append(solved + (None,))
    if not use_solve or ambiguous:
        alts += [c + (best[1],) for c in cands]  # a candidate is acceptable only if it is (one of) the cheapest
    x, cost = solved if use_solve else best
    return x, cost, alts


def cost_bits_of(cost):
    return int(np.float32(max(cost, 0.0)).view(np.uint32))


def flip_ok(topo, v, a, b, x32, slack=0.0):
    """The flip rule for the faces of star(a) u star(b) without both endpoints, corner a or b at the fp32 x."""
    p = np.asarray(v, np.float64)
    x = np.asarray(x32, np.float32).astype(np.float64)
    for w, other in ((a, b), (b, a)):
        f = topo.faces(w)
        t = topo.tri[f]
        t = t[~(t == other).any(1)]
        if not len(t):
            continue
        old = p[t]
        new = np.where((t == w)[:, :, None], x[None, None, :], old)
        n0 = np.cross(old[:, 1] - old[:, 0], old[:, 2] - old[:, 0])
        n1 = np.cross(new[:, 1] - new[:, 0], new[:, 2] - new[:, 0])
        oo, nn, on = (n0 * n0).sum(1), (n1 * n1).sum(1), (n0 * n1).sum(1)
        if not ((nn > 0) & (on > (FLIP_COS - slack) * np.sqrt(oo) * np.sqrt(nn))).all():
            return False
    return True


def link_ok(topo, a, b):
    """Every validity rule of the contract except the flip test; the reason it fails, or None."""
    if a == b or topo.locked[a] or topo.locked[b]:
        return "locked"
    na, nb = topo.N(a), topo.N(b)
    if len(na) + len(nb) - 4 < 3:
        return "degree"
    common = np.intersect1d(na, nb)
    if len(common) != 2:
        return "link"
    if any(len(topo.N(c)) < 4 for c in common):
        return "valence"
    return None


def round_edges(v, tri, Q, check_flip=True):
    """Step 3 for every edge, sequentially: (topo, cost_bits (E) int64 with INVALID, xopt (E,3) fp32, would_flip (E)
    bool: passes every other rule but not the flip test -- with check_flip False such an edge is valid)."""
    topo = Topology(tri, len(v))
    E = len(topo.edges)
    cost_bits, xopt, would_flip = np.full(E, INVALID, np.int64), np.zeros((E, 3), np.float32), np.zeros(E, bool)
    for e, (a, b) in enumerate(topo.edges):
        a, b = int(a), int(b)
        if link_ok(topo, a, b) is not None:
            continue
        x, cost, _ = solve_edge(Q[a] + Q[b], v[a], v[b])
        x32 = x.astype(np.float32)
        if not flip_ok(topo, v, a, b, x32):
            would_flip[e] = True
            if check_flip:
                continue
        cost_bits[e], xopt[e] = cost_bits_of(cost), x32
    return topo, cost_bits, xopt, would_flip


def select(topo, cost_bits, rnd, need, quantile=QUANTILE, passes=PASSES):
    """Steps 4 to 6: the kept edge indices, ascending."""
    valid = np.flatnonzero(cost_bits != INVALID)
    if not len(valid):
        return valid
    tau = np.sort(cost_bits[valid])[int(np.floor(quantile * len(valid)))]
    state = {int(e): 1 for e in valid if cost_bits[e] <= tau}
    key = {e: (hash32(int(topo.edges[e, 0]), int(topo.edges[e, 1]), rnd) << 32) | e for e in state}
    hood = {e: topo.closed(*topo.edges[e]) for e in state}
    taken = set()
    for _ in range(passes):
        owner = {}
        for e, s in state.items():
            if s != 1:
                continue
            if hood[e] & taken:
                state[e] = 3
                continue
            for w in hood[e]:
                owner[w] = min(owner.get(w, 1 << 64), key[e])
        won = [e for e, s in state.items() if s == 1 and all(owner[w] == key[e] for w in hood[e])]
        for e in won:
            state[e] = 2
            taken |= hood[e]
    sel = sorted(e for e, s in state.items() if s == 2)
    if len(sel) > need:
        sel = sorted(sorted(sel, key=lambda e: (cost_bits[e], e))[:need])
    return np.asarray(sel, np.int64)


def apply_round(v, tri, Q, root, edges, xopt):
    """Step 7: the state after the collapses b -> a of `edges` (k,2) at `xopt` (k,3) fp32."""
    v, Q = np.array(v, np.float32), np.array(Q)
    remap = np.arange(len(v))
    for (a, b), x in zip(np.asarray(edges, np.int64), np.asarray(xopt, np.float32)):
        v[a] = x
        Q[a] = Q[a] + Q[b]
        remap[b] = a
    t = remap[np.asarray(tri, np.int64)]
    keep = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
    return v, t[keep], Q, remap[root]


def emit(v, tri, root):
    used = np.zeros(len(v), bool)
    used[tri.reshape(-1)] = True
    new = np.cumsum(used) - 1
    vertex_map = np.where(used[root], new[root], -1).astype(np.int32)
    return np.asarray(v, np.float32)[used], new[tri].astype(np.int32), vertex_map


def decimate(v, tri, target_faces, max_rounds=1024, check_flip=True):
    """The whole loop, sequentially: (v', t', info) with info as ops.mesh_decimate's (numpy; the trace always)."""
    v, tri = np.asarray(v, np.float32), np.asarray(tri, np.int64)
    V = len(v)
    Q, root, trace, stalled, n_locked = vertex_quadrics(v, tri), np.arange(V), [], False, 0
    rnd = 0
    while len(tri) > target_faces and rnd < max_rounds:
        topo, cost_bits, xopt, _ = round_edges(v, tri, Q, check_flip)
        if rnd == 0:
            n_locked = int(topo.locked.sum())
        kept = select(topo, cost_bits, rnd, (len(tri) - target_faces + 1) // 2)
        if not len(kept):
            stalled = True
            break
        trace.append((topo.edges[kept].astype(np.int32), xopt[kept], cost_bits[kept]))
        v, tri, Q, root = apply_round(v, tri, Q, root, topo.edges[kept], xopt[kept])
        rnd += 1
    v_out, t_out, vertex_map = emit(v, tri, root)
    return v_out, t_out, {"target_faces": target_faces, "n_rounds": rnd, "stalled": stalled, "n_locked": n_locked,
                          "vertex_map": vertex_map, "trace": trace}


# ---------------------------------------------------------------------------------------------------------------
# checker
def check_trace(v, tri, trace, target_faces, final=None, stalled=False, validate=True):
    """Replays `trace` (a list of (edges (k,2), xopt (k,3) fp32, cost_bits (k,)) per round, as ops.mesh_decimate
    returns it, numpy) on the input mesh and asserts, per round: every kept edge is an edge of the current mesh and
    valid by the restatement's rules at the traced point (flip slack 1e-6); the kept closed neighbourhoods are pairwise
    disjoint; at least one edge is kept and no more than the budget; point and cost agree with the restatement.  With
    stalled it asserts that the mesh left over has no valid edge (flip margin 1e-6).  With final = (v_pos, t_pos_idx,
    vertex_map) it asserts that the replay reproduces them exactly.  validate=False only replays (remap and in-order
    compaction of the traced collapses) and compares.  Returns the replay's (v_pos, t_pos_idx,
    vertex_map)."""
    v, tri = np.asarray(v, np.float32), np.asarray(tri, np.int64)
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0).astype(np.float64)))
    Q, root = vertex_quadrics(v, tri), np.arange(len(v))
    for rnd, (edges, xopt, cost_bits) in enumerate(trace):
        edges, xopt = np.asarray(edges, np.int64), np.asarray(xopt, np.float32)
        cost = np.asarray(cost_bits, np.int64).astype(np.uint32).view(np.float32).astype(np.float64)
        assert len(tri) > target_faces, f"round {rnd}: ran at {len(tri)} faces, target {target_faces}"
        assert 1 <= len(edges) <= (len(tri) - target_faces + 1) // 2, f"round {rnd}: {len(edges)} kept edges"
        topo = Topology(tri, len(v)) if validate else None
        seen = set()
        for (a, b), x32, c in zip(edges, xopt, cost) if validate else ():
            a, b = int(a), int(b)
            assert (a, b) in topo.edge_index, f"round {rnd}: ({a},{b}) is no edge of the mesh"
            why = link_ok(topo, a, b)
            assert why is None, f"round {rnd}: edge ({a},{b}) breaks the {why} rule"
            assert flip_ok(topo, v, a, b, x32, slack=1e-6), f"round {rnd}: edge ({a},{b}) flips a face"
            hood = topo.closed(a, b)
            assert not (hood & seen), f"round {rnd}: the neighbourhood of ({a},{b}) meets another kept edge's"
            seen |= hood
            alts = solve_edge(Q[a] + Q[b], v[a], v[b])[2]
            tol = lambda ref: 1e-3 * abs(ref) + 1e-12 * diag * diag
            match = [xr for xr, cr, floor in alts
                     if np.linalg.norm(xr - x32.astype(np.float64)) <= 1e-5 * diag
                     and abs(max(cr, 0.0) - c) <= tol(max(cr, 0.0)) and (floor is None or cr <= floor + tol(floor))]
            assert match, f"round {rnd}: edge ({a},{b}) point {x32} cost {c} against {alts}"
        v, tri, Q, root = apply_round(v, tri, Q, root, edges, xopt)
    if stalled:
        assert len(tri) > target_faces
        topo = Topology(tri, len(v))
        for a, b in topo.edges:
            a, b = int(a), int(b)
            if link_ok(topo, a, b) is None:
                x = solve_edge(Q[a] + Q[b], v[a], v[b])[0].astype(np.float32)
                assert not flip_ok(topo, v, a, b, x, slack=-1e-6), f"stalled, but edge ({a},{b}) is valid"
    out = emit(v, tri, root)
    if final is not None:
        fv, ft, fm = (np.asarray(x) for x in final)
        assert fv.shape == out[0].shape and np.array_equal(fv.view(np.uint32), out[0].view(np.uint32)), "v_pos differs"
        assert np.array_equal(ft.astype(np.int64), out[1].astype(np.int64)), "t_pos_idx differs"
        assert np.array_equal(fm.astype(np.int64), out[2].astype(np.int64)), "vertex_map differs"
    return out
