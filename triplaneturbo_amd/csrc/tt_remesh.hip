// tt_remesh.hip -- isotropic remeshing (Botsch & Kobbelt 2004): split the long edges, collapse the short ones, flip
// towards valence 6, relax tangentially and pull back onto the input surface.  The contract (thresholds, templates,
// candidates, independent sets, move and fold guard, output, determinism, guarantees) is written in include/tt_abi.h,
// "isotropic remeshing".  The topology of a round (one face-edge sort, the vertex -> neighbour and vertex -> face CSR
// tables, the face edges of every unique edge) is torch on the host side (ops.mesh_remesh), the closest point of the
// input mesh is tt_dist_query, the selection, the application of a collapse round and the final compaction are
// tt_decimate_mark / _select / _apply / _emit; everything else is here:
//   k_rm_split_mark    one thread per unique edge: len2 > hi2
//   k_rm_split_count   one thread per item (edge | face): marked edges and child faces, first level of the compaction
//   k_rm_split_emit    one thread per item: the midpoints and the marked edges in order, the children by template
//   k_rm_collapse_cand one thread per unique edge: the candidate rules at the fp32 midpoint
//   k_rm_flip_cand / _mark / _select / _apply   one thread per unique edge: the flip rules, a 64-bit atomicMin of the
//                      key into owner[] of a, b, c, d, selected iff it owns the four, the two faces rewritten in place
//   k_rm_relax         one thread per vertex: the tangential step, fp64
//   k_rm_place         one thread per vertex: the closest point from its face and barycentrics
//   k_rm_fold_flag / k_rm_revert   one thread per face / vertex: the fold guard, Jacobi
// The star loops walk the CSR rows with scalars only (no per-thread arrays).  No float atomics: an integer min, an
// integer add for a count and flag stores, so identical inputs give bit-identical outputs.
#include "tt_decimate.h"

#pragma clang fp contract(off)  // the fp32 lengths and midpoints exactly as written: the host restates them bit for bit

struct RmWs {
    int* misc;            // [0..1] totals of the last compaction
    unsigned char* mark;  // [E] edge is split in this pass
    TtCompact2 c;         // items: max(E, T); low counter: marked edges, high: child faces
};

struct RmLayout {
    RmWs w;
    long long bytes;
};

// the workspace sections (tt_remesh_workspace_bytes); base may be null for the size alone
static RmLayout rm_layout(void* base, long long E, long long T) {
    TtCarver c{(char*)base};
    RmLayout l;
    l.w.misc = c.take<int>(64);
    l.w.mark = c.take<unsigned char>(E);
    l.w.c = tt_compact2_carve(c, E > T ? E : T, base ? l.w.misc : nullptr);
    l.bytes = c.bytes();
    return l;
}

struct RmF3 {
    float x, y, z;
};

__device__ __forceinline__ RmF3 rm_pos(const float* __restrict__ v_pos, unsigned v) {
    return RmF3{v_pos[(size_t)v * 3], v_pos[(size_t)v * 3 + 1], v_pos[(size_t)v * 3 + 2]};
}
// (dx dx + dy dy) + dz dz, every operation rounded to fp32
__device__ __forceinline__ float rm_len2(RmF3 p, RmF3 q) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ RmF3 rm_mid(RmF3 p, RmF3 q) {
    return RmF3{0.5f * (p.x + q.x), 0.5f * (p.y + q.y), 0.5f * (p.z + q.z)};
}
__device__ __forceinline__ DecP rm_wide(RmF3 p) { return DecP{(double)p.x, (double)p.y, (double)p.z}; }

// ---------------------------------------------------------------------------------------------------------------
// split
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEC_BLOCK) void k_rm_split_mark(const float* __restrict__ v_pos,
                                                             const int* __restrict__ edges, int V, int E, float hi2,
                                                             unsigned char* __restrict__ mark) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    const unsigned a = (unsigned)edges[(size_t)e * 2], b = (unsigned)edges[(size_t)e * 2 + 1];
    unsigned char m = 0;
    if (a < (unsigned)V && b < (unsigned)V && a != b) m = (unsigned char)(rm_len2(rm_pos(v_pos, a), rm_pos(v_pos, b)) > hi2);
    mark[e] = m;
}

// the unique edge of face edge 3f + k, clamped into [0, E)
__device__ __forceinline__ int rm_face_edge(const int* __restrict__ fe2e, int f, int k, int E) {
    return dec_clamp(fe2e[(size_t)f * 3 + k], 0, E - 1);
}

__global__ __launch_bounds__(DEC_BLOCK) void k_rm_split_count(const int* __restrict__ fe2e, int T, int E, RmWs w) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    unsigned lo = 0, hi = 0;
    if (i < E) lo = w.mark[i];
    if (i < T) {
        hi = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) hi += w.mark[rm_face_edge(fe2e, i, k, E)];
    }
    tt_compact2_first_level<4>(w.c, lo, hi);
}

__device__ __forceinline__ void rm_put(int* __restrict__ t_out, int o, int Tn, int x, int y, int z) {
    if ((unsigned)o >= (unsigned)Tn) return;  // bound of every face write: the buffer
    t_out[(size_t)o * 3] = x;
    t_out[(size_t)o * 3 + 1] = y;
    t_out[(size_t)o * 3 + 2] = z;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_rm_split_emit(const float* __restrict__ v_pos,
                                                             const int* __restrict__ tri,
                                                             const int* __restrict__ edges,
                                                             const int* __restrict__ fe2e, int V, int T, int E, int M,
                                                             int Tn, RmWs w, float* __restrict__ v_new,
                                                             int* __restrict__ marked, int* __restrict__ t_out) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    const int nm = min(w.misc[0], M), nt = min(w.misc[1], Tn);  // the totals the scan produced, and the buffers
    if (i < E && w.mark[i]) {
        const int r = tt_compact2_lo(w.c, i);
        const unsigned a = (unsigned)edges[(size_t)i * 2], b = (unsigned)edges[(size_t)i * 2 + 1];
        if ((unsigned)r < (unsigned)nm && a < (unsigned)V && b < (unsigned)V) {
            const RmF3 m = rm_mid(rm_pos(v_pos, a), rm_pos(v_pos, b));
            v_new[(size_t)r * 3] = m.x;
            v_new[(size_t)r * 3 + 1] = m.y;
            v_new[(size_t)r * 3 + 2] = m.z;
            marked[(size_t)r * 2] = (int)a;
            marked[(size_t)r * 2 + 1] = (int)b;
        }
    }
    if (i >= T) return;
    const int o = tt_compact2_hi(w.c, i);
    int c0 = tri[(size_t)i * 3], c1 = tri[(size_t)i * 3 + 1], c2 = tri[(size_t)i * 3 + 2];
    if ((unsigned)max(max(c0, c1), c2) >= (unsigned)V || min(min(c0, c1), c2) < 0) {  // never with a checked mesh
        rm_put(t_out, o, nt, c0, c1, c2);
        return;
    }
    // the midpoint vertex of edge k (corners k, k + 1), -1 when the edge is not split
    int m0, m1, m2;
    {
        const int e0 = rm_face_edge(fe2e, i, 0, E), e1 = rm_face_edge(fe2e, i, 1, E), e2 = rm_face_edge(fe2e, i, 2, E);
        m0 = w.mark[e0] ? V + tt_compact2_lo(w.c, e0) : -1;
        m1 = w.mark[e1] ? V + tt_compact2_lo(w.c, e1) : -1;
        m2 = w.mark[e2] ? V + tt_compact2_lo(w.c, e2) : -1;
    }
    const int n = (int)(m0 >= 0) + (int)(m1 >= 0) + (int)(m2 >= 0);
    if (n == 0) {
        rm_put(t_out, o, nt, c0, c1, c2);
    } else if (n == 3) {
        rm_put(t_out, o, nt, c0, m0, m2);
        rm_put(t_out, o + 1, nt, c1, m1, m0);
        rm_put(t_out, o + 2, nt, c2, m2, m1);
        rm_put(t_out, o + 3, nt, m0, m1, m2);
    } else {
        // rotate: one split edge -> it becomes edge 0 (a, b); two -> the edge that is NOT split becomes edge 0
        const int k = n == 1 ? (m0 >= 0 ? 0 : (m1 >= 0 ? 1 : 2)) : (m0 < 0 ? 0 : (m1 < 0 ? 1 : 2));
        int a = c0, b = c1, c = c2, ma = m0, mb = m1, mc = m2;  // ma: midpoint of (a, b), mb: of (b, c), mc: of (c, a)
        if (k == 1) a = c1, b = c2, c = c0, ma = m1, mb = m2, mc = m0;
        if (k == 2) a = c2, b = c0, c = c1, ma = m2, mb = m0, mc = m1;
        if (n == 1) {
            rm_put(t_out, o, nt, a, ma, c);
            rm_put(t_out, o + 1, nt, ma, b, c);
        } else {
            // corner c is cut off; the quad a, b, mb, mc is cut by its shorter diagonal, a tie from the smaller id
            const RmF3 pa = rm_pos(v_pos, (unsigned)a), pb = rm_pos(v_pos, (unsigned)b), pc = rm_pos(v_pos, (unsigned)c);
            const float da = rm_len2(pa, rm_mid(pb, pc)), db = rm_len2(pb, rm_mid(pc, pa));
            const bool from_a = da < db || (da == db && a < b);
            rm_put(t_out, o, nt, mb, c, mc);
            rm_put(t_out, o + 1, nt, a, b, from_a ? mb : mc);
            rm_put(t_out, o + 2, nt, from_a ? a : b, mb, mc);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// collapse candidates
// ---------------------------------------------------------------------------------------------------------------
// 1 when no vertex of the row of v other than a and b is farther than hi2 (squared, fp32) from x
__device__ __forceinline__ unsigned rm_ring_ok(const float* __restrict__ v_pos, const DecTopo& t, unsigned v, unsigned a,
                                               unsigned b, RmF3 x, float hi2) {
    unsigned ok = 1;
    const int rb = dec_clamp(t.nbr_ptr[v], 0, t.NN), re = dec_clamp(t.nbr_ptr[v + 1], 0, t.NN);
    for (int i = rb; i < re; ++i) {
        const unsigned w = (unsigned)t.nbr_col[i];
        if (w >= (unsigned)t.V || w == a || w == b) continue;
        ok &= (unsigned)(rm_len2(rm_pos(v_pos, w), x) <= hi2);
    }
    return ok;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_rm_collapse_cand(const float* __restrict__ v_pos,
                                                                const int* __restrict__ tri,
                                                                const int* __restrict__ edges,
                                                                const unsigned char* __restrict__ locked, DecTopo t,
                                                                int E, float hi2, float lo2,
                                                                unsigned* __restrict__ cost_bits,
                                                                float* __restrict__ xopt) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    cost_bits[e] = DEC_INVALID;
#pragma unroll
    for (int k = 0; k < 3; ++k) xopt[(size_t)e * 3 + k] = 0.f;
    const unsigned a = (unsigned)edges[(size_t)e * 2], b = (unsigned)edges[(size_t)e * 2 + 1];
    if (a >= (unsigned)t.V || b >= (unsigned)t.V || a == b) return;
    if (locked[a] | locked[b]) return;  // an unlocked endpoint has two faces on every edge
    const RmF3 pa = rm_pos(v_pos, a), pb = rm_pos(v_pos, b);
    if (!(rm_len2(pa, pb) < lo2)) return;
    const int a0 = dec_clamp(t.nbr_ptr[a], 0, t.NN), a1 = dec_clamp(t.nbr_ptr[a + 1], 0, t.NN);
    const int b0 = dec_clamp(t.nbr_ptr[b], 0, t.NN), b1 = dec_clamp(t.nbr_ptr[b + 1], 0, t.NN);
    if ((a1 - a0) + (b1 - b0) - 4 < 3) return;
    // the link condition, as decimation's: a merge of the two ascending rows
    int i = a0, j = b0, common = 0, thin = 0;
    while (i < a1 && j < b1) {
        const int x = t.nbr_col[i], y = t.nbr_col[j];
        if (x == y) {
            const int c = dec_clamp(x, 0, t.V - 1);
            ++common;
            thin += (int)(t.nbr_ptr[c + 1] - t.nbr_ptr[c] < 4);
        }
        i += (int)(x <= y);
        j += (int)(y <= x);
    }
    if (common != 2 || thin != 0) return;
    const RmF3 x = rm_mid(pa, pb);
    if (!rm_ring_ok(v_pos, t, a, a, b, x, hi2)) return;
    if (!rm_ring_ok(v_pos, t, b, a, b, x, hi2)) return;
    if (!dec_star_ok(v_pos, tri, t, a, b, rm_wide(x))) return;
    if (!dec_star_ok(v_pos, tri, t, b, a, rm_wide(x))) return;
    cost_bits[e] = 0u;  // every candidate is eligible: one cost, and the threshold of tt_decimate_mark at 0
    xopt[(size_t)e * 3] = x.x;
    xopt[(size_t)e * 3 + 1] = x.y;
    xopt[(size_t)e * 3 + 2] = x.z;
}

// ---------------------------------------------------------------------------------------------------------------
// flip
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rm_degree(const DecTopo& t, unsigned v) {
    return dec_clamp(t.nbr_ptr[v + 1], 0, t.NN) - dec_clamp(t.nbr_ptr[v], 0, t.NN);
}
// |valence + delta - target| with the target 6 for an unlocked and 4 for a locked vertex
__device__ __forceinline__ int rm_dev(const DecTopo& t, const unsigned char* __restrict__ locked, unsigned v, int delta) {
    return abs(rm_degree(t, v) + delta - (locked[v] ? 4 : 6));
}
// how often w stands in the row of v (a count, not an OR of compare masks: DESIGN.md section 6)
__device__ __forceinline__ int rm_count_edge(const DecTopo& t, unsigned v, unsigned w) {
    const int rb = dec_clamp(t.nbr_ptr[v], 0, t.NN), re = dec_clamp(t.nbr_ptr[v + 1], 0, t.NN);
    int n = 0;
    for (int i = rb; i < re; ++i) n += (int)((unsigned)t.nbr_col[i] == w);
    return n;
}

// face edge fe = 3f + k of a mesh of T faces: corners k, k + 1 and the opposite one; false when out of range
__device__ __forceinline__ bool rm_corner(const int* __restrict__ tri, int T, int V, int fe, unsigned* u, unsigned* w,
                                          unsigned* o) {
    if (fe < 0 || fe >= 3 * T) return false;
    const int f = fe / 3, k = fe - 3 * f;
    *u = (unsigned)tri[(size_t)f * 3 + k];
    *w = (unsigned)tri[(size_t)f * 3 + (k + 1) % 3];
    *o = (unsigned)tri[(size_t)f * 3 + (k + 2) % 3];
    return max(*u, max(*w, *o)) < (unsigned)V;
}

// state of an edge: 0 no candidate, 1 candidate, 2 selected.  cd[e] = (c, d), the corners opposite the edge in the face
// that runs a -> b and in the face that runs b -> a; ff[e] = those two faces
__global__ __launch_bounds__(DEC_BLOCK) void k_rm_flip_cand(const float* __restrict__ v_pos,
                                                            const int* __restrict__ tri,
                                                            const int* __restrict__ edges,
                                                            const int* __restrict__ edge_fe,
                                                            const unsigned char* __restrict__ locked, DecTopo t, int E,
                                                            float hi2, unsigned char* __restrict__ state,
                                                            int* __restrict__ cd, int* __restrict__ ff) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    state[e] = 0;
    cd[(size_t)e * 2] = cd[(size_t)e * 2 + 1] = -1;
    ff[(size_t)e * 2] = ff[(size_t)e * 2 + 1] = -1;
    const unsigned a = (unsigned)edges[(size_t)e * 2], b = (unsigned)edges[(size_t)e * 2 + 1];
    if (a >= (unsigned)t.V || b >= (unsigned)t.V || a == b) return;
    if (locked[a] | locked[b]) return;
    int fe0 = edge_fe[(size_t)e * 2], fe1 = edge_fe[(size_t)e * 2 + 1];
    unsigned u0, w0, c, u1, w1, d;
    if (!rm_corner(tri, t.T, t.V, fe0, &u0, &w0, &c) || !rm_corner(tri, t.T, t.V, fe1, &u1, &w1, &d)) return;
    if (u0 == b) {  // the first face runs b -> a: swap the two
        unsigned s;
        s = u0, u0 = u1, u1 = s;
        s = w0, w0 = w1, w1 = s;
        s = c, c = d, d = s;
        const int q = fe0;
        fe0 = fe1, fe1 = q;
    }
    if (u0 != a || w0 != b || u1 != b || w1 != a) return;  // two faces of the same direction
    if (c == d || c == a || c == b || d == a || d == b) return;
    if (rm_count_edge(t, c, d) != 0) return;
    const int before = rm_dev(t, locked, a, 0) + rm_dev(t, locked, b, 0) + rm_dev(t, locked, c, 0) + rm_dev(t, locked, d, 0);
    const int after = rm_dev(t, locked, a, -1) + rm_dev(t, locked, b, -1) + rm_dev(t, locked, c, 1) + rm_dev(t, locked, d, 1);
    if (!(after < before)) return;
    const RmF3 fc = rm_pos(v_pos, c), fd = rm_pos(v_pos, d);
    if (!(rm_len2(fc, fd) <= hi2)) return;
    const DecP pa = dec_pos(v_pos, a), pb = dec_pos(v_pos, b), pc = rm_wide(fc), pd = rm_wide(fd);
    const DecP o0 = dec_cross(dec_sub(pb, pa), dec_sub(pc, pa)), o1 = dec_cross(dec_sub(pa, pb), dec_sub(pd, pb));
    const DecP n0 = dec_cross(dec_sub(pd, pa), dec_sub(pc, pa)), n1 = dec_cross(dec_sub(pb, pd), dec_sub(pc, pd));
    unsigned ok = (unsigned)(dec_dot(n0, o0) > 0.0);
    ok &= (unsigned)(dec_dot(n0, o1) > 0.0);
    ok &= (unsigned)(dec_dot(n1, o0) > 0.0);
    ok &= (unsigned)(dec_dot(n1, o1) > 0.0);
    if (!ok) return;
    state[e] = 1;
    cd[(size_t)e * 2] = (int)c;
    cd[(size_t)e * 2 + 1] = (int)d;
    ff[(size_t)e * 2] = fe0 / 3;
    ff[(size_t)e * 2 + 1] = fe1 / 3;
}

// f(w) for the four vertices of a flip; false when one is out of range
template <class F>
__device__ __forceinline__ bool rm_flip_quad(const int* __restrict__ edges, const int* __restrict__ cd, int e, int V,
                                             F f) {
    const unsigned q[4] = {(unsigned)edges[(size_t)e * 2], (unsigned)edges[(size_t)e * 2 + 1],
                           (unsigned)cd[(size_t)e * 2], (unsigned)cd[(size_t)e * 2 + 1]};
    if (max(max(q[0], q[1]), max(q[2], q[3])) >= (unsigned)V) return false;
#pragma unroll
    for (int k = 0; k < 4; ++k) f(q[k]);
    return true;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_rm_flip_mark(const int* __restrict__ edges, const int* __restrict__ cd,
                                                            const unsigned char* __restrict__ state, int V, int E,
                                                            int round, unsigned long long* __restrict__ owner) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E || state[e] != 1) return;
    const unsigned long long key =
        ((unsigned long long)dec_hash((unsigned)edges[(size_t)e * 2], (unsigned)edges[(size_t)e * 2 + 1], (unsigned)round) << 32) |
        (unsigned)e;
    rm_flip_quad(edges, cd, e, V, [&](unsigned w) { atomicMin(owner + w, key); });
}

__global__ __launch_bounds__(DEC_BLOCK) void k_rm_flip_select(const int* __restrict__ edges, const int* __restrict__ cd,
                                                              int V, int E, int round,
                                                              const unsigned long long* __restrict__ owner,
                                                              unsigned char* __restrict__ state) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E || state[e] != 1) return;
    const unsigned long long key =
        ((unsigned long long)dec_hash((unsigned)edges[(size_t)e * 2], (unsigned)edges[(size_t)e * 2 + 1], (unsigned)round) << 32) |
        (unsigned)e;
    unsigned mine = 1;
    if (!rm_flip_quad(edges, cd, e, V, [&](unsigned w) { mine &= (unsigned)(owner[w] == key); })) return;
    if (mine) state[e] = 2;
}

// the faces of a selected flip, (a, b, c) and (b, a, d), become (a, d, c) and (d, b, c); selected flips share no vertex,
// so no face is written twice
__global__ __launch_bounds__(DEC_BLOCK) void k_rm_flip_apply(const int* __restrict__ edges, const int* __restrict__ cd,
                                                             const int* __restrict__ ff,
                                                             const unsigned char* __restrict__ state, int V, int T,
                                                             int E, int* __restrict__ tri) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E || state[e] != 2) return;
    const int a = edges[(size_t)e * 2], b = edges[(size_t)e * 2 + 1], c = cd[(size_t)e * 2], d = cd[(size_t)e * 2 + 1];
    const int f0 = ff[(size_t)e * 2], f1 = ff[(size_t)e * 2 + 1];
    if ((unsigned)max(max(a, b), max(c, d)) >= (unsigned)V || (unsigned)max(f0, f1) >= (unsigned)T || min(f0, f1) < 0) return;
    tri[(size_t)f0 * 3] = a;
    tri[(size_t)f0 * 3 + 1] = d;
    tri[(size_t)f0 * 3 + 2] = c;
    tri[(size_t)f1 * 3] = d;
    tri[(size_t)f1 * 3 + 1] = b;
    tri[(size_t)f1 * 3 + 2] = c;
}

// ---------------------------------------------------------------------------------------------------------------
// move
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEC_BLOCK) void k_rm_relax(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                        const unsigned char* __restrict__ locked, DecTopo t,
                                                        float* __restrict__ q_out,
                                                        unsigned char* __restrict__ movable) {
    const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (v >= t.V) return;
    const DecP p = dec_pos(v_pos, (unsigned)v);
    DecP q = p;
    unsigned char mv = 0;
    const int nb = dec_clamp(t.nbr_ptr[v], 0, t.NN), ne = dec_clamp(t.nbr_ptr[v + 1], 0, t.NN);
    const int fb = dec_clamp(t.vf_ptr[v], 0, 3 * t.T), fe = dec_clamp(t.vf_ptr[v + 1], 0, 3 * t.T);
    if (!locked[v] && ne > nb && fe > fb) {
        DecP g{0.0, 0.0, 0.0}, n{0.0, 0.0, 0.0};
        int cnt = 0;
        for (int i = nb; i < ne; ++i) {
            const unsigned w = (unsigned)t.nbr_col[i];
            if (w >= (unsigned)t.V) continue;
            const DecP pw = dec_pos(v_pos, w);
            g.x += pw.x, g.y += pw.y, g.z += pw.z;
            ++cnt;
        }
        for (int i = fb; i < fe; ++i) {  // ascending face order
            const unsigned f = (unsigned)t.vf_col[i] / 3u;
            if (f >= (unsigned)t.T) continue;
            const unsigned i0 = (unsigned)tri[(size_t)f * 3], i1 = (unsigned)tri[(size_t)f * 3 + 1],
                           i2 = (unsigned)tri[(size_t)f * 3 + 2];
            if (max(i0, max(i1, i2)) >= (unsigned)t.V) continue;
            const DecP p0 = dec_pos(v_pos, i0);
            const DecP c = dec_cross(dec_sub(dec_pos(v_pos, i1), p0), dec_sub(dec_pos(v_pos, i2), p0));
            n.x += c.x, n.y += c.y, n.z += c.z;
        }
        if (cnt > 0) {
            g.x /= (double)cnt, g.y /= (double)cnt, g.z /= (double)cnt;
            const double l = sqrt(dec_dot(n, n));
            if (l > 0.0) n.x /= l, n.y /= l, n.z /= l;
            else n = DecP{0.0, 0.0, 0.0};
            const DecP d = dec_sub(g, p);
            const double s = dec_dot(d, n);
            q = DecP{(p.x + d.x) - s * n.x, (p.y + d.y) - s * n.y, (p.z + d.z) - s * n.z};
            mv = 1;
        }
    }
    q_out[(size_t)v * 3] = (float)q.x;
    q_out[(size_t)v * 3 + 1] = (float)q.y;
    q_out[(size_t)v * 3 + 2] = (float)q.z;
    movable[v] = mv;
}

// a movable vertex goes to (b0 s0 + b1 s1) + b2 s2 of the face of the source mesh it was sent to, fp32
__global__ __launch_bounds__(DEC_BLOCK) void k_rm_place(const float* __restrict__ v_old, const int* __restrict__ face,
                                                        const float* __restrict__ bary,
                                                        const float* __restrict__ src_pos,
                                                        const int* __restrict__ src_tri,
                                                        const unsigned char* __restrict__ movable, int V, int V0, int T0,
                                                        float* __restrict__ v_new) {
    const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (v >= V) return;
    RmF3 p = rm_pos(v_old, (unsigned)v);
    const int f = face[v];
    if (movable[v] && (unsigned)f < (unsigned)T0) {
        const unsigned i0 = (unsigned)src_tri[(size_t)f * 3], i1 = (unsigned)src_tri[(size_t)f * 3 + 1],
                       i2 = (unsigned)src_tri[(size_t)f * 3 + 2];
        if (max(i0, max(i1, i2)) < (unsigned)V0) {
            const RmF3 s0 = rm_pos(src_pos, i0), s1 = rm_pos(src_pos, i1), s2 = rm_pos(src_pos, i2);
            const float b0 = bary[(size_t)v * 3], b1 = bary[(size_t)v * 3 + 1], b2 = bary[(size_t)v * 3 + 2];
            const RmF3 x{(b0 * s0.x + b1 * s1.x) + b2 * s2.x, (b0 * s0.y + b1 * s1.y) + b2 * s2.y,
                         (b0 * s0.z + b1 * s1.z) + b2 * s2.z};
            if (isfinite(x.x) && isfinite(x.y) && isfinite(x.z)) p = x;
        }
    }
    v_new[(size_t)v * 3] = p.x;
    v_new[(size_t)v * 3 + 1] = p.y;
    v_new[(size_t)v * 3 + 2] = p.z;
}

// One Jacobi step of the fold guard: positions are v_old where rev_in says so, else v_new; a face whose old normal is
// not zero and whose new normal has a non-positive dot product with it sets rev_out of its corners (rev_out holds a
// copy of rev_in on entry) and counts itself.  Such a face has a corner that rev_in does not hold yet.
__global__ __launch_bounds__(DEC_BLOCK) void k_rm_fold_flag(const float* __restrict__ v_old,
                                                            const float* __restrict__ v_new,
                                                            const int* __restrict__ tri,
                                                            const unsigned char* __restrict__ rev_in, int V, int T,
                                                            unsigned char* __restrict__ rev_out,
                                                            int* __restrict__ count) {
    const int f = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (f >= T) return;
    const unsigned i0 = (unsigned)tri[(size_t)f * 3], i1 = (unsigned)tri[(size_t)f * 3 + 1],
                   i2 = (unsigned)tri[(size_t)f * 3 + 2];
    if (max(i0, max(i1, i2)) >= (unsigned)V) return;
    const DecP o0 = dec_pos(v_old, i0), o1 = dec_pos(v_old, i1), o2 = dec_pos(v_old, i2);
    const DecP c0 = rev_in[i0] ? o0 : dec_pos(v_new, i0), c1 = rev_in[i1] ? o1 : dec_pos(v_new, i1),
               c2 = rev_in[i2] ? o2 : dec_pos(v_new, i2);
    const DecP n_old = dec_cross(dec_sub(o1, o0), dec_sub(o2, o0)), n_new = dec_cross(dec_sub(c1, c0), dec_sub(c2, c0));
    if (!(dec_dot(n_old, n_old) > 0.0)) return;
    if (dec_dot(n_old, n_new) > 0.0) return;
    rev_out[i0] = 1;
    rev_out[i1] = 1;
    rev_out[i2] = 1;
    atomicAdd(count, 1);
}

__global__ __launch_bounds__(DEC_BLOCK) void k_rm_revert(const float* __restrict__ v_old,
                                                         const unsigned char* __restrict__ rev, int V,
                                                         float* __restrict__ v_new) {
    const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (v >= V || !rev[v]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) v_new[(size_t)v * 3 + k] = v_old[(size_t)v * 3 + k];
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
static bool rm_len_ok(float x) { return x > 0.f && x < INFINITY; }

extern "C" int64_t tt_remesh_workspace_bytes(int32_t T, int32_t E) {
    if (T < 1 || T > TT_MESH_MAX_ITEMS || !dec_edges_ok(T, E)) return TT_ERR_BAD_ARG;
    return rm_layout(nullptr, E, T).bytes;
}

extern "C" int tt_remesh_split_count(const float* v_pos, const int32_t* edges, const int32_t* face_edge, int32_t V,
                                     int32_t T, int32_t E, float hi2, void* workspace, int32_t* out_totals,
                                     void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E) || !rm_len_ok(hi2)) return TT_ERR_BAD_ARG;
    if (!v_pos || !edges || !face_edge || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    const RmWs w = rm_layout(workspace, E, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rm_split_mark, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, s, v_pos, (const int*)edges, (int)V, (int)E,
                       hi2, w.mark);
    hipLaunchKernelGGL(k_rm_split_count, dim3((unsigned)w.c.nblk), dim3(DEC_BLOCK), 0, s, (const int*)face_edge, (int)T,
                       (int)E, w);
    tt_compact2_scan_blocks(w.c, (int*)out_totals, s);
    return tt_check_launch();
}

extern "C" int tt_remesh_split_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edges,
                                    const int32_t* face_edge, int32_t V, int32_t T, int32_t E, int32_t M, int32_t Tn,
                                    void* workspace, float* v_new, int32_t* marked, int32_t* t_out, void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E) || M < 1 || M > E || Tn < T || (long long)Tn > 4ll * T ||
        (long long)V + M > TT_MESH_MAX_ITEMS || Tn > TT_MESH_MAX_ITEMS)
        return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !edges || !face_edge || !workspace || !v_new || !marked || !t_out) return TT_ERR_BAD_ARG;
    const RmWs w = rm_layout(workspace, E, T).w;
    hipLaunchKernelGGL(k_rm_split_emit, dim3((unsigned)w.c.nblk), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, (const int*)edges, (const int*)face_edge, (int)V, (int)T, (int)E, (int)M,
                       (int)Tn, w, v_new, (int*)marked, (int*)t_out);
    return tt_check_launch();
}

extern "C" int tt_remesh_collapse_candidates(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edges,
                                             const int32_t* nbr_ptr, const int32_t* nbr_col, const int32_t* vf_ptr,
                                             const int32_t* vf_col, const uint8_t* locked, int32_t V, int32_t T,
                                             int32_t E, float hi2, float lo2, int32_t* cost_bits, float* xopt,
                                             void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E) || !rm_len_ok(hi2) || !rm_len_ok(lo2)) return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !edges || !nbr_ptr || !nbr_col || !vf_ptr || !vf_col || !locked || !cost_bits || !xopt)
        return TT_ERR_BAD_ARG;
    const DecTopo t = dec_topo(nbr_ptr, nbr_col, vf_ptr, vf_col, V, T, E);
    hipLaunchKernelGGL(k_rm_collapse_cand, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, (const int*)edges, (const unsigned char*)locked, t, (int)E, hi2, lo2,
                       (unsigned*)cost_bits, xopt);
    return tt_check_launch();
}

extern "C" int tt_remesh_flip_select(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edges,
                                     const int32_t* edge_fe, const int32_t* nbr_ptr, const int32_t* nbr_col,
                                     const uint8_t* locked, int32_t V, int32_t T, int32_t E, float hi2, int32_t round,
                                     uint8_t* state, int32_t* cd, int32_t* faces, int64_t* owner, void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E) || !rm_len_ok(hi2) || round < 0) return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !edges || !edge_fe || !nbr_ptr || !nbr_col || !locked || !state || !cd || !faces ||
        !owner)
        return TT_ERR_BAD_ARG;
    const DecTopo t = dec_topo(nbr_ptr, nbr_col, nullptr, nullptr, V, T, E);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(owner, 0xff, (size_t)V * 8, s) != hipSuccess) return TT_ERR_DEVICE;
    hipLaunchKernelGGL(k_rm_flip_cand, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, s, v_pos, (const int*)t_pos_idx,
                       (const int*)edges, (const int*)edge_fe, (const unsigned char*)locked, t, (int)E, hi2,
                       (unsigned char*)state, (int*)cd, (int*)faces);
    hipLaunchKernelGGL(k_rm_flip_mark, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, s, (const int*)edges, (const int*)cd,
                       (const unsigned char*)state, (int)V, (int)E, (int)round, (unsigned long long*)owner);
    hipLaunchKernelGGL(k_rm_flip_select, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, s, (const int*)edges, (const int*)cd,
                       (int)V, (int)E, (int)round, (const unsigned long long*)owner, (unsigned char*)state);
    return tt_check_launch();
}

extern "C" int tt_remesh_flip_apply(const int32_t* edges, const int32_t* cd, const int32_t* faces, const uint8_t* state,
                                    int32_t V, int32_t T, int32_t E, int32_t* t_pos_idx, void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E) || !edges || !cd || !faces || !state || !t_pos_idx)
        return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_rm_flip_apply, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, (const int*)edges,
                       (const int*)cd, (const int*)faces, (const unsigned char*)state, (int)V, (int)T, (int)E,
                       (int*)t_pos_idx);
    return tt_check_launch();
}

extern "C" int tt_remesh_relax(const float* v_pos, const int32_t* t_pos_idx, const int32_t* nbr_ptr,
                               const int32_t* nbr_col, const int32_t* vf_ptr, const int32_t* vf_col,
                               const uint8_t* locked, int32_t V, int32_t T, int32_t E, float* q, uint8_t* movable,
                               void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E)) return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !nbr_ptr || !nbr_col || !vf_ptr || !vf_col || !locked || !q || !movable)
        return TT_ERR_BAD_ARG;
    const DecTopo t = dec_topo(nbr_ptr, nbr_col, vf_ptr, vf_col, V, T, E);
    hipLaunchKernelGGL(k_rm_relax, dim3(tt_grid(V)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, (const unsigned char*)locked, t, q, (unsigned char*)movable);
    return tt_check_launch();
}

extern "C" int tt_remesh_place(const float* v_old, const int32_t* face, const float* bary, const float* src_pos,
                               const int32_t* src_tri, const uint8_t* movable, int32_t V, int32_t V0, int32_t T0,
                               float* v_new, void* stream) {
    if (V < 1 || V > TT_MESH_MAX_ITEMS || !dec_sizes_ok(V0, T0)) return TT_ERR_BAD_ARG;
    if (!v_old || !face || !bary || !src_pos || !src_tri || !movable || !v_new) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_rm_place, dim3(tt_grid(V)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_old, (const int*)face,
                       bary, src_pos, (const int*)src_tri, (const unsigned char*)movable, (int)V, (int)V0, (int)T0, v_new);
    return tt_check_launch();
}

extern "C" int tt_remesh_fold_flag(const float* v_old, const float* v_new, const int32_t* t_pos_idx,
                                   const uint8_t* rev_in, int32_t V, int32_t T, uint8_t* rev_out, int32_t* count,
                                   void* stream) {
    if (!dec_sizes_ok(V, T) || !v_old || !v_new || !t_pos_idx || !rev_in || !rev_out || !count) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(rev_out, rev_in, (size_t)V, hipMemcpyDeviceToDevice, s) != hipSuccess) return TT_ERR_DEVICE;
    if (hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) return TT_ERR_DEVICE;
    hipLaunchKernelGGL(k_rm_fold_flag, dim3(tt_grid(T)), dim3(DEC_BLOCK), 0, s, v_old, v_new, (const int*)t_pos_idx,
                       (const unsigned char*)rev_in, (int)V, (int)T, (unsigned char*)rev_out, (int*)count);
    return tt_check_launch();
}

extern "C" int tt_remesh_revert(const float* v_old, const uint8_t* rev, int32_t V, float* v_new, void* stream) {
    if (V < 1 || V > TT_MESH_MAX_ITEMS || !v_old || !rev || !v_new) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_rm_revert, dim3(tt_grid(V)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_old,
                       (const unsigned char*)rev, (int)V, v_new);
    return tt_check_launch();
}
