// tt_decimate.hip -- manifold-preserving mesh decimation: round-based parallel quadric edge collapse (the quadrics of
// Garland & Heckbert 1997; collapses with pairwise disjoint closed neighbourhoods run in the same round).  The contract
// (state, locking, cost and validity, threshold, independent set, budget, apply, output, determinism, non-guarantees)
// is written in include/tt_abi.h, "mesh decimation".  The topology of a round (one face-edge sort, the vertex ->
// neighbour and vertex -> face CSR tables), the threshold and the budget are torch on the host side
// (ops.mesh_decimate); everything else is here:
//   k_dec_quadrics     one thread per vertex: its quadric, a sum over its faces in ascending face order, fp64
//   k_dec_lock         one thread per unique edge: the endpoints of an edge that other than two face edges use
//   k_dec_edges        one thread per unique edge: optimal point, cost, the validity rules
//   k_dec_mark         one thread per unique edge: candidates, blocking, 64-bit atomicMin of the key into owner[]
//   k_dec_select       one thread per unique edge: selected iff it owns its whole closed neighbourhood
//   k_dec_collapse     one thread per kept edge: position, quadric, remap
//   k_dec_faces_count / k_compact2_blocks / k_dec_faces_emit   (tt_compact.h) the surviving faces in order, roots
//   k_dec_unmap        remap back to the identity
//   k_dec_vmark / k_compact2_flags / k_compact2_blocks / k_dec_emit   the referenced vertices, faces, vertex_map
// The star loops walk the CSR rows with scalars only (no per-thread arrays).  No float atomics; the one atomic is an
// integer min, so identical inputs give bit-identical outputs.
#include "tt_decimate.h"

struct DecWs {
    int* misc;             // [0..1] totals of the last compaction
    unsigned char* vmark;  // [V] vertex referenced by a live face
    TtCompact2 c;          // items: max(V, T); low counter: referenced vertices, high: surviving faces
};

struct DecLayout {
    DecWs w;
    long long bytes;
};

// the workspace sections (tt_decimate_workspace_bytes); base may be null for the size alone
static DecLayout dec_layout(void* base, long long V, long long T) {
    TtCarver c{(char*)base};
    DecLayout l;
    l.w.misc = c.take<int>(64);
    l.w.vmark = c.take<unsigned char>(V);
    l.w.c = tt_compact2_carve(c, V > T ? V : T, base ? l.w.misc : nullptr);
    l.bytes = c.bytes();
    return l;
}

// ---------------------------------------------------------------------------------------------------------------
// quadrics and locking
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_quadrics(const float* __restrict__ v_pos,
                                                            const int* __restrict__ tri, DecTopo t,
                                                            double* __restrict__ quadrics) {
    const int v = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (v >= t.V) return;
    double q[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) q[j] = 0.0;
    const int rb = dec_clamp(t.vf_ptr[v], 0, 3 * t.T), re = dec_clamp(t.vf_ptr[v + 1], 0, 3 * t.T);
    for (int i = rb; i < re; ++i) {
        const unsigned f = (unsigned)t.vf_col[i] / 3u;
        if (f >= (unsigned)t.T) continue;
        const unsigned i0 = (unsigned)tri[(size_t)f * 3], i1 = (unsigned)tri[(size_t)f * 3 + 1],
                       i2 = (unsigned)tri[(size_t)f * 3 + 2];
        if (max(i0, max(i1, i2)) >= (unsigned)t.V) continue;
        const DecP p0 = dec_pos(v_pos, i0);
        const DecP n = dec_cross(dec_sub(dec_pos(v_pos, i1), p0), dec_sub(dec_pos(v_pos, i2), p0));
        const double l = sqrt(dec_dot(n, n));
        if (!(l > 0.0)) continue;
        const DecP nh{n.x / l, n.y / l, n.z / l};
        const double area = 0.5 * l, d = -dec_dot(nh, p0);
        q[0] += area * nh.x * nh.x;
        q[1] += area * nh.x * nh.y;
        q[2] += area * nh.x * nh.z;
        q[3] += area * nh.y * nh.y;
        q[4] += area * nh.y * nh.z;
        q[5] += area * nh.z * nh.z;
        q[6] += area * d * nh.x;
        q[7] += area * d * nh.y;
        q[8] += area * d * nh.z;
        q[9] += area * d * d;
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) quadrics[(size_t)v * 10 + j] = q[j];
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_lock(const int* __restrict__ edges, const int* __restrict__ counts,
                                                        int V, int E, unsigned char* __restrict__ locked) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    const unsigned a = (unsigned)edges[(size_t)e * 2], b = (unsigned)edges[(size_t)e * 2 + 1];
    if (counts[e] == 2 && a != b) return;
    if (a < (unsigned)V) locked[a] = 1;
    if (b < (unsigned)V) locked[b] = 1;
}

// ---------------------------------------------------------------------------------------------------------------
// cost and validity
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dec_cost(const double* q, DecP x) {
    const double ax = q[0] * x.x + q[1] * x.y + q[2] * x.z, ay = q[1] * x.x + q[3] * x.y + q[4] * x.z,
                 az = q[2] * x.x + q[4] * x.y + q[5] * x.z;
    return (x.x * ax + x.y * ay + x.z * az) + 2.0 * (q[6] * x.x + q[7] * x.y + q[8] * x.z) + q[9];
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_edges(const float* __restrict__ v_pos,
                                                         const double* __restrict__ quadrics,
                                                         const int* __restrict__ tri, const int* __restrict__ edges,
                                                         const unsigned char* __restrict__ locked, DecTopo t, int E,
                                                         unsigned* __restrict__ cost_bits, float* __restrict__ xopt) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    cost_bits[e] = DEC_INVALID;
#pragma unroll
    for (int k = 0; k < 3; ++k) xopt[(size_t)e * 3 + k] = 0.f;
    const unsigned a = (unsigned)edges[(size_t)e * 2], b = (unsigned)edges[(size_t)e * 2 + 1];
    if (a >= (unsigned)t.V || b >= (unsigned)t.V || a == b) return;
    if (locked[a] | locked[b]) return;
    const int a0 = dec_clamp(t.nbr_ptr[a], 0, t.NN), a1 = dec_clamp(t.nbr_ptr[a + 1], 0, t.NN);
    const int b0 = dec_clamp(t.nbr_ptr[b], 0, t.NN), b1 = dec_clamp(t.nbr_ptr[b + 1], 0, t.NN);
    if ((a1 - a0) + (b1 - b0) - 4 < 3) return;
    // the link condition: a merge of the two ascending rows
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
    if (common != 2) return;
    if (thin != 0) return;
    double q[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) q[k] = quadrics[(size_t)a * 10 + k] + quadrics[(size_t)b * 10 + k];
    // x = -A^-1 b by cofactors
    const double c00 = q[3] * q[5] - q[4] * q[4], c01 = q[2] * q[4] - q[1] * q[5], c02 = q[1] * q[4] - q[2] * q[3];
    const double c11 = q[0] * q[5] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[4], c22 = q[0] * q[3] - q[1] * q[1];
    const double det = q[0] * c00 + q[1] * c01 + q[2] * c02, tr = (q[0] + q[3] + q[5]) / 3.0;
    DecP x;
    double cost;
    if (fabs(det) > 1e-9 * (tr * tr * tr)) {
        x.x = -(c00 * q[6] + c01 * q[7] + c02 * q[8]) / det;
        x.y = -(c01 * q[6] + c11 * q[7] + c12 * q[8]) / det;
        x.z = -(c02 * q[6] + c12 * q[7] + c22 * q[8]) / det;
        cost = dec_cost(q, x);
    } else {
        const DecP pa = dec_pos(v_pos, a), pb = dec_pos(v_pos, b);
        const DecP pm{0.5 * (pa.x + pb.x), 0.5 * (pa.y + pb.y), 0.5 * (pa.z + pb.z)};
        x = pa;
        cost = dec_cost(q, pa);
        const double cb = dec_cost(q, pb), cm = dec_cost(q, pm);
        if (cb < cost) {
            cost = cb;
            x = pb;
        }
        if (cm < cost) {
            cost = cm;
            x = pm;
        }
    }
    const float xf[3] = {(float)x.x, (float)x.y, (float)x.z};
    const DecP xr{(double)xf[0], (double)xf[1], (double)xf[2]};
    if (!dec_star_ok(v_pos, tri, t, a, b, xr)) return;
    if (!dec_star_ok(v_pos, tri, t, b, a, xr)) return;
    const float cf = (float)fmax(cost, 0.0);
    if (!(cf >= 0.f)) return;
    cost_bits[e] = __float_as_uint(cf);
#pragma unroll
    for (int k = 0; k < 3; ++k) xopt[(size_t)e * 3 + k] = xf[k];
}

// ---------------------------------------------------------------------------------------------------------------
// independent set
// ---------------------------------------------------------------------------------------------------------------
// state of an edge: 0 no candidate, 1 candidate, 2 selected, 3 blocked
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_mark(const int* __restrict__ edges,
                                                        const unsigned* __restrict__ cost_bits,
                                                        const long long* __restrict__ tau, DecTopo t, int E, int round,
                                                        int pass, unsigned char* __restrict__ state,
                                                        const unsigned char* __restrict__ taken,
                                                        unsigned long long* __restrict__ owner) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E) return;
    const unsigned a = (unsigned)edges[(size_t)e * 2], b = (unsigned)edges[(size_t)e * 2 + 1];
    if (max(a, b) >= (unsigned)t.V) {
        if (pass == 0) state[e] = 0;
        return;
    }
    unsigned st;
    if (pass == 0) {
        // valid and at most tau in ONE compare: an invalid edge holds the largest bit pattern
        const long long lim = min(tau[0], (long long)DEC_INVALID - 1);
        st = (unsigned)((long long)cost_bits[e] <= lim);
        state[e] = (unsigned char)st;
    } else {
        st = state[e];
    }
    if (st != 1u) return;
    if (pass > 0) {
        unsigned blocked = 0;
        dec_neighbourhood(t, a, b, [&](unsigned w) { blocked |= taken[w]; });
        if (blocked) {
            state[e] = 3;
            return;
        }
    }
    const unsigned long long key = ((unsigned long long)dec_hash(a, b, (unsigned)round) << 32) | (unsigned)e;
    dec_neighbourhood(t, a, b, [&](unsigned w) { atomicMin(owner + w, key); });
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_select(const int* __restrict__ edges, DecTopo t, int E, int round,
                                                          unsigned char* __restrict__ state,
                                                          unsigned char* __restrict__ taken,
                                                          const unsigned long long* __restrict__ owner) {
    const int e = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (e >= E || state[e] != 1) return;
    const unsigned a = (unsigned)edges[(size_t)e * 2], b = (unsigned)edges[(size_t)e * 2 + 1];
    if (a >= (unsigned)t.V || b >= (unsigned)t.V) return;
    const unsigned long long key = ((unsigned long long)dec_hash(a, b, (unsigned)round) << 32) | (unsigned)e;
    unsigned mine = 1;
    dec_neighbourhood(t, a, b, [&](unsigned w) { mine &= (unsigned)(owner[w] == key); });
    if (!mine) return;
    state[e] = 2;
    dec_neighbourhood(t, a, b, [&](unsigned w) { taken[w] = 1; });
}

// ---------------------------------------------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_collapse(const int* __restrict__ kept_edges,
                                                            const float* __restrict__ kept_x, int V, int K,
                                                            float* __restrict__ v_pos, double* __restrict__ quadrics,
                                                            int* __restrict__ remap) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (i >= K) return;
    const unsigned a = (unsigned)kept_edges[(size_t)i * 2], b = (unsigned)kept_edges[(size_t)i * 2 + 1];
    if (a >= (unsigned)V || b >= (unsigned)V || a == b) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) v_pos[(size_t)a * 3 + k] = kept_x[(size_t)i * 3 + k];
#pragma unroll
    for (int k = 0; k < 10; ++k) quadrics[(size_t)a * 10 + k] += quadrics[(size_t)b * 10 + k];
    remap[b] = (int)a;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_unmap(const int* __restrict__ kept_edges, int V, int K,
                                                         int* __restrict__ remap) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (i >= K) return;
    const unsigned b = (unsigned)kept_edges[(size_t)i * 2 + 1];
    if (b < (unsigned)V) remap[b] = (int)b;
}

// the remapped corners of face f (any f >= 0); 1 when f < T and the face survives (three distinct corners, all in
// range), else 0
__device__ __forceinline__ unsigned dec_face(const int* __restrict__ tri, const int* __restrict__ remap, int V, int T,
                                             int f, int r[3]) {
    unsigned m = 0;  // the largest index met; reads clamped into bounds
    const int fc = min(f, T - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned v = (unsigned)tri[(size_t)fc * 3 + k];
        r[k] = remap[min(v, (unsigned)(V - 1))];
        m = max(m, max(v, (unsigned)r[k]));
    }
    // integer arithmetic, no compare masks to combine: in = 1 iff m < V and f < T; d = 0 iff two
    // corners are equal; (d | -d) >> 31 = 1 iff d != 0
    const unsigned in = (unsigned)((((long long)m - (long long)V) & ((long long)f - (long long)T)) >> 63) & 1u;
    const unsigned d = min(min((unsigned)(r[0] ^ r[1]), (unsigned)(r[1] ^ r[2])), (unsigned)(r[2] ^ r[0]));
    return ((d | (0u - d)) >> 31) & in;
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_faces_count(const int* __restrict__ tri,
                                                               const int* __restrict__ remap, int V, int T, DecWs w) {
    const int f = blockIdx.x * DEC_BLOCK + threadIdx.x;
    int r[3];
    tt_compact2_first_level<1>(w.c, 0u, dec_face(tri, remap, V, T, f, r));
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_faces_emit(const int* __restrict__ tri,
                                                              const int* __restrict__ remap, int V, int T, DecWs w,
                                                              int* __restrict__ tri_out, int* __restrict__ root) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    const int nt = min(w.misc[1], T);  // bound of every write: the total the scan produced, and the buffer
    if (i < T) {
        int r[3];
        if (dec_face(tri, remap, V, T, i, r)) {
            const int o = tt_compact2_hi(w.c, i);
            if ((unsigned)o < (unsigned)nt) {
#pragma unroll
                for (int k = 0; k < 3; ++k) tri_out[(size_t)o * 3 + k] = r[k];
            }
        }
    }
    if (i < V) {
        const unsigned r = (unsigned)root[i];
        if (r < (unsigned)V) root[i] = remap[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// output
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEC_BLOCK) void k_dec_vmark(const int* __restrict__ tri, int V, int T, DecWs w) {
    const int f = blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (f >= T) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned v = (unsigned)tri[(size_t)f * 3 + k];
        if (v < (unsigned)V) w.vmark[v] = 1;
    }
}

__global__ __launch_bounds__(DEC_BLOCK) void k_dec_emit(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                        const int* __restrict__ root, int V, int T, DecWs w,
                                                        float* __restrict__ v_out, int* __restrict__ t_out,
                                                        int* __restrict__ vertex_map) {
    const int i = blockIdx.x * DEC_BLOCK + threadIdx.x;
    const int nv = w.misc[0];  // bound of every vertex write: the total the scan produced
    if (i < V && w.vmark[i]) {
        const int o = tt_compact2_lo(w.c, i);
        if ((unsigned)o < (unsigned)nv) {
#pragma unroll
            for (int k = 0; k < 3; ++k) v_out[(size_t)o * 3 + k] = v_pos[(size_t)i * 3 + k];
        }
    }
    if (i < T) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned v = min((unsigned)tri[(size_t)i * 3 + k], (unsigned)(V - 1));
            t_out[(size_t)i * 3 + k] = tt_compact2_lo(w.c, (int)v);
        }
    }
    if (i < V) {
        const unsigned r = (unsigned)root[i];
        int m = -1;
        if (r < (unsigned)V) {
            if (w.vmark[r]) m = tt_compact2_lo(w.c, (int)r);
        }
        vertex_map[i] = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t tt_decimate_workspace_bytes(int32_t V, int32_t T) {
    if (!dec_sizes_ok(V, T)) return TT_ERR_BAD_ARG;
    return dec_layout(nullptr, V, T).bytes;
}

extern "C" int tt_decimate_quadrics(const float* v_pos, const int32_t* t_pos_idx, const int32_t* vf_ptr,
                                    const int32_t* vf_col, int32_t V, int32_t T, double* quadrics, void* stream) {
    if (!dec_sizes_ok(V, T) || !v_pos || !t_pos_idx || !vf_ptr || !vf_col || !quadrics) return TT_ERR_BAD_ARG;
    const DecTopo t = dec_topo(nullptr, nullptr, vf_ptr, vf_col, V, T, 0);
    hipLaunchKernelGGL(k_dec_quadrics, dim3(tt_grid(V)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, t, quadrics);
    return tt_check_launch();
}

extern "C" int tt_decimate_lock(const int32_t* edges, const int32_t* counts, int32_t V, int32_t E, uint8_t* locked,
                                void* stream) {
    if (V < 1 || V > TT_MESH_MAX_ITEMS || E < 1 || E > 3ll * TT_MESH_MAX_ITEMS || !edges || !counts || !locked)
        return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(locked, 0, (size_t)V, s) != hipSuccess) return TT_ERR_DEVICE;
    hipLaunchKernelGGL(k_dec_lock, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, s, (const int*)edges, (const int*)counts,
                       (int)V, (int)E, (unsigned char*)locked);
    return tt_check_launch();
}

extern "C" int tt_decimate_edges(const float* v_pos, const double* quadrics, const int32_t* t_pos_idx,
                                 const int32_t* edges, const int32_t* nbr_ptr, const int32_t* nbr_col,
                                 const int32_t* vf_ptr, const int32_t* vf_col, const uint8_t* locked, int32_t V,
                                 int32_t T, int32_t E, int32_t* cost_bits, float* xopt, void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E)) return TT_ERR_BAD_ARG;
    if (!v_pos || !quadrics || !t_pos_idx || !edges || !nbr_ptr || !nbr_col || !vf_ptr || !vf_col || !locked ||
        !cost_bits || !xopt)
        return TT_ERR_BAD_ARG;
    const DecTopo t = dec_topo(nbr_ptr, nbr_col, vf_ptr, vf_col, V, T, E);
    hipLaunchKernelGGL(k_dec_edges, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_pos, quadrics,
                       (const int*)t_pos_idx, (const int*)edges, (const unsigned char*)locked, t, (int)E,
                       (unsigned*)cost_bits, xopt);
    return tt_check_launch();
}

extern "C" int tt_decimate_mark(const int32_t* edges, const int32_t* nbr_ptr, const int32_t* nbr_col,
                                const int32_t* cost_bits, const int64_t* tau, int32_t V, int32_t T, int32_t E,
                                int32_t round, int32_t pass, uint8_t* state, const uint8_t* taken, int64_t* owner,
                                void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E) || round < 0 || pass < 0) return TT_ERR_BAD_ARG;
    if (!edges || !nbr_ptr || !nbr_col || !cost_bits || !tau || !state || !taken || !owner) return TT_ERR_BAD_ARG;
    const DecTopo t = dec_topo(nbr_ptr, nbr_col, nullptr, nullptr, V, T, E);
    hipLaunchKernelGGL(k_dec_mark, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, (const int*)edges,
                       (const unsigned*)cost_bits, (const long long*)tau, t, (int)E, (int)round, (int)pass,
                       (unsigned char*)state, (const unsigned char*)taken, (unsigned long long*)owner);
    return tt_check_launch();
}

extern "C" int tt_decimate_select(const int32_t* edges, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V,
                                  int32_t T, int32_t E, int32_t round, uint8_t* state, uint8_t* taken,
                                  const int64_t* owner, void* stream) {
    if (!dec_sizes_ok(V, T) || !dec_edges_ok(T, E) || round < 0) return TT_ERR_BAD_ARG;
    if (!edges || !nbr_ptr || !nbr_col || !state || !taken || !owner) return TT_ERR_BAD_ARG;
    const DecTopo t = dec_topo(nbr_ptr, nbr_col, nullptr, nullptr, V, T, E);
    hipLaunchKernelGGL(k_dec_select, dim3(tt_grid(E)), dim3(DEC_BLOCK), 0, (hipStream_t)stream, (const int*)edges, t,
                       (int)E, (int)round, (unsigned char*)state, (unsigned char*)taken,
                       (const unsigned long long*)owner);
    return tt_check_launch();
}

extern "C" int tt_decimate_apply(const int32_t* kept_edges, const float* kept_xopt, const int32_t* t_pos_idx,
                                 int32_t V, int32_t T, int32_t K, void* workspace, float* v_pos, double* quadrics,
                                 int32_t* remap, int32_t* root, int32_t* t_out, int32_t* out_totals, void* stream) {
    if (!dec_sizes_ok(V, T) || K < 1 || K > T) return TT_ERR_BAD_ARG;
    if (!kept_edges || !kept_xopt || !t_pos_idx || !workspace || !v_pos || !quadrics || !remap || !root || !t_out ||
        !out_totals)
        return TT_ERR_BAD_ARG;
    const DecWs w = dec_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dec_collapse, dim3(tt_grid(K)), dim3(DEC_BLOCK), 0, s, (const int*)kept_edges, kept_xopt,
                       (int)V, (int)K, v_pos, quadrics, (int*)remap);
    hipLaunchKernelGGL(k_dec_faces_count, dim3((unsigned)w.c.nblk), dim3(DEC_BLOCK), 0, s, (const int*)t_pos_idx,
                       (const int*)remap, (int)V, (int)T, w);
    tt_compact2_scan_blocks(w.c, (int*)out_totals, s);
    hipLaunchKernelGGL(k_dec_faces_emit, dim3((unsigned)w.c.nblk), dim3(DEC_BLOCK), 0, s, (const int*)t_pos_idx,
                       (const int*)remap, (int)V, (int)T, w, (int*)t_out, (int*)root);
    hipLaunchKernelGGL(k_dec_unmap, dim3(tt_grid(K)), dim3(DEC_BLOCK), 0, s, (const int*)kept_edges, (int)V, (int)K,
                       (int*)remap);
    return tt_check_launch();
}

extern "C" int tt_decimate_emit_count(const int32_t* t_pos_idx, int32_t V, int32_t T, void* workspace,
                                      int32_t* out_totals, void* stream) {
    if (!dec_sizes_ok(V, T) || !t_pos_idx || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    const DecWs w = dec_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w.vmark, 0, (size_t)V, s) != hipSuccess) return TT_ERR_DEVICE;
    hipLaunchKernelGGL(k_dec_vmark, dim3(tt_grid(T)), dim3(DEC_BLOCK), 0, s, (const int*)t_pos_idx, (int)V, (int)T, w);
    tt_compact2_scan_flags(w.vmark, V, w.vmark, 0, w.c, (int*)out_totals, s);
    return tt_check_launch();
}

extern "C" int tt_decimate_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* root, int32_t V,
                                int32_t T, void* workspace, float* v_out, int32_t* t_out, int32_t* vertex_map,
                                void* stream) {
    if (!dec_sizes_ok(V, T) || !v_pos || !t_pos_idx || !root || !workspace || !v_out || !t_out || !vertex_map)
        return TT_ERR_BAD_ARG;
    const DecWs w = dec_layout(workspace, V, T).w;
    hipLaunchKernelGGL(k_dec_emit, dim3((unsigned)w.c.nblk), dim3(DEC_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, (const int*)root, (int)V, (int)T, w, v_out, (int*)t_out,
                       (int*)vertex_map);
    return tt_check_launch();
}
