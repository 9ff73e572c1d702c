// tt_simplify.hip -- mesh simplification by vertex clustering with quadric-error placement (Lindstrom 2000, the
// quadrics of Garland & Heckbert 1997).  The contract (box, cells, clusters, quadrics, placement, face rule, output
// order, determinism, non-guarantees) is written in include/tt_abi.h, "mesh simplification".  The three sorts (vertex
// keys, pair keys, face keys) are stable torch sorts on the host side (ops.mesh_simplify); everything else is here:
//   k_simp_keys     cell key of every vertex
//   k_simp_starts   run starts of the sorted keys            -> tt_exclusive_scan -> ranks
//   k_simp_ranks    rank of every vertex, cluster keys, member segment pointers
//   k_simp_pairs    (rank << 32 | 3f + k) per face corner that contributes, pairs per cluster (integer atomics)
//                   -> tt_exclusive_scan -> pair segment pointers
//   k_simp_solve    one wave per cluster: quadric and member mean (lane-strided partial sums, a fixed shuffle tree),
//                   lane 0 solves and clamps
//   k_simp_faces    63-bit key of every face's rotated rank triple
//   k_simp_keep     first face of every run of equal sorted keys
//   k_simp_mark     clusters a kept face references
//   k_compact2_flags / k_compact2_blocks   (tt_compact.h) offsets of the marked clusters and kept faces, (V', T')
//   k_simp_emit     vertices, faces, vertex_map
// No float atomics; identical inputs give bit-identical outputs.
#include "tt_compact.h"
#include "tt_trigrid.h"

#define SIMP_BLOCK TT_ITEM_BLOCK
#define SIMP_WAVES (SIMP_BLOCK / 64)
#define SIMP_SENTINEL 0x7fffffffffffffffll

struct SimpWs {
    int *excl, *xs, *ckey, *mptr, *pptr, *misc;
    unsigned char *fkeep, *cmark;
    TtCompact2 c;  // items: max(V, T); low counter: marked clusters, high: kept faces; totals in misc[2..3]
};

struct SimpLayout {
    SimpWs w;
    long long bytes;  // size of the workspace
};

// the workspace sections (tt_simplify_workspace_bytes); base may be null for the size alone
static SimpLayout simp_layout(void* base, long long V, long long T) {
    TtCarver c{(char*)base};
    SimpLayout l;
    l.w.excl = c.take<int>(V);                      // [V] run starts of the sorted keys, scanned in place
    l.w.xs = c.take<int>(tt_xscan_blocks(V) + 1);   // block sums of both tt_exclusive_scan calls (V, then C <= V items)
    l.w.ckey = c.take<int>(V);                      // [C] cell key of a cluster
    l.w.mptr = c.take<int>(V + 1);                  // [C+1] member segments in the sorted vertex order
    l.w.pptr = c.take<int>(V + 1);                  // [C+1] pairs per cluster, scanned in place: pair segments
    l.w.misc = c.take<int>(64);                     // [0] C, [2..3] (V', T')
    l.w.fkeep = c.take<unsigned char>(T);           // [T] face kept
    l.w.cmark = c.take<unsigned char>(V);           // [C] cluster referenced by a kept face
    l.w.c = tt_compact2_carve(c, V > T ? V : T, base ? l.w.misc + 2 : nullptr);
    l.bytes = c.bytes();
    return l;
}

struct SimpBox {
    float lo[3], h, inv_h;
    int G;
};

// ---------------------------------------------------------------------------------------------------------------
// cells and clusters
// ---------------------------------------------------------------------------------------------------------------
// a vertex's cell is tri_cell (tt_trigrid.h); nothing here may contract into an FMA (tt_abi.h)
__device__ __forceinline__ void simp_centre(int key, const SimpBox& b, float ctr[3]) {
    const int c[3] = {key / (b.G * b.G), (key / b.G) % b.G, key % b.G};
#pragma unroll
    for (int a = 0; a < 3; ++a) ctr[a] = __fadd_rn(b.lo[a], __fmul_rn((float)c[a] + 0.5f, b.h));
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_keys(const float* __restrict__ v_pos, int V, SimpBox b,
                                                          long long* __restrict__ keys) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= V) return;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = tri_cell(v_pos[(size_t)i * 3 + a], b.lo[a], b.inv_h, b.G);
    keys[i] = (long long)tri_key(c, b.G);
}

__device__ __forceinline__ int simp_start(const long long* __restrict__ skeys, int i) {
    return (i == 0 || skeys[i] != skeys[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_starts(const long long* __restrict__ skeys, int V, SimpWs w) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= V) return;
    w.excl[i] = simp_start(skeys, i);
    w.pptr[i] = 0;
    if (i == 0) w.pptr[V] = 0;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_ranks(const long long* __restrict__ skeys,
                                                           const long long* __restrict__ perm, int V, int G, SimpWs w,
                                                           int* __restrict__ rank, int* __restrict__ out_totals) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= V) return;
    const int s = simp_start(skeys, i);
    const int r = min(max(w.excl[i] + s - 1, 0), V - 1);  // the scan's value is in [0, V) already
    const long long p = perm[i];
    if ((unsigned long long)p < (unsigned long long)V) rank[p] = r;
    if (s) {
        const long long cells = (long long)G * G * G;
        w.ckey[r] = (int)min(max(skeys[i], 0ll), cells - 1);
        w.mptr[r] = i;
    }
    if (i == V - 1) w.mptr[r + 1] = V;
    if (i == 0) out_totals[0] = w.misc[0];
}

// ---------------------------------------------------------------------------------------------------------------
// pairs
// ---------------------------------------------------------------------------------------------------------------
// the ranks of a face's corners; 0 when an index or a rank is out of range (such a face takes part in nothing), else 1.
// Every read is clamped into bounds and the verdict is integer arithmetic on single compares: no select here depends
// on a scalar-ALU combination of compare masks (tools/mask_hazard_lint.py).
__device__ __forceinline__ unsigned simp_face_ranks(const int* __restrict__ tri, const int* __restrict__ rank, int V,
                                                    int C, int f, int r[3]) {
    unsigned bad = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned v = (unsigned)tri[(size_t)f * 3 + k];
        bad |= (unsigned)(v >= (unsigned)V);
        r[k] = rank[min(v, (unsigned)(V - 1))];
        bad |= (unsigned)((unsigned)r[k] >= (unsigned)C);
    }
    return bad ^ 1u;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_pairs(const int* __restrict__ tri, const int* __restrict__ rank,
                                                           int V, int T, int C, SimpWs w,
                                                           long long* __restrict__ pkeys) {
    const int f = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (f >= T) return;
    int r[3];
    const unsigned ok = simp_face_ranks(tri, rank, V, C, f, r);
    // corner k contributes iff its cluster differs from the clusters of the corners before it
    const unsigned use[3] = {ok, ok & (unsigned)(r[1] != r[0]), ok & (unsigned)(r[2] != r[0]) & (unsigned)(r[2] != r[1])};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pkeys[(size_t)f * 3 + k] = use[k] ? (((long long)r[k] << 32) | (long long)(3 * f + k)) : SIMP_SENTINEL;
        if (use[k]) atomicAdd(w.pptr + r[k], 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// quadrics and placement
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_solve(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                           const long long* __restrict__ spkeys,
                                                           const long long* __restrict__ perm, int V, int T, int C,
                                                           SimpBox box, double lam, SimpWs w,
                                                           float* __restrict__ cpos) {
    const int c = blockIdx.x * SIMP_WAVES + (threadIdx.x >> 6);  // one wave per cluster
    const int lane = threadIdx.x & 63;
    if (c >= C) return;
    float ctr[3];
    simp_centre(w.ckey[c], box, ctr);
    // quadric: A (xx, xy, xz, yy, yz, zz), b, w
    float q[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) q[j] = 0.f;
    const int pb = max(w.pptr[c], 0), pe = min(w.pptr[c + 1], 3 * T);
    for (int i = pb + lane; i < pe; i += 64) {
        const unsigned f = (unsigned)(spkeys[i] & 0xffffffffll) / 3u;
        if (f >= (unsigned)T) continue;
        float p[3][3];
        unsigned bad = 0;  // reads clamped into bounds, the verdict integer arithmetic (see simp_face_ranks)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned v = (unsigned)tri[(size_t)f * 3 + k];
            bad |= (unsigned)(v >= (unsigned)V);
            const unsigned vs = min(v, (unsigned)(V - 1));
#pragma unroll
            for (int a = 0; a < 3; ++a) p[k][a] = v_pos[(size_t)vs * 3 + a];
        }
        const float e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const float e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float l = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        bad |= (unsigned)!(l > 0.f);
        if (bad) continue;
        const float nh[3] = {n[0] / l, n[1] / l, n[2] / l};
        const float area = 0.5f * l;
        const float d = -(nh[0] * (p[0][0] - ctr[0]) + nh[1] * (p[0][1] - ctr[1]) + nh[2] * (p[0][2] - ctr[2]));
        q[0] += area * nh[0] * nh[0];
        q[1] += area * nh[0] * nh[1];
        q[2] += area * nh[0] * nh[2];
        q[3] += area * nh[1] * nh[1];
        q[4] += area * nh[1] * nh[2];
        q[5] += area * nh[2] * nh[2];
        q[6] += area * d * nh[0];
        q[7] += area * d * nh[1];
        q[8] += area * d * nh[2];
        q[9] += area;
    }
    // member mean relative to the centre
    float m[3] = {0.f, 0.f, 0.f};
    const int mb = max(w.mptr[c], 0), me = min(w.mptr[c + 1], V);
    for (int i = mb + lane; i < me; i += 64) {
        const long long v = perm[i];
        if ((unsigned long long)v >= (unsigned long long)V) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] += v_pos[(size_t)v * 3 + a] - ctr[a];
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) q[j] = tt_wave_sum(q[j]);
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = tt_wave_sum(m[a]);
    if (lane != 0) return;
    const int cnt = me - mb;
    double x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = cnt > 0 ? (double)m[a] / (double)cnt : 0.0;
    if (q[9] > 0.f) {
        // (A + lam w I) x = lam w m - b by Cholesky, in double from the fp32 sums; SPD since w > 0
        const double lw = lam * (double)q[9];
        const double a00 = q[0] + lw, a10 = q[1], a20 = q[2], a11 = q[3] + lw, a21 = q[4], a22 = q[5] + lw;
        const double r0 = lw * x[0] - q[6], r1 = lw * x[1] - q[7], r2 = lw * x[2] - q[8];
        const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
        const double l11 = sqrt(a11 - l10 * l10), l21 = (a21 - l20 * l10) / l11;
        const double l22 = sqrt(a22 - l20 * l20 - l21 * l21);
        const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = (r2 - l20 * y0 - l21 * y1) / l22;
        const double s2 = y2 / l22, s1 = (y1 - l21 * s2) / l11, s0 = (y0 - l10 * s1 - l20 * s2) / l00;
        if (s0 == s0 && s1 == s1 && s2 == s2) {  // lam = 0 on a rank-deficient quadric: the member mean stays
            x[0] = s0;
            x[1] = s1;
            x[2] = s2;
        }
    }
    const double half = 0.5 * (double)box.h;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        cpos[(size_t)c * 3 + a] = __fadd_rn(ctr[a], (float)fmin(fmax(x[a], -half), half));
}

// ---------------------------------------------------------------------------------------------------------------
// faces
// ---------------------------------------------------------------------------------------------------------------
// a face's rank triple rotated so that the smallest rank comes first (orientation kept); 0 when two corners share a
// cluster (or the face is out of range), else 1
__device__ __forceinline__ unsigned simp_rotated(const int* __restrict__ tri, const int* __restrict__ rank, int V, int C,
                                             int f, int r[3]) {
    int q[3];
    unsigned ok = simp_face_ranks(tri, rank, V, C, f, q);
    ok &= (unsigned)(q[0] != q[1]) & (unsigned)(q[1] != q[2]) & (unsigned)(q[2] != q[0]);
    // position of the smallest rank: 0, 1 or 2 (ties only on faces that are dropped anyway)
    const int m01 = min(q[0], q[1]), mn = min(m01, q[2]);
    const int s = (int)(q[0] != mn) * (1 + (int)(q[1] != mn));
    const int t[5] = {q[0], q[1], q[2], q[0], q[1]};
    r[0] = mn;
    r[1] = s == 0 ? t[1] : (s == 1 ? t[2] : t[3]);
    r[2] = s == 0 ? t[2] : (s == 1 ? t[3] : t[4]);
    return ok;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_faces(const int* __restrict__ tri, const int* __restrict__ rank,
                                                           int V, int T, int C, long long* __restrict__ fkeys) {
    const int f = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (f >= T) return;
    int r[3];
    fkeys[f] = simp_rotated(tri, rank, V, C, f, r) ? (((long long)r[0] << 42) | ((long long)r[1] << 21) | (long long)r[2])
                                                  : SIMP_SENTINEL;
}

// sorted position i holds face fperm[i] (stable sort: ascending face index inside a run of equal keys)
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_keep(const long long* __restrict__ sfkeys,
                                                          const long long* __restrict__ fperm, int T, int C, SimpWs w) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i < C) w.cmark[i] = 0;
    if (i >= T) return;
    const long long k = sfkeys[i];
    const bool keep = k != SIMP_SENTINEL && (i == 0 || k != sfkeys[i - 1]);
    const long long f = fperm[i];
    if ((unsigned long long)f < (unsigned long long)T) w.fkeep[f] = keep ? 1 : 0;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_mark(const int* __restrict__ tri, const int* __restrict__ rank,
                                                          int V, int T, int C, SimpWs w) {
    const int f = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (f >= T || !w.fkeep[f]) return;
    int r[3];
    if (!simp_face_ranks(tri, rank, V, C, f, r)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) w.cmark[r[k]] = 1;  // in range: simp_face_ranks checked it
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_emit(const float* __restrict__ cpos, const int* __restrict__ tri,
                                                          const int* __restrict__ rank, int V, int T, int C, SimpWs w,
                                                          float* __restrict__ v_out, int* __restrict__ t_out,
                                                          int* __restrict__ vertex_map) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    const int nv = w.misc[2], nt = w.misc[3];  // bound of every write: the totals the scan produced
    if (i < C && w.cmark[i]) {
        const int o = tt_compact2_lo(w.c, i);
        if (o < nv) {
#pragma unroll
            for (int a = 0; a < 3; ++a) v_out[(size_t)o * 3 + a] = cpos[(size_t)i * 3 + a];
        }
    }
    if (i < T && w.fkeep[i]) {
        const int o = tt_compact2_hi(w.c, i);
        int r[3];
        if (o < nt && simp_rotated(tri, rank, V, C, i, r)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) t_out[(size_t)o * 3 + k] = tt_compact2_lo(w.c, r[k]);
        }
    }
    if (i < V) {
        const int r = rank[i];
        vertex_map[i] = ((unsigned)r < (unsigned)C && w.cmark[r]) ? tt_compact2_lo(w.c, r) : -1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
static bool simp_grid_ok(int32_t G) { return G >= TT_SIMPLIFY_MIN_GRID && G <= TT_SIMPLIFY_MAX_GRID; }
// C clusters of V vertices; more than TT_SIMPLIFY_MAX_CLUSTERS do not fit the face key
static int simp_clusters_status(int32_t V, int32_t C) {
    if (C < 1 || C > V) return TT_ERR_BAD_ARG;
    return C > TT_SIMPLIFY_MAX_CLUSTERS ? TT_ERR_UNSUPPORTED : TT_OK;
}

extern "C" int64_t tt_simplify_workspace_bytes(int32_t V, int32_t T) {
    if (!tri_mesh_ok(V, T)) return TT_ERR_BAD_ARG;
    return simp_layout(nullptr, V, T).bytes;
}

extern "C" int tt_simplify_keys(const float* v_pos, int32_t V, int32_t grid, float lo_x, float lo_y, float lo_z,
                                float inv_h, int64_t* keys, void* stream) {
    if (!tri_count_ok(V) || !simp_grid_ok(grid) || !v_pos || !keys) return TT_ERR_BAD_ARG;
    if (!tri_finite(lo_x) || !tri_finite(lo_y) || !tri_finite(lo_z) || !tri_finite(inv_h) || !(inv_h > 0.f))
        return TT_ERR_BAD_ARG;
    const SimpBox b{{lo_x, lo_y, lo_z}, 0.f, inv_h, (int)grid};
    hipLaunchKernelGGL(k_simp_keys, dim3(tt_grid(V)), dim3(SIMP_BLOCK), 0, (hipStream_t)stream, v_pos, (int)V, b,
                       (long long*)keys);
    return tt_check_launch();
}

extern "C" int tt_simplify_ranks(const int64_t* sorted_keys, const int64_t* perm, int32_t V, int32_t T, int32_t grid,
                                 void* workspace, int32_t* rank, int32_t* out_totals, void* stream) {
    if (!tri_mesh_ok(V, T) || !simp_grid_ok(grid)) return TT_ERR_BAD_ARG;
    if (!sorted_keys || !perm || !workspace || !rank || !out_totals) return TT_ERR_BAD_ARG;
    const SimpWs w = simp_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_simp_starts, dim3(tt_grid(V)), dim3(SIMP_BLOCK), 0, s, (const long long*)sorted_keys,
                       (int)V, w);
    tt_exclusive_scan<int>(w.excl, V, w.excl, w.xs, w.misc, s);
    hipLaunchKernelGGL(k_simp_ranks, dim3(tt_grid(V)), dim3(SIMP_BLOCK), 0, s, (const long long*)sorted_keys,
                       (const long long*)perm, (int)V, (int)grid, w, (int*)rank, (int*)out_totals);
    return tt_check_launch();
}

extern "C" int tt_simplify_pairs(const int32_t* t_pos_idx, const int32_t* rank, int32_t V, int32_t T, int32_t C,
                                 void* workspace, int64_t* pair_keys, void* stream) {
    if (!tri_mesh_ok(V, T) || !t_pos_idx || !rank || !workspace || !pair_keys) return TT_ERR_BAD_ARG;
    if (const int st = simp_clusters_status(V, C)) return st;
    const SimpWs w = simp_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_simp_pairs, dim3(tt_grid(T)), dim3(SIMP_BLOCK), 0, s, (const int*)t_pos_idx,
                       (const int*)rank, (int)V, (int)T, (int)C, w, (long long*)pair_keys);
    tt_exclusive_scan<int>(w.pptr, C, w.pptr, w.xs, w.pptr + C, s);
    return tt_check_launch();
}

extern "C" int tt_simplify_solve(const float* v_pos, const int32_t* t_pos_idx, const int64_t* sorted_pair_keys,
                                 const int64_t* perm, int32_t V, int32_t T, int32_t C, int32_t grid, float lo_x,
                                 float lo_y, float lo_z, float h, double lam, void* workspace, float* cluster_pos,
                                 void* stream) {
    if (!tri_mesh_ok(V, T) || !simp_grid_ok(grid)) return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !sorted_pair_keys || !perm || !workspace || !cluster_pos) return TT_ERR_BAD_ARG;
    if (!tri_finite(lo_x) || !tri_finite(lo_y) || !tri_finite(lo_z) || !tri_finite(h) || !(h > 0.f))
        return TT_ERR_BAD_ARG;
    if (!tri_finite(lam) || !(lam >= 0.0)) return TT_ERR_BAD_ARG;
    if (const int st = simp_clusters_status(V, C)) return st;
    const SimpWs w = simp_layout(workspace, V, T).w;
    const SimpBox b{{lo_x, lo_y, lo_z}, h, 0.f, (int)grid};
    hipLaunchKernelGGL(k_simp_solve, dim3((unsigned)((C + SIMP_WAVES - 1) / SIMP_WAVES)), dim3(SIMP_BLOCK), 0,
                       (hipStream_t)stream, v_pos, (const int*)t_pos_idx, (const long long*)sorted_pair_keys,
                       (const long long*)perm, (int)V, (int)T, (int)C, b, lam, w, cluster_pos);
    return tt_check_launch();
}

extern "C" int tt_simplify_faces(const int32_t* t_pos_idx, const int32_t* rank, int32_t V, int32_t T, int32_t C,
                                 int64_t* face_keys, void* stream) {
    if (!tri_mesh_ok(V, T) || !t_pos_idx || !rank || !face_keys) return TT_ERR_BAD_ARG;
    if (const int st = simp_clusters_status(V, C)) return st;
    hipLaunchKernelGGL(k_simp_faces, dim3(tt_grid(T)), dim3(SIMP_BLOCK), 0, (hipStream_t)stream,
                       (const int*)t_pos_idx, (const int*)rank, (int)V, (int)T, (int)C, (long long*)face_keys);
    return tt_check_launch();
}

extern "C" int tt_simplify_emit_count(const int64_t* sorted_face_keys, const int64_t* face_perm,
                                      const int32_t* t_pos_idx, const int32_t* rank, int32_t V, int32_t T, int32_t C,
                                      void* workspace, int32_t* out_totals, void* stream) {
    if (!tri_mesh_ok(V, T)) return TT_ERR_BAD_ARG;
    if (!sorted_face_keys || !face_perm || !t_pos_idx || !rank || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    if (const int st = simp_clusters_status(V, C)) return st;
    const SimpWs w = simp_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_simp_keep, dim3((unsigned)w.c.nblk), dim3(SIMP_BLOCK), 0, s,
                       (const long long*)sorted_face_keys, (const long long*)face_perm, (int)T, (int)C, w);
    hipLaunchKernelGGL(k_simp_mark, dim3(tt_grid(T)), dim3(SIMP_BLOCK), 0, s, (const int*)t_pos_idx,
                       (const int*)rank, (int)V, (int)T, (int)C, w);
    tt_compact2_scan_flags(w.cmark, C, w.fkeep, T, w.c, (int*)out_totals, s);
    return tt_check_launch();
}

extern "C" int tt_simplify_emit(const float* cluster_pos, const int32_t* t_pos_idx, const int32_t* rank, int32_t V,
                                int32_t T, int32_t C, void* workspace, float* v_out, int32_t* t_out,
                                int32_t* vertex_map, void* stream) {
    if (!tri_mesh_ok(V, T)) return TT_ERR_BAD_ARG;
    if (!cluster_pos || !t_pos_idx || !rank || !workspace || !v_out || !t_out || !vertex_map) return TT_ERR_BAD_ARG;
    if (const int st = simp_clusters_status(V, C)) return st;
    const SimpWs w = simp_layout(workspace, V, T).w;
    hipLaunchKernelGGL(k_simp_emit, dim3((unsigned)w.c.nblk), dim3(SIMP_BLOCK), 0, (hipStream_t)stream, cluster_pos,
                       (const int*)t_pos_idx, (const int*)rank, (int)V, (int)T, (int)C, w, v_out, (int*)t_out,
                       (int*)vertex_map);
    return tt_check_launch();
}
