// tt_wind.hip -- generalized winding number of a triangle mesh: the exact sum and a Barnes-Hut (dipole) tree.
// The contract (the pair, the exact answer, the tree, the stackless walk) is written in include/tt_abi.h, "winding number".
//   k_wind_face_keys   48-byte record of every triangle (tri_record of tt_trigrid.h) and the Morton key of its centroid's
//                      leaf cell (tri_cell of the cube with G = 2^L); the host sorts (key, face) (stable) and gathers
//                      the records into that order
//   k_wind_leaves      one thread per leaf: N, c, r over the leaf's faces in sorted order
//   k_wind_up          one thread per node of a level, one launch per level: the eight children in child order
//   k_wind_point_keys  Morton key of every point's leaf cell (the host's optional cell-order sort)
//   k_wind_exact       one thread per point, tiles of records staged in LDS, every face in ascending order
//   k_wind_fast        one thread per point, the (l, m) walk
// wind_pair is the only place a (point, triangle) pair is evaluated; each of the two query kernels holds one call of it.
// Sums run in a fixed order in double and there is no float atomic: every table and every answer is deterministic.
#include <math.h>

#include "tt_mask.h"
#include "tt_trigrid.h"

#define WIND_BLOCK TT_ITEM_BLOCK
#define WIND_TILE WIND_BLOCK  // records per LDS tile of k_wind_exact: one per thread, 12 KB

__device__ __forceinline__ float wind_dot(const float x[3], const float y[3]) {
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2];
}

// ---------------------------------------------------------------------------------------------------------------
// the pair: signed solid angle of triangle (a, b, c) seen from p (Van Oosterom-Strackee)
// ---------------------------------------------------------------------------------------------------------------
// atan2 for y != 0 (Cephes' atanf: t = min / max of the magnitudes, reduced about pi/4 above tan(pi/8), a degree-9 odd
// polynomial, about 2 ulp; then the octant).  The device library's atan2f selects on an and of two class compares for
// its inf / inf case, the sequence tt_mask.h rules out; here every select hangs on one compare and the reduction is a
// 0/1 factor, so the quotient is one division: (t - b) / (b t + 1) = (mn - b mx) / (b mn + mx).  inf / inf gives NaN.
__device__ __forceinline__ float wind_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float b = tt_opaque(mn > 0.41421356f * mx ? 1.f : 0.f);
    const float t = (mn - b * mx) / (b * mn + mx);
    const float z = t * t;
    float a = b * 0.78539816f +
              (t + t * z * (((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f));
    a = tt_opaque(ay > ax ? 1.57079633f - a : a);
    a = tt_opaque(x < 0.f ? 3.14159265f - a : a);
    return copysignf(a, y);
}

// num == 0 (of either sign: no area, or p in the triangle's plane) is exactly 0 -- atan2 would turn a zero's sign into
// +-pi where den < 0.  Differences beyond 2^40 overflow the triple products; the NaN of inf - inf counts 0 as well.
__device__ __forceinline__ float wind_pair(const float p[3], const float4 ra, const float4 rb, const float4 rc) {
    const float A[3] = {ra.x - p[0], ra.y - p[1], ra.z - p[2]};
    const float B[3] = {rb.x - p[0], rb.y - p[1], rb.z - p[2]};
    const float C[3] = {rc.x - p[0], rc.y - p[1], rc.z - p[2]};
    const float bxc[3] = {B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]};
    const float num = wind_dot(A, bxc);
    const float la = sqrtf(wind_dot(A, A)), lb = sqrtf(wind_dot(B, B)), lc = sqrtf(wind_dot(C, C));
    const float den = la * lb * lc + wind_dot(A, B) * lc + wind_dot(B, C) * la + wind_dot(C, A) * lb;
    // two selects of one compare each, never a select on an or of two compares (tt_mask.h)
    const float w = tt_opaque(num == 0.f ? 0.f : 2.f * wind_atan2(num, den));
    return w == w ? w : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// cells and keys
// ---------------------------------------------------------------------------------------------------------------
// a leaf cell is tri_cell (tt_trigrid.h) of the cube with G = 2^L
// bit b of (x, y, z) goes to bits 3b+2, 3b+1, 3b: child k = 4 x_bit + 2 y_bit + z_bit of its parent
__device__ __forceinline__ unsigned wind_morton(const int c[3], int L) {
    unsigned key = 0;
    for (int b = 0; b < L; ++b)
        key |= (unsigned)(((c[0] >> b) & 1) << 2 | ((c[1] >> b) & 1) << 1 | ((c[2] >> b) & 1)) << (3 * b);
    return key;
}

__global__ __launch_bounds__(WIND_BLOCK) void k_wind_face_keys(const float* __restrict__ v_pos,
                                                               const int* __restrict__ tri, int V, int T, TriCube g,
                                                               int L, float4* __restrict__ rec,
                                                               long long* __restrict__ keys) {
    const int f = blockIdx.x * WIND_BLOCK + threadIdx.x;
    if (f >= T) return;
    float4 r[3];
    tri_record(v_pos, tri, V, f, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[(size_t)f * 3 + k] = r[k];
    const float third = 0.33333334f;
    const float cen[3] = {__fmul_rn(__fadd_rn(__fadd_rn(r[0].x, r[1].x), r[2].x), third),
                          __fmul_rn(__fadd_rn(__fadd_rn(r[0].y, r[1].y), r[2].y), third),
                          __fmul_rn(__fadd_rn(__fadd_rn(r[0].z, r[1].z), r[2].z), third)};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = tri_cell(cen[a], g.lo[a], g.inv_h, g.G);
    keys[f] = (long long)wind_morton(c, L);
}

__global__ __launch_bounds__(WIND_BLOCK) void k_wind_point_keys(const float* __restrict__ points, int N, TriCube g,
                                                                int L, long long* __restrict__ keys) {
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float p[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    int c[3] = {0, 0, 0};
    const bool ok = tri_finite3(p[0], p[1], p[2]);
    if (ok) tri_point_cell(p, g, c);
    keys[i] = ok ? (long long)wind_morton(c, L) : -1ll;
}

// ---------------------------------------------------------------------------------------------------------------
// node table: level l holds 8^l nodes from node (8^l - 1) / 7 on; a node is two float4: (N, r), (c, A).  r < 0: empty
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned wind_level_base(int l) { return ((1u << (3 * l)) - 1u) / 7u; }

__device__ __forceinline__ void wind_store_node(float4* __restrict__ nodes, size_t idx, const double N[3],
                                                const float c[3], float r, double A) {
    nodes[idx * 2] = make_float4((float)N[0], (float)N[1], (float)N[2], r);
    nodes[idx * 2 + 1] = make_float4(c[0], c[1], c[2], (float)A);
}

__global__ __launch_bounds__(WIND_BLOCK) void k_wind_leaves(const float4* __restrict__ rec,
                                                            const int* __restrict__ leaf_ptr, int T, int L,
                                                            float4* __restrict__ nodes) {
    const unsigned m = blockIdx.x * WIND_BLOCK + threadIdx.x;
    if (m >= 1u << (3 * L)) return;
    const int kb = min(max(leaf_ptr[m], 0), T), ke = min(max(leaf_ptr[m + 1], kb), T);
    double N[3] = {0, 0, 0}, S[3] = {0, 0, 0}, M[3] = {0, 0, 0}, A = 0;
    for (int k = kb; k < ke; ++k) {
        const float4 a = rec[(size_t)k * 3], b = rec[(size_t)k * 3 + 1], c = rec[(size_t)k * 3 + 2];
        const float e1[3] = {b.x - a.x, b.y - a.y, b.z - a.z}, e2[3] = {c.x - a.x, c.y - a.y, c.z - a.z};
        const float n[3] = {0.5f * (e1[1] * e2[2] - e1[2] * e2[1]), 0.5f * (e1[2] * e2[0] - e1[0] * e2[2]),
                            0.5f * (e1[0] * e2[1] - e1[1] * e2[0])};
        const float area = sqrtf(wind_dot(n, n));
        const float cen[3] = {(a.x + b.x + c.x) * 0.33333334f, (a.y + b.y + c.y) * 0.33333334f,
                              (a.z + b.z + c.z) * 0.33333334f};
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            N[x] += (double)n[x];
            S[x] += (double)area * (double)cen[x];
            M[x] += (double)cen[x];
        }
        A += (double)area;
    }
    float cf[3] = {0.f, 0.f, 0.f};
    float r = -1.f;
    if (ke > kb) {
        // faces without area have no weight: then the plain mean of the centroids (N is 0 there, only r uses c)
#pragma unroll
        for (int x = 0; x < 3; ++x) cf[x] = (float)(A > 0 ? S[x] / A : M[x] / (double)(ke - kb));
        float r2 = 0.f;
        for (int k = kb; k < ke; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 v = rec[(size_t)k * 3 + j];
                const float d[3] = {v.x - cf[0], v.y - cf[1], v.z - cf[2]};
                r2 = fmaxf(r2, wind_dot(d, d));
            }
        r = sqrtf(r2);
    }
    wind_store_node(nodes, (size_t)wind_level_base(L) + m, N, cf, r, A);
}

__global__ __launch_bounds__(WIND_BLOCK) void k_wind_up(int l, float4* __restrict__ nodes) {
    const unsigned m = blockIdx.x * WIND_BLOCK + threadIdx.x;
    if (m >= 1u << (3 * l)) return;
    const size_t child = (size_t)wind_level_base(l + 1) + (size_t)m * 8;
    double N[3] = {0, 0, 0}, S[3] = {0, 0, 0}, M[3] = {0, 0, 0}, A = 0;
    int occupied = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 q0 = nodes[(child + k) * 2], q1 = nodes[(child + k) * 2 + 1];
        if (q0.w < 0.f) continue;
        ++occupied;
        N[0] += (double)q0.x, N[1] += (double)q0.y, N[2] += (double)q0.z;
        S[0] += (double)q1.w * (double)q1.x, S[1] += (double)q1.w * (double)q1.y, S[2] += (double)q1.w * (double)q1.z;
        M[0] += (double)q1.x, M[1] += (double)q1.y, M[2] += (double)q1.z;
        A += (double)q1.w;
    }
    float cf[3] = {0.f, 0.f, 0.f};
    float r = -1.f;
    if (occupied) {
#pragma unroll
        for (int x = 0; x < 3; ++x) cf[x] = (float)(A > 0 ? S[x] / A : M[x] / (double)occupied);
        r = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 q0 = nodes[(child + k) * 2], q1 = nodes[(child + k) * 2 + 1];
            const float d[3] = {q1.x - cf[0], q1.y - cf[1], q1.z - cf[2]};
            if (q0.w >= 0.f) r = fmaxf(r, sqrtf(wind_dot(d, d)) + q0.w);
        }
    }
    wind_store_node(nodes, (size_t)wind_level_base(l) + m, N, cf, r, A);
}

// ---------------------------------------------------------------------------------------------------------------
// queries
// ---------------------------------------------------------------------------------------------------------------
#define WIND_INV_4PI 0.07957747154594767

__global__ __launch_bounds__(WIND_BLOCK) void k_wind_exact(const float* __restrict__ points, int N,
                                                           const float4* __restrict__ rec, int T,
                                                           float* __restrict__ out) {
    __shared__ float4 tile[WIND_TILE * 3];
    const int i = blockIdx.x * WIND_BLOCK + threadIdx.x;
    float p[3] = {0.f, 0.f, 0.f};
    if (i < N) {
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = points[(size_t)i * 3 + a];
    }
    // a point that is not finite stages its share of every tile and takes no part in the pair loop
    const bool live = i < N && tri_finite3(p[0], p[1], p[2]);
    double acc = 0.0;
    for (int base = 0; base < T; base += WIND_TILE) {
        const int n = min(WIND_TILE, T - base);
        if ((int)threadIdx.x < n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) tile[threadIdx.x * 3 + k] = rec[(size_t)(base + threadIdx.x) * 3 + k];
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < n; ++k)  // every lane reads the same record: a broadcast
                acc += (double)wind_pair(p, tile[k * 3], tile[k * 3 + 1], tile[k * 3 + 2]);
        }
        __syncthreads();
    }
    if (i < N) out[i] = live ? (float)(acc * WIND_INV_4PI) : tri_nan();
}

__global__ __launch_bounds__(WIND_BLOCK) void k_wind_fast(const float* __restrict__ points,
                                                          const long long* __restrict__ order, int N,
                                                          const float4* __restrict__ rec,
                                                          const int* __restrict__ leaf_ptr,
                                                          const float4* __restrict__ nodes, int T, int L, float beta,
                                                          float* __restrict__ out) {
    const int t = blockIdx.x * WIND_BLOCK + threadIdx.x;
    if (t >= N) return;
    const long long i = tri_row(order, t, N);
    if (i < 0) return;
    const float p[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    if (!tri_finite3(p[0], p[1], p[2])) {  // before the walk: no loop depends on such a point
        out[i] = tri_nan();
        return;
    }
    double acc = 0.0;
    int l = 0;
    unsigned m = 0;
    for (;;) {  // at most one visit of each of the (8^(L+1) - 1) / 7 nodes: m < 8^l and l <= L throughout
        const size_t idx = (size_t)wind_level_base(l) + m;
        const float4 q0 = nodes[idx * 2];
        bool descend = false;
        if (q0.w >= 0.f) {
            const float4 q1 = nodes[idx * 2 + 1];
            const float d[3] = {q1.x - p[0], q1.y - p[1], q1.z - p[2]};
            const float d2 = wind_dot(d, d), br = beta * q0.w;
            // the dipole term of every occupied node, times a 0/1 factor: the select that drops a term that is not
            // finite (a node without extent at the point itself) must not share a mask with the far test (tt_mask.h)
            const float nd = q0.x * d[0] + q0.y * d[1] + q0.z * d[2];
            const float term = tt_opaque(nd / (d2 * sqrtf(d2)));
            const float far = tt_opaque(d2 > br * br ? 1.f : 0.f);
            acc += (double)(far * tt_opaque(fabsf(term) <= 3.4028235e38f ? term : 0.f));
            descend = far == 0.f && l < L;
            if (far == 0.f && l == L) {
                const int kb = min(max(leaf_ptr[m], 0), T), ke = min(max(leaf_ptr[m + 1], kb), T);
                for (int k = kb; k < ke; ++k)
                    acc += (double)wind_pair(p, rec[(size_t)k * 3], rec[(size_t)k * 3 + 1], rec[(size_t)k * 3 + 2]);
            }
        }
        if (descend) {
            ++l;
            m <<= 3;
            continue;
        }
        while (l > 0 && (m & 7u) == 7u) {
            m >>= 3;
            --l;
        }
        if (l == 0) break;
        ++m;
    }
    out[i] = (float)(acc * WIND_INV_4PI);
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
static bool wind_levels_ok(int32_t L) { return L >= 0 && L <= TT_WIND_MAX_LEVELS; }
// the cube of a tree of L levels: G = 2^L leaf cells per axis
static bool wind_cube(int32_t L, float lo_x, float lo_y, float lo_z, float ext, float inv_h, TriCube* out) {
    return wind_levels_ok(L) && tri_cube(1 << L, 1 << TT_WIND_MAX_LEVELS, lo_x, lo_y, lo_z, ext, 0.f, inv_h, out);
}

extern "C" int64_t tt_wind_node_count(int32_t levels) {
    if (!wind_levels_ok(levels)) return TT_ERR_BAD_ARG;
    return (int64_t)wind_level_base(levels + 1);
}

extern "C" int tt_wind_face_keys(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T, int32_t levels,
                                 float lo_x, float lo_y, float lo_z, float ext, float inv_h, float* records,
                                 int64_t* keys, void* stream) {
    TriCube g;
    if (!tri_mesh_ok(V, T) || !wind_cube(levels, lo_x, lo_y, lo_z, ext, inv_h, &g))
        return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !records || !keys) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_wind_face_keys, dim3(tt_grid(T)), dim3(WIND_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, (int)V, (int)T, g, (int)levels, (float4*)records, (long long*)keys);
    return tt_check_launch();
}

extern "C" int tt_wind_build(const float* sorted_records, const int32_t* leaf_ptr, int32_t T, int32_t levels,
                             float* nodes, void* stream) {
    if (!tri_count_ok(T) || !wind_levels_ok(levels)) return TT_ERR_BAD_ARG;
    if (!sorted_records || !leaf_ptr || !nodes) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_wind_leaves, dim3(tt_grid(1ll << (3 * levels))), dim3(WIND_BLOCK), 0, s,
                       (const float4*)sorted_records, (const int*)leaf_ptr, (int)T, (int)levels, (float4*)nodes);
    for (int l = levels - 1; l >= 0; --l)
        hipLaunchKernelGGL(k_wind_up, dim3(tt_grid(1ll << (3 * l))), dim3(WIND_BLOCK), 0, s, l, (float4*)nodes);
    return tt_check_launch();
}

extern "C" int tt_wind_point_keys(const float* points, int32_t N, int32_t levels, float lo_x, float lo_y, float lo_z,
                                  float ext, float inv_h, int64_t* keys, void* stream) {
    TriCube g;
    if (!tri_items_ok(N) || !wind_cube(levels, lo_x, lo_y, lo_z, ext, inv_h, &g)) return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!points || !keys) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_wind_point_keys, dim3(tt_grid(N)), dim3(WIND_BLOCK), 0, (hipStream_t)stream, points, (int)N, g,
                       (int)levels, (long long*)keys);
    return tt_check_launch();
}

extern "C" int tt_wind_exact(const float* points, int32_t N, const float* records, int32_t T, float* out,
                             void* stream) {
    if (!tri_items_ok(N) || !tri_count_ok(T)) return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!points || !records || !out) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_wind_exact, dim3(tt_grid(N)), dim3(WIND_BLOCK), 0, (hipStream_t)stream, points, (int)N,
                       (const float4*)records, (int)T, out);
    return tt_check_launch();
}

extern "C" int tt_wind_fast(const float* points, const int64_t* order, int32_t N, const float* sorted_records,
                            const int32_t* leaf_ptr, const float* nodes, int32_t T, int32_t levels, float beta,
                            float* out, void* stream) {
    if (!tri_items_ok(N) || !tri_count_ok(T) || !wind_levels_ok(levels) || !(beta > 0.f))
        return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!points || !sorted_records || !leaf_ptr || !nodes || !out) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_wind_fast, dim3(tt_grid(N)), dim3(WIND_BLOCK), 0, (hipStream_t)stream, points,
                       (const long long*)order, (int)N, (const float4*)sorted_records, (const int*)leaf_ptr,
                       (const float4*)nodes, (int)T, (int)levels, beta, out);
    return tt_check_launch();
}
