// tt_dist.hip -- closest point on a triangle mesh (uniform grid, exact, deterministic), its backward pass, and the
// surface sampler.  The contract (per-pair arithmetic, the (d2, face) answer, grid, ring search and its stopping rule,
// backward, sampler) is written in include/tt_abi.h, "point-to-mesh distance".
//   k_dist_build    48-byte record of every triangle, triangles per overlapped cell (integer atomics)
//                   -> tt_exclusive_scan -> cell_ptr; M read back by the host
//   k_dist_fill     cell_tri: every triangle into the rows of the cells its box overlaps
//   k_dist_keys     cell key of every point (the host's optional cell-order sort)
//   k_dist_query    one thread per point: Chebyshev rings around the point's cell until the bound passes the best d2
//   k_dist_bwd      grad_points written, grad_v_pos by float atomicAdd, the face fixed
//   k_dist_sample_count -> tt_exclusive_scan<long long> -> k_dist_sample_emit   one thread per sample
// The answer of a query is the lexicographic minimum of (d2, face) over ALL triangles; dist_closest is the only place a
// pair is evaluated and k_dist_query holds its only call, so neither the grid, the order inside a cell nor the launch
// can change a bit of it.  The cube, its cell rule, the record, the `order` lookup, the grid's device view and the
// argument checks are tt_trigrid.h, shared with tt_ray.hip, tt_wind.hip and tt_simplify.hip.
#include <math.h>

#include "tt_scan.h"
#include "tt_trigrid.h"

#define DIST_BLOCK TT_ITEM_BLOCK

struct DistWs {
    int *xs, *cursor;
};
struct DistLayout {
    DistWs w;
    long long bytes;
};
static DistLayout dist_layout(void* base, long long cells) {
    TtCarver c{(char*)base};
    DistLayout l;
    l.w.xs = c.take<int>(tt_xscan_blocks(cells) + 1);  // block sums of the scan of the cell counts
    l.w.cursor = c.take<int>(cells);                   // [G^3] rows filled so far (tt_dist_build_fill)
    l.bytes = c.bytes();
    return l;
}

// ---------------------------------------------------------------------------------------------------------------
// the pair: closest point on triangle (a, b, c) to p
// ---------------------------------------------------------------------------------------------------------------
struct DistHit {
    float d2, v, w;  // barycentrics (1 - v - w, v, w)
};

__device__ __forceinline__ float dist_dot(const float x[3], const float y[3]) {
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2];
}
__device__ __forceinline__ void dist_cross(const float x[3], const float y[3], float o[3]) {
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}
// parameter of the closest point on the segment from the origin along e (e.e = ee) to the point with e.x = t
__device__ __forceinline__ float dist_seg_t(float t, float ee) {
    return ee > 0.f ? fminf(fmaxf(t / ee, 0.f), 1.f) : 0.f;
}

// Voronoi regions (Ericson 5.1.5): the vertex regions from the six edge projections; the edge and face regions from the
// signed areas va, vb, vc -- taken as n . (edge x offset) rather than as differences of products of the projections,
// which cancel to noise once |p - a| is a few hundred edge lengths.  A triangle whose normal vanishes (sin^2 of the
// angle at a below 1e-12, equal vertices included) is the union of its three edge segments.  Never NaN for finite input.
__device__ __forceinline__ DistHit dist_closest(const float p[3], const float a[3], const float b[3], const float c[3]) {
    float ab[3], ac[3], ap[3], bp[3], cp[3], n[3], t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k];
        bp[k] = p[k] - b[k];
        cp[k] = p[k] - c[k];
    }
    const float d1 = dist_dot(ab, ap), d2 = dist_dot(ac, ap);
    const float d3 = dist_dot(ab, bp), d4 = dist_dot(ac, bp);
    const float d5 = dist_dot(ab, cp), d6 = dist_dot(ac, cp);
    const float ab2 = dist_dot(ab, ab), ac2 = dist_dot(ac, ac);
    dist_cross(ab, ac, n);
    const float nn = dist_dot(n, n);
    float v, w;
    if (!(nn > 1e-12f * ab2 * ac2)) {
        // degenerate: the nearest of the three segments, ties to ab, then ac, then bc
        const float tab = dist_seg_t(d1, ab2), tac = dist_seg_t(d2, ac2);
        float bc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) bc[k] = c[k] - b[k];
        const float tbc = dist_seg_t(dist_dot(bc, bp), dist_dot(bc, bc));
        float e0 = 0.f, e1 = 0.f, e2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x0 = ap[k] - tab * ab[k], x1 = ap[k] - tac * ac[k], x2 = bp[k] - tbc * bc[k];
            e0 += x0 * x0;
            e1 += x1 * x1;
            e2 += x2 * x2;
        }
        v = tab;
        w = 0.f;
        float e = e0;
        if (e1 < e) {
            e = e1;
            v = 0.f;
            w = tac;
        }
        if (e2 < e) {
            v = 1.f - tbc;
            w = tbc;
        }
    } else if (d1 <= 0.f && d2 <= 0.f) {
        v = 0.f;
        w = 0.f;
    } else if (d3 >= 0.f && d4 <= d3) {
        v = 1.f;
        w = 0.f;
    } else if (d6 >= 0.f && d5 <= d6) {
        v = 0.f;
        w = 1.f;
    } else {
        dist_cross(ab, ap, t);
        const float vc = dist_dot(n, t);
        dist_cross(ap, ac, t);
        const float vb = dist_dot(n, t);
        float bc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) bc[k] = c[k] - b[k];
        dist_cross(bc, bp, t);
        const float va = dist_dot(n, t);
        if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
            v = dist_seg_t(d1, ab2);
            w = 0.f;
        } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
            v = 0.f;
            w = dist_seg_t(d2, ac2);
        } else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {
            w = dist_seg_t(d4 - d3, (d4 - d3) + (d5 - d6));
            v = 1.f - w;
        } else {
            // inside: the three areas are positive here (or the point sits on the noise of a boundary: clamped)
            const float pa = fmaxf(va, 0.f), pb = fmaxf(vb, 0.f), pc = fmaxf(vc, 0.f);
            const float s = pa + pb + pc;
            v = s > 0.f ? pb / s : 0.f;
            w = s > 0.f ? pc / s : 0.f;
        }
    }
    DistHit hit;
    hit.v = v;
    hit.w = w;
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = ap[k] - (v * ab[k] + w * ac[k]);
        e += x * x;
    }
    hit.d2 = e;
    return hit;
}

// ---------------------------------------------------------------------------------------------------------------
// grid build
// ---------------------------------------------------------------------------------------------------------------
// the cells of a triangle's box: tri_cell (tt_trigrid.h) of its two corners; monotone, which is all the search's bound needs
__device__ __forceinline__ void dist_tri_cells(const float4 r0, const float4 r1, const float4 r2, const TriCube& g,
                                               int c0[3], int c1[3]) {
    const float mn[3] = {fminf(r0.x, fminf(r1.x, r2.x)), fminf(r0.y, fminf(r1.y, r2.y)), fminf(r0.z, fminf(r1.z, r2.z))};
    const float mx[3] = {fmaxf(r0.x, fmaxf(r1.x, r2.x)), fmaxf(r0.y, fmaxf(r1.y, r2.y)), fmaxf(r0.z, fmaxf(r1.z, r2.z))};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c0[a] = tri_cell(mn[a], g.lo[a], g.inv_h, g.G);
        c1[a] = max(c0[a], tri_cell(mx[a], g.lo[a], g.inv_h, g.G));
    }
}

__global__ __launch_bounds__(DIST_BLOCK) void k_dist_zero(int* __restrict__ a, long long na, int* __restrict__ b,
                                                          long long nb, unsigned long long* __restrict__ total) {
    const long long i = (long long)blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (i < na) a[i] = 0;
    if (i < nb) b[i] = 0;
    if (i == 0 && total) *total = 0ull;
}

__global__ __launch_bounds__(DIST_BLOCK) void k_dist_build(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                           int V, int T, TriCube g, float4* __restrict__ rec,
                                                           int* __restrict__ cell_cnt,
                                                           unsigned long long* __restrict__ total) {
    const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (f >= T) return;
    float4 r[3];
    tri_record(v_pos, tri, V, f, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[(size_t)f * 3 + k] = r[k];
    int c0[3], c1[3];
    dist_tri_cells(r[0], r[1], r[2], g, c0, c1);
    for (int z = c0[0]; z <= c1[0]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[2]; x <= c1[2]; ++x) atomicAdd(cell_cnt + ((size_t)z * g.G + y) * g.G + x, 1);
    atomicAdd(total, (unsigned long long)(c1[0] - c0[0] + 1) * (unsigned long long)(c1[1] - c0[1] + 1) *
                         (unsigned long long)(c1[2] - c0[2] + 1));
}

__global__ __launch_bounds__(DIST_BLOCK) void k_dist_fill(const float4* __restrict__ rec, int T, TriCube g,
                                                          const int* __restrict__ cell_ptr, int* __restrict__ cursor,
                                                          int M, int* __restrict__ cell_tri) {
    const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (f >= T) return;
    int c0[3], c1[3];
    dist_tri_cells(rec[(size_t)f * 3], rec[(size_t)f * 3 + 1], rec[(size_t)f * 3 + 2], g, c0, c1);
    for (int z = c0[0]; z <= c1[0]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[2]; x <= c1[2]; ++x) {
                const size_t cell = ((size_t)z * g.G + y) * g.G + x;
                const int slot = cell_ptr[cell] + atomicAdd(cursor + cell, 1);
                if (slot >= 0 && slot < cell_ptr[cell + 1] && slot < M) cell_tri[slot] = f;  // bound of every write
            }
}

// ---------------------------------------------------------------------------------------------------------------
// query
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DIST_BLOCK) void k_dist_keys(const float* __restrict__ points, int N, TriCube g,
                                                          long long* __restrict__ keys) {
    const int i = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float p[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    int c[3] = {0, 0, 0};
    const bool ok = tri_finite3(p[0], p[1], p[2]);
    if (ok) tri_point_cell(p, g, c);
    keys[i] = ok ? (long long)tri_key(c, g.G) : -1ll;
}

struct DistBest {
    float d2, v, w;
    int f;
};

__global__ __launch_bounds__(DIST_BLOCK) void k_dist_query(const float* __restrict__ points,
                                                           const long long* __restrict__ order, int N,
                                                           TriGridView grid, float* __restrict__ out_d2,
                                                           int* __restrict__ out_face, float* __restrict__ out_bary) {
    const int t = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (t >= N) return;
    const long long i = tri_row(order, t, N);
    if (i < 0) return;
    const TriCube& g = grid.cube;
    const float p[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    if (!tri_finite3(p[0], p[1], p[2])) {  // before the search: no loop depends on such a point
        out_d2[i] = tri_nan();
        out_face[i] = -1;
        out_bary[(size_t)i * 3] = out_bary[(size_t)i * 3 + 1] = out_bary[(size_t)i * 3 + 2] = 0.f;
        return;
    }
    int c[3];
    const float pq2 = tri_point_cell(p, g, c);
    const int G = g.G;
    const int rmax = max(max(max(c[0], G - 1 - c[0]), max(c[1], G - 1 - c[1])), max(c[2], G - 1 - c[2]));
    DistBest best{tri_inf(), 0.f, 0.f, 0x7fffffff};
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(c[0] - r, 0), z1 = min(c[0] + r, G - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, G - 1);
        const int x0 = c[2] - r, x1 = c[2] + r;
        for (int z = z0; z <= z1; ++z) {
            const bool zshell = z - c[0] == r || c[0] - z == r;
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * G + y) * G;
                // the row's cells of this ring: all of its span on the shell's faces, else its two end cells (r >= 1).
                // Consecutive cells along x are consecutive CSR rows: one span is one range of cell_tri.
                const bool whole = zshell || y - c[1] == r || c[1] - y == r;
                const int s0[2] = {whole ? max(x0, 0) : x0, x1};
                const int s1[2] = {whole ? min(x1, G - 1) : x0, whole ? x1 - 1 : x1};  // whole: the second span is empty
#pragma nounroll
                for (int sp = 0; sp < 2; ++sp) {  // one loop, so dist_closest has one call site and one instruction stream
                    if (s0[sp] < 0 || s1[sp] > G - 1 || s0[sp] > s1[sp]) continue;
                    int kb, ke;
                    tri_rows(grid, row + s0[sp], row + s1[sp], kb, ke);
                    for (int k = kb; k < ke; ++k) {
                        const int f = grid.cell_tri[k];
                        if (!tri_face_ok(grid, f)) continue;
                        const float4 r0 = grid.rec[(size_t)f * 3], r1 = grid.rec[(size_t)f * 3 + 1],
                                     r2 = grid.rec[(size_t)f * 3 + 2];
                        const float ta[3] = {r0.x, r0.y, r0.z}, tb[3] = {r1.x, r1.y, r1.z}, tc[3] = {r2.x, r2.y, r2.z};
                        const DistHit hit = dist_closest(p, ta, tb, tc);
                        if (hit.d2 < best.d2 || (hit.d2 == best.d2 && f < best.f)) {
                            best.d2 = hit.d2;
                            best.v = hit.v;
                            best.w = hit.w;
                            best.f = f;
                        }
                    }
                }
            }
        }
        // every triangle not yet seen is at squared distance >= |p - q|^2 + (r h)^2; strictly below the (rounding-safe)
        // bound, nothing unseen can win or tie
        const float rr = fmaxf((float)r - 0.015625f, 0.f) * g.h;
        if (best.d2 < pq2 * 0.99998474f + rr * rr) break;
    }
    const bool hit = best.f != 0x7fffffff;
    out_d2[i] = best.d2;
    out_face[i] = hit ? best.f : -1;
    out_bary[(size_t)i * 3] = hit ? fmaxf(1.f - best.v - best.w, 0.f) : 0.f;
    out_bary[(size_t)i * 3 + 1] = hit ? best.v : 0.f;
    out_bary[(size_t)i * 3 + 2] = hit ? best.w : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// backward: d(d2)/dp = 2 (p - c), d(d2)/dv_k = -2 b_k (p - c), the face and its barycentrics fixed
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DIST_BLOCK) void k_dist_bwd(const float* __restrict__ points,
                                                         const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                         const int* __restrict__ face, const float* __restrict__ bary,
                                                         const float* __restrict__ g_d2, int N, int V, int T,
                                                         float* __restrict__ grad_points, float* __restrict__ grad_v) {
    const int i = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int f = face[i];
    unsigned idx[3] = {0, 0, 0};
    unsigned bad = (unsigned)((unsigned)f >= (unsigned)T);
    const int fs = bad ? 0 : f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = (unsigned)tri[(size_t)fs * 3 + k];
        bad |= (unsigned)(idx[k] >= (unsigned)V);
        idx[k] = min(idx[k], (unsigned)(V - 1));
    }
    float d[3] = {0.f, 0.f, 0.f};
    const float b[3] = {bary[(size_t)i * 3], bary[(size_t)i * 3 + 1], bary[(size_t)i * 3 + 2]};
    if (!bad) {
        const float s = 2.f * g_d2[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float cpt = b[0] * v_pos[(size_t)idx[0] * 3 + a] + b[1] * v_pos[(size_t)idx[1] * 3 + a] +
                              b[2] * v_pos[(size_t)idx[2] * 3 + a];
            d[a] = s * (points[(size_t)i * 3 + a] - cpt);
        }
    }
    if (grad_points) {
#pragma unroll
        for (int a = 0; a < 3; ++a) grad_points[(size_t)i * 3 + a] = d[a];
    }
    if (grad_v && !bad) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) atomicAdd(grad_v + (size_t)idx[k] * 3 + a, -b[k] * d[a]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// surface sampler
// ---------------------------------------------------------------------------------------------------------------
#define DIST_SAMPLE_MAX_K 131072  // a face beyond this has more samples than TT_DIST_MAX_SAMPLES by itself

// k_f = max(1, ceil(L_f / spacing)), L_f the fp32 longest edge: every product and sum rounded on its own
__device__ __forceinline__ int dist_face_k(const float4 p[3], float spacing) {
    float l2 = 0.f;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int j = (e + 1) % 3;
        const float x = __fsub_rn(p[j].x, p[e].x), y = __fsub_rn(p[j].y, p[e].y), z = __fsub_rn(p[j].z, p[e].z);
        l2 = fmaxf(l2, __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    }
    const float k = ceilf(__fdiv_rn(__fsqrt_rn(l2), spacing));
    return k >= (float)DIST_SAMPLE_MAX_K ? DIST_SAMPLE_MAX_K : max(1, (int)k);  // NaN: 1
}

__global__ __launch_bounds__(DIST_BLOCK) void k_dist_sample_count(const float* __restrict__ v_pos,
                                                                  const int* __restrict__ tri, int V, int T,
                                                                  float spacing, long long* __restrict__ cnt) {
    const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (f >= T) return;
    float4 p[3];
    tri_record(v_pos, tri, V, f, p);
    const long long k = dist_face_k(p, spacing);
    cnt[f] = (k + 1) * (k + 2) / 2;
}

__global__ __launch_bounds__(DIST_BLOCK) void k_dist_sample_emit(const float* __restrict__ v_pos,
                                                                 const int* __restrict__ tri,
                                                                 const long long* __restrict__ offs, int V, int T,
                                                                 float spacing, int S, float* __restrict__ out,
                                                                 int* __restrict__ out_face) {
    const int s = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (s >= S) return;
    // the face: the last f with offs[f] <= s
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= (long long)s) lo = mid; else hi = mid - 1;
    }
    const int f = lo;
    float4 p[3];
    tri_record(v_pos, tri, V, f, p);
    const int k = dist_face_k(p, spacing);
    const long long m = min(max((long long)s - offs[f], 0ll), ((long long)k + 1) * (k + 2) / 2 - 1);
    // row i starts at i (k + 1) - i (i - 1) / 2 and holds j = 0 .. k - i
    const double B = 2.0 * k + 3.0;
    int i = (int)((B - sqrt(fmax(B * B - 8.0 * (double)m, 0.0))) * 0.5);
    i = min(max(i, 0), k);
    for (int it = 0; it < 2 && i < k && (long long)(i + 1) * (k + 1) - (long long)(i + 1) * i / 2 <= m; ++it) ++i;
    for (int it = 0; it < 2 && i > 0 && (long long)i * (k + 1) - (long long)i * (i - 1) / 2 > m; ++it) --i;
    const int j = (int)(m - ((long long)i * (k + 1) - (long long)i * (i - 1) / 2));
    const float fi = (float)i / (float)k, fj = (float)j / (float)k;
    out[(size_t)s * 3] = p[0].x + fi * (p[1].x - p[0].x) + fj * (p[2].x - p[0].x);
    out[(size_t)s * 3 + 1] = p[0].y + fi * (p[1].y - p[0].y) + fj * (p[2].y - p[0].y);
    out[(size_t)s * 3 + 2] = p[0].z + fi * (p[1].z - p[0].z) + fj * (p[2].z - p[0].z);
    out_face[s] = f;
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
static long long dist_grid_size(int32_t G) { return (long long)G * G * G; }

extern "C" int64_t tt_dist_workspace_bytes(int32_t grid) {
    if (grid < 1 || grid > TT_DIST_MAX_GRID) return TT_ERR_BAD_ARG;
    return dist_layout(nullptr, dist_grid_size(grid)).bytes;
}

extern "C" int tt_dist_build_count(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T, int32_t grid,
                                   float lo_x, float lo_y, float lo_z, float ext, float inv_h, void* workspace,
                                   float* records, int32_t* cell_ptr, int64_t* out_total, void* stream) {
    TriCube g;
    if (!tri_mesh_ok(V, T) || !tri_cube(grid, TT_DIST_MAX_GRID, lo_x, lo_y, lo_z, ext, 0.f, inv_h, &g))
        return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !workspace || !records || !cell_ptr || !out_total) return TT_ERR_BAD_ARG;
    const long long cells = dist_grid_size(grid);
    const DistWs w = dist_layout(workspace, cells).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dist_zero, dim3(tt_grid(cells + 1)), dim3(DIST_BLOCK), 0, s, (int*)cell_ptr, cells + 1,
                       w.cursor, cells, (unsigned long long*)out_total);
    hipLaunchKernelGGL(k_dist_build, dim3(tt_grid(T)), dim3(DIST_BLOCK), 0, s, v_pos, (const int*)t_pos_idx, (int)V,
                       (int)T, g, (float4*)records, (int*)cell_ptr, (unsigned long long*)out_total);
    tt_exclusive_scan<int>((int*)cell_ptr, cells, (int*)cell_ptr, w.xs, (int*)cell_ptr + cells, s);
    return tt_check_launch();
}

extern "C" int tt_dist_build_fill(const float* records, int32_t T, int32_t grid, float lo_x, float lo_y, float lo_z,
                                  float ext, float inv_h, void* workspace, const int32_t* cell_ptr, int32_t M,
                                  int32_t* cell_tri, void* stream) {
    TriCube g;
    if (!tri_count_ok(T) || M < 1 || !tri_cube(grid, TT_DIST_MAX_GRID, lo_x, lo_y, lo_z, ext, 0.f, inv_h, &g))
        return TT_ERR_BAD_ARG;
    if (!records || !workspace || !cell_ptr || !cell_tri) return TT_ERR_BAD_ARG;
    const DistWs w = dist_layout(workspace, dist_grid_size(grid)).w;
    hipLaunchKernelGGL(k_dist_fill, dim3(tt_grid(T)), dim3(DIST_BLOCK), 0, (hipStream_t)stream,
                       (const float4*)records, (int)T, g, (const int*)cell_ptr, w.cursor, (int)M, (int*)cell_tri);
    return tt_check_launch();
}

extern "C" int tt_dist_keys(const float* points, int32_t N, int32_t grid, float lo_x, float lo_y, float lo_z, float ext,
                            float inv_h, int64_t* keys, void* stream) {
    TriCube g;
    if (!tri_items_ok(N) || !tri_cube(grid, TT_DIST_MAX_GRID, lo_x, lo_y, lo_z, ext, 0.f, inv_h, &g))
        return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!points || !keys) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_dist_keys, dim3(tt_grid(N)), dim3(DIST_BLOCK), 0, (hipStream_t)stream, points, (int)N, g,
                       (long long*)keys);
    return tt_check_launch();
}

extern "C" int tt_dist_query(const float* points, const int64_t* order, int32_t N, const float* records,
                             const int32_t* cell_ptr, const int32_t* cell_tri, int32_t T, int32_t M, int32_t grid,
                             float lo_x, float lo_y, float lo_z, float ext, float h, float inv_h, float* d2,
                             int32_t* face, float* bary, void* stream) {
    TriGridView g;
    if (!tri_view(N, records, cell_ptr, cell_tri, T, M, grid, lo_x, lo_y, lo_z, ext, h, inv_h, &g))
        return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!points || !d2 || !face || !bary) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_dist_query, dim3(tt_grid(N)), dim3(DIST_BLOCK), 0, (hipStream_t)stream, points,
                       (const long long*)order, (int)N, g, d2, (int*)face, bary);
    return tt_check_launch();
}

extern "C" int tt_dist_bwd(const float* points, const float* v_pos, const int32_t* t_pos_idx, const int32_t* face,
                           const float* bary, const float* g_d2, int32_t N, int32_t V, int32_t T, float* grad_points,
                           float* grad_v_pos, void* stream) {
    if (!tri_items_ok(N) || !tri_mesh_ok(V, T)) return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!points || !v_pos || !t_pos_idx || !face || !bary || !g_d2 || (!grad_points && !grad_v_pos))
        return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_dist_bwd, dim3(tt_grid(N)), dim3(DIST_BLOCK), 0, (hipStream_t)stream, points, v_pos,
                       (const int*)t_pos_idx, (const int*)face, bary, g_d2, (int)N, (int)V, (int)T, grad_points,
                       grad_v_pos);
    return tt_check_launch();
}

extern "C" int64_t tt_dist_sample_workspace_bytes(int32_t T) {
    if (!tri_count_ok(T)) return TT_ERR_BAD_ARG;
    TtCarver c{nullptr};
    c.take<long long>(tt_xscan_blocks(T) + 1);
    return c.bytes();
}

extern "C" int tt_dist_sample_count(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T, float spacing,
                                    void* workspace, int64_t* offsets, void* stream) {
    if (!tri_mesh_ok(V, T) || !tri_finite(spacing) || !(spacing > 0.f)) return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !workspace || !offsets) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dist_sample_count, dim3(tt_grid(T)), dim3(DIST_BLOCK), 0, s, v_pos, (const int*)t_pos_idx,
                       (int)V, (int)T, spacing, (long long*)offsets);
    tt_exclusive_scan<long long>((long long*)offsets, T, (long long*)offsets, (long long*)workspace,
                                 (long long*)offsets + T, s);
    return tt_check_launch();
}

extern "C" int tt_dist_sample_emit(const float* v_pos, const int32_t* t_pos_idx, const int64_t* offsets, int32_t V,
                                   int32_t T, float spacing, int32_t S, float* points, int32_t* face, void* stream) {
    if (!tri_mesh_ok(V, T) || !tri_finite(spacing) || !(spacing > 0.f) || S < 1 || S > TT_DIST_MAX_SAMPLES)
        return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !offsets || !points || !face) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_dist_sample_emit, dim3(tt_grid(S)), dim3(DIST_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, (const long long*)offsets, (int)V, (int)T, spacing, (int)S, points,
                       (int*)face);
    return tt_check_launch();
}
