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

// ---------------------------------------------------------------------------------------------------------------
// mesh to SDF grid (include/tt_abi.h, "mesh to SDF grid"): the fourth consumer of the triangle record, the other way
// round -- triangles scatter to the grid corners near them.
//   k_sdf_count    work items of every triangle -> tt_exclusive_scan<long long> -> offsets, the total stays on the device
//   k_sdf_scatter  one thread per item (triangle, one i-plane x SDF_ROWS rows of its grown box): dist_closest at every
//                  corner that can be within reach, 64-bit integer atomicMin of (bits of d2) << 32 | face
//   k_sdf_flags    the corners some triangle reached (the CANDIDATES) -> tt_compact.h; k_sdf_emit: their ids, positions
//   k_sdf_keys     the query's (d2, face) and the sign of every candidate, handed back by the host, into keys / level
//   k_sdf_finish   one wave per (i, j) row: level and face of every corner, the far sign carried along the row
// The scatter's own d2 is NOT the query's bit for bit, although both call dist_closest under this file's contraction
// setting: inlined into two kernels the function is scheduled and fused twice, and on 30 % of the band corners of a
// 32^3 sphere the two d2 differ in the last bit (measured; an optimisation barrier on the twelve inputs did not change
// that).  So the scatter only FINDS the corners near the surface, with a margin far above that last bit, and the host
// runs k_dist_query itself on them -- near points, which the ring search is built for.  What is written to level and
// face is the query's answer by construction.
// ---------------------------------------------------------------------------------------------------------------
#include "tt_compact.h"

#define SDF_ROWS 4               // rows (second axis) of one work item
#define SDF_EMPTY (~0ull)        // a key no triangle reached: its d2 half is a NaN, which fails both band tests
#define SDF_SCATTER_BLOCKS 4096  // grid-stride blocks of k_sdf_scatter (the item count never leaves the device)

struct SdfGrid {
    float lo[3], h, tau, sign_tau;
    double reach, mag;  // sign_tau / h + 1/100 cells; max |lo_a| + R h, the largest coordinate of a corner
    int R;
};
struct SdfWs {
    unsigned long long* keys;
    long long *offs, *xs;
    int* tot;
    TtCompact2 cmp;
};
struct SdfLayout {
    SdfWs w;
    long long bytes;
};
static SdfLayout sdf_layout(void* base, long long R, long long T) {
    TtCarver c{(char*)base};
    SdfLayout l;
    const long long n = R * R * R;
    l.w.keys = c.take<unsigned long long>(n);
    l.w.offs = c.take<long long>(T + 1);
    l.w.xs = c.take<long long>(tt_xscan_blocks(T) + 1);
    l.w.tot = c.take<int>(2);
    l.w.cmp = tt_compact2_carve(c, n, l.w.tot);
    l.bytes = c.bytes();
    return l;
}

// corner i of an axis: fl(lo + fl(i * h)), the product and the sum each rounded, whatever the file's setting
__device__ __forceinline__ float sdf_corner(float lo, int i, float h) {
#pragma clang fp contract(off)
    const float s = (float)i * h;
    return lo + s;
}

// The corners [c0, c1] per axis a triangle can reach (empty: c0 > c1 on some axis) and the squared distance `lim` up
// to which a corner is a candidate.  The reach is sign_tau plus a slack: 1/100 cell, and 2^-18 of the largest
// coordinate in play (d2 is a difference of vectors that long, each rounded to 2^-24 of it a few times over; a corner
// carries two such roundings).  A record that is not finite reaches nothing.
__device__ __forceinline__ bool sdf_box(const float4 r0, const float4 r1, const float4 r2, const SdfGrid& g, int c0[3],
                                        int c1[3], float mn[3], float mx[3], float* lim) {
    if (!tri_finite3(r0.x, r0.y, r0.z) || !tri_finite3(r1.x, r1.y, r1.z) || !tri_finite3(r2.x, r2.y, r2.z)) return false;
    mn[0] = fminf(r0.x, fminf(r1.x, r2.x)), mn[1] = fminf(r0.y, fminf(r1.y, r2.y)), mn[2] = fminf(r0.z, fminf(r1.z, r2.z));
    mx[0] = fmaxf(r0.x, fmaxf(r1.x, r2.x)), mx[1] = fmaxf(r0.y, fmaxf(r1.y, r2.y)), mx[2] = fmaxf(r0.z, fmaxf(r1.z, r2.z));
    double mag = g.mag;
#pragma unroll
    for (int a = 0; a < 3; ++a) mag = fmax(mag, fmax(fabs((double)mn[a]), fabs((double)mx[a])));
    const double reach = g.reach + mag / (double)g.h * (1.0 / 262144.0);
    const double r = reach * (double)g.h;
    *lim = (float)(r * r);
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = ceil(((double)mn[a] - (double)g.lo[a]) / (double)g.h - reach);
        const double hi = floor(((double)mx[a] - (double)g.lo[a]) / (double)g.h + reach);
        c0[a] = (int)fmin(fmax(lo, 0.0), (double)g.R);  // R: past the last corner, an empty range
        c1[a] = (int)fmin(fmax(hi, -1.0), (double)(g.R - 1));
        any = any && c0[a] <= c1[a];
    }
    return any;
}
__device__ __forceinline__ long long sdf_items(const int c0[3], const int c1[3]) {
    return (long long)(c1[0] - c0[0] + 1) * ((c1[1] - c0[1]) / SDF_ROWS + 1);
}

__global__ __launch_bounds__(DIST_BLOCK) void k_sdf_init(unsigned long long* __restrict__ keys, long long n) {
    const long long i = (long long)blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (i < n) keys[i] = SDF_EMPTY;
}

__global__ __launch_bounds__(DIST_BLOCK) void k_sdf_count(const float4* __restrict__ rec, int T, SdfGrid g,
                                                          long long* __restrict__ cnt) {
    const int f = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (f >= T) return;
    int c0[3], c1[3];
    float mn[3], mx[3], lim;
    const bool any = sdf_box(rec[(size_t)f * 3], rec[(size_t)f * 3 + 1], rec[(size_t)f * 3 + 2], g, c0, c1, mn, mx, &lim);
    cnt[f] = any ? sdf_items(c0, c1) : 0ll;
}

__global__ __launch_bounds__(DIST_BLOCK) void k_sdf_scatter(const float4* __restrict__ rec, int T, SdfGrid g,
                                                            const long long* __restrict__ offs,
                                                            unsigned long long* __restrict__ keys) {
    const long long total = offs[T];
    const int R = g.R;
    for (long long item = (long long)blockIdx.x * DIST_BLOCK + threadIdx.x; item < total;
         item += (long long)gridDim.x * DIST_BLOCK) {
        int lo = 0, hi = T - 1;  // the face: the last f with offs[f] <= item
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= item) lo = mid; else hi = mid - 1;
        }
        const int f = lo;
        const float4 r0 = rec[(size_t)f * 3], r1 = rec[(size_t)f * 3 + 1], r2 = rec[(size_t)f * 3 + 2];
        int c0[3], c1[3];
        float mn[3], mx[3], lim;
        if (!sdf_box(r0, r1, r2, g, c0, c1, mn, mx, &lim)) continue;
        const float box_lim = lim * 1.001f;  // the squared distance to the triangle's BOX, with its own rounding
        const long long local = item - offs[f];
        const int nrb = (c1[1] - c0[1]) / SDF_ROWS + 1;
        const int i = c0[0] + (int)(local / nrb), jb = c0[1] + (int)(local % nrb) * SDF_ROWS;
        if (local < 0 || i > c1[0]) continue;
        const float ta[3] = {r0.x, r0.y, r0.z}, tb[3] = {r1.x, r1.y, r1.z}, tc[3] = {r2.x, r2.y, r2.z};
        float p[3];
        p[0] = sdf_corner(g.lo[0], i, g.h);
        const float bx = fmaxf(fmaxf(mn[0] - p[0], p[0] - mx[0]), 0.f);
        const int je = min(jb + SDF_ROWS - 1, c1[1]);
        for (int j = jb; j <= je; ++j) {
            p[1] = sdf_corner(g.lo[1], j, g.h);
            const float by = fmaxf(fmaxf(mn[1] - p[1], p[1] - mx[1]), 0.f);
            const float bxy = bx * bx + by * by;
            if (bxy > box_lim) continue;
            const size_t row = ((size_t)i * R + j) * R;
            for (int k = c0[2]; k <= c1[2]; ++k) {
                p[2] = sdf_corner(g.lo[2], k, g.h);
                const float bz = fmaxf(fmaxf(mn[2] - p[2], p[2] - mx[2]), 0.f);
                if (bxy + bz * bz > box_lim) continue;
                const DistHit hit = dist_closest(p, ta, tb, tc);
                if (!(hit.d2 <= lim)) continue;
                const unsigned long long key = ((unsigned long long)__float_as_uint(hit.d2) << 32) | (unsigned)f;
                unsigned long long* slot = keys + row + k;  // i, j, k in [0, R): sdf_box clamps every range
                if (key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);
            }
        }
    }
}

// the correctly rounded root, as torch's sqrt is (HIP's __fsqrt_rn is the hardware's approximation)
__device__ __forceinline__ float sdf_key_d(unsigned long long key) { return sqrtf(__uint_as_float((unsigned)(key >> 32))); }

// both streams of the compaction: the candidates
__global__ __launch_bounds__(TT_COMPACT_BLOCK) void k_sdf_flags(const unsigned long long* __restrict__ keys, TtCompact2 c) {
    const int i = blockIdx.x * TT_COMPACT_BLOCK + threadIdx.x;
    const unsigned cand = i < c.n ? (unsigned)(keys[i] != SDF_EMPTY) : 0u;
    tt_compact2_first_level<1>(c, cand, cand);
}

__global__ __launch_bounds__(DIST_BLOCK) void k_sdf_emit(const unsigned long long* __restrict__ keys, SdfGrid g,
                                                         TtCompact2 c, int n_cand, int* __restrict__ corner,
                                                         float* __restrict__ points) {
    const int i = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (i >= c.n || keys[i] == SDF_EMPTY) return;
    const int at = tt_compact2_hi(c, i);
    if (at < 0 || at >= n_cand) return;
    corner[at] = i;
    const int k = i % g.R, j = (i / g.R) % g.R, z = i / (g.R * g.R);
    points[(size_t)at * 3] = sdf_corner(g.lo[0], z, g.h);
    points[(size_t)at * 3 + 1] = sdf_corner(g.lo[1], j, g.h);
    points[(size_t)at * 3 + 2] = sdf_corner(g.lo[2], k, g.h);
}

// the query's answer replaces the scatter's key; the sign goes to level (-1 where w > 0.5, the rule of
// ops.mesh_signed_distance).  A face of -1 (a point the query refused) leaves the corner empty.
__global__ __launch_bounds__(DIST_BLOCK) void k_sdf_keys(const int* __restrict__ corner, const float* __restrict__ d2,
                                                         const int* __restrict__ face, const float* __restrict__ w,
                                                         int n_cand, int n, unsigned long long* __restrict__ keys,
                                                         float* __restrict__ level) {
    const int s = blockIdx.x * DIST_BLOCK + threadIdx.x;
    if (s >= n_cand) return;
    const int i = corner[s];
    if ((unsigned)i >= (unsigned)n) return;
    const int f = face[s];
    keys[i] = f >= 0 ? ((unsigned long long)__float_as_uint(d2[s]) << 32) | (unsigned)f : SDF_EMPTY;
    level[i] = w[s] > 0.5f ? -1.f : 1.f;
}

// One wave per (i, j) row, 64 corners of the last axis at a time: a sign corner carries its own sign (in `level`, from
// k_sdf_keys); any other corner takes the sign of the nearest sign corner below it in the row, + when there is none.
__global__ __launch_bounds__(DIST_BLOCK) void k_sdf_finish(const unsigned long long* __restrict__ keys, int R, float tau,
                                                           float sign_tau, float* __restrict__ level,
                                                           int* __restrict__ face) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (DIST_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= (long long)R * R) return;  // wave-uniform
    unsigned carry = 0;  // 1: the last sign corner so far was inside
    for (int kb = 0; kb < R; kb += 64) {
        const int k = kb + lane;
        const size_t at = (size_t)row * R + min(k, R - 1);
        const unsigned long long key = k < R ? keys[at] : SDF_EMPTY;
        const float d = sdf_key_d(key);
        const bool band = d < tau, sign = d < sign_tau;
        const bool neg = sign && level[at] < 0.f;
        const unsigned long long sm = __ballot(sign), nm = __ballot(neg);
        const unsigned long long below = sm & ((1ull << lane) - 1ull);
        unsigned inside = carry;
        if (below) inside = (unsigned)((nm >> (63 - __clzll((long long)below))) & 1ull);
        if (sign) inside = neg ? 1u : 0u;
        if (k < R) {
            level[at] = (inside ? -1.f : 1.f) * (band ? d : tau);
            face[at] = band ? (int)(unsigned)(key & 0xffffffffull) : -1;
        }
        if (sm) carry = (unsigned)((nm >> (63 - __clzll((long long)sm))) & 1ull);
    }
}

// (R, lo, h, tau, sign_tau) as a grid; false for an argument out of range or not finite
static bool sdf_grid(int32_t R, float lo_x, float lo_y, float lo_z, float h, float tau, float sign_tau, SdfGrid* out) {
    if (!(R >= 2 && R <= TT_SDFGRID_MAX_RES && tri_finite(lo_x) && tri_finite(lo_y) && tri_finite(lo_z) &&
          tri_finite(h) && h > 0.f && tri_finite(tau) && tau > 0.f && tri_finite(sign_tau) && sign_tau >= tau))
        return false;
    const double cells = (double)sign_tau / (double)h;
    if (!(cells <= TT_SDFGRID_MAX_BAND + 1.0)) return false;
    const double mag = fmax(fmax(fabs((double)lo_x), fabs((double)lo_y)), fabs((double)lo_z)) + (double)R * (double)h;
    *out = SdfGrid{{lo_x, lo_y, lo_z}, h, tau, sign_tau, cells + 0.01, mag, (int)R};
    return true;
}

extern "C" int64_t tt_sdfgrid_workspace_bytes(int32_t resolution, int32_t T) {
    if (resolution < 2 || resolution > TT_SDFGRID_MAX_RES || !tri_count_ok(T)) return TT_ERR_BAD_ARG;
    return sdf_layout(nullptr, resolution, T).bytes;
}

extern "C" int tt_sdfgrid_scatter(const float* records, int32_t T, int32_t resolution, float lo_x, float lo_y,
                                  float lo_z, float h, float tau, float sign_tau, void* workspace, int32_t* out_count,
                                  void* stream) {
    SdfGrid g;
    if (!tri_count_ok(T) || !sdf_grid(resolution, lo_x, lo_y, lo_z, h, tau, sign_tau, &g)) return TT_ERR_BAD_ARG;
    if (!records || !workspace || !out_count) return TT_ERR_BAD_ARG;
    const SdfWs w = sdf_layout(workspace, resolution, T).w;
    const long long n = (long long)resolution * resolution * resolution;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sdf_init, dim3(tt_grid(n)), dim3(DIST_BLOCK), 0, s, w.keys, n);
    hipLaunchKernelGGL(k_sdf_count, dim3(tt_grid(T)), dim3(DIST_BLOCK), 0, s, (const float4*)records, (int)T, g, w.offs);
    tt_exclusive_scan<long long>(w.offs, T, w.offs, w.xs, w.offs + T, s);
    hipLaunchKernelGGL(k_sdf_scatter, dim3(SDF_SCATTER_BLOCKS), dim3(DIST_BLOCK), 0, s, (const float4*)records, (int)T,
                       g, (const long long*)w.offs, w.keys);
    hipLaunchKernelGGL(k_sdf_flags, dim3((unsigned)w.cmp.nblk), dim3(TT_COMPACT_BLOCK), 0, s,
                       (const unsigned long long*)w.keys, w.cmp);
    tt_compact2_scan_blocks(w.cmp, (int*)out_count, s);
    return tt_check_launch();
}

extern "C" int tt_sdfgrid_corners(int32_t resolution, int32_t T, float lo_x, float lo_y, float lo_z, float h, float tau,
                                  float sign_tau, const void* workspace, int32_t n_cand, int32_t* corner,
                                  float* points, void* stream) {
    SdfGrid g;
    const long long n = (long long)resolution * resolution * resolution;
    if (!tri_count_ok(T) || !sdf_grid(resolution, lo_x, lo_y, lo_z, h, tau, sign_tau, &g) || n_cand < 0 || n_cand > n)
        return TT_ERR_BAD_ARG;
    if (n_cand == 0) return TT_OK;
    if (!workspace || !corner || !points) return TT_ERR_BAD_ARG;
    const SdfWs w = sdf_layout((void*)workspace, resolution, T).w;
    hipLaunchKernelGGL(k_sdf_emit, dim3(tt_grid(n)), dim3(DIST_BLOCK), 0, (hipStream_t)stream,
                       (const unsigned long long*)w.keys, g, w.cmp, (int)n_cand, (int*)corner, points);
    return tt_check_launch();
}

extern "C" int tt_sdfgrid_finish(int32_t resolution, int32_t T, float tau, float sign_tau, void* workspace,
                                 const int32_t* corner, const float* d2, const int32_t* nearest, const float* winding,
                                 int32_t n_cand, float* level, int32_t* face, void* stream) {
    const long long n = (long long)resolution * resolution * resolution;
    if (resolution < 2 || resolution > TT_SDFGRID_MAX_RES || !tri_count_ok(T) || !tri_finite(tau) || !(tau > 0.f) ||
        !tri_finite(sign_tau) || !(sign_tau >= tau) || n_cand < 0 || n_cand > n)
        return TT_ERR_BAD_ARG;
    if (!workspace || !level || !face || (n_cand > 0 && (!corner || !d2 || !nearest || !winding))) return TT_ERR_BAD_ARG;
    const SdfWs w = sdf_layout(workspace, resolution, T).w;
    hipStream_t s = (hipStream_t)stream;
    if (n_cand > 0)
        hipLaunchKernelGGL(k_sdf_keys, dim3(tt_grid(n_cand)), dim3(DIST_BLOCK), 0, s, (const int*)corner, d2,
                           (const int*)nearest, winding, (int)n_cand, (int)n, w.keys, level);
    const long long rows = (long long)resolution * resolution;
    hipLaunchKernelGGL(k_sdf_finish, dim3((unsigned)((rows + DIST_BLOCK / 64 - 1) / (DIST_BLOCK / 64))), dim3(DIST_BLOCK),
                       0, s, (const unsigned long long*)w.keys, (int)resolution, tau, sign_tau, level, (int*)face);
    return tt_check_launch();
}
