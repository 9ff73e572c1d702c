// tt_trigrid.h -- the one triangle grid of the mesh-query stages: the bounding cube and its cell rule, the 48-byte
// triangle record, the `order` indirection, the device view of a built grid and the host-side argument checks.  Used by
// tt_dist.hip (which builds the grid and searches it), tt_ray.hip (which walks it), tt_wind.hip (whose octree leaves
// are the cells of the cube with G = 2^L) and tt_simplify.hip (the cell rule and the checks only).  The contract is
// written in include/tt_abi.h, "point-to-mesh distance" (grid), "winding number" (tree) and "ray casting" (walk).
//
// Rule of this header: nothing in it may depend on the including file's floating-point contraction setting (tt_ray.hip
// switches contraction off, the others leave it on).  tri_cell holds a difference that feeds a product and no product
// that feeds a sum, so there is nothing in it to fuse; tri_point_cell's |p - q|^2 names its own setting.  Anything
// added here has to be of one of these two kinds.
#pragma once
#include <math.h>

#include "tt_host.h"

// The bounding cube: lo_a = min v_a, ext = the largest extent, h = ext / G, inv_h = G / ext (ext == 0: h = inv_h = 0).
// An entry point that does not take h leaves it 0.
struct TriCube {
    float lo[3], ext, h, inv_h;
    int G;
};

__device__ __forceinline__ float tri_inf() { return __int_as_float(0x7f800000); }
__device__ __forceinline__ float tri_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ bool tri_finite3(float x, float y, float z) {
    return fabsf(x) <= 3.4028235e38f && fabsf(y) <= 3.4028235e38f && fabsf(z) <= 3.4028235e38f;  // NaN: false
}

// THE cell rule: cell(x) = clamp(floor((x - lo) * inv_h), 0, G - 1), the difference and the product each rounded to
// fp32.  Monotone in x -- the ring search's bound and the ray walk's conservativeness rest on triangles, points and
// rays all going through this one function.  The clamp is taken in float, before the conversion, so that +-inf and NaN
// (an overflowing ray) land on a cell too: fmaxf(NaN, 0) = 0.
__device__ __forceinline__ int tri_cell(float x, float lo, float inv_h, int G) {
    const float c = floorf((x - lo) * inv_h);
    return (int)fminf(fmaxf(c, 0.f), (float)(G - 1));
}

// p clamped to the cube, its cell, |p - q|^2
__device__ __forceinline__ float tri_point_cell(const float p[3], const TriCube& g, int c[3]) {
#pragma clang fp contract(fast)  // the sum of squares fuses, as it always has in tt_dist.hip, whoever includes this
    float pq2 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = fminf(fmaxf(p[a], g.lo[a]), g.lo[a] + g.ext);
        c[a] = tri_cell(q, g.lo[a], g.inv_h, g.G);
        pq2 += (p[a] - q) * (p[a] - q);
    }
    return pq2;
}

// the linear key of a cell: consecutive cells along the last axis are consecutive rows
__device__ __forceinline__ int tri_key(const int c[3], int G) { return (c[0] * G + c[1]) * G + c[2]; }

// Face f of (v_pos, tri, V) as its 48-byte record: three float4 a, b, c, w unused.  The host checked the index range;
// the clamp keeps a read in bounds whatever it holds.
__device__ __forceinline__ void tri_record(const float* __restrict__ v_pos, const int* __restrict__ tri, int V, int f,
                                           float4 r[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned i = min((unsigned)tri[(size_t)f * 3 + k], (unsigned)(V - 1));
        r[k] = make_float4(v_pos[(size_t)i * 3], v_pos[(size_t)i * 3 + 1], v_pos[(size_t)i * 3 + 2], 0.f);
    }
}

// The row thread t < N serves: t, or order[t] where the host passed a permutation; -1 for an entry outside [0, N).
__device__ __forceinline__ long long tri_row(const long long* __restrict__ order, int t, int N) {
    if (!order) return t;
    const long long i = order[t];
    return (unsigned long long)i < (unsigned long long)N ? i : -1ll;
}

// A built grid as the query kernels take it, by value: records (T, 3), CSR rows (G^3 + 1), their faces (M).  The
// triangle loops stay in the kernels (dist_closest and ray_pair keep one call site each); this bounds their reads.
struct TriGridView {
    const float4* __restrict__ rec;
    const int *__restrict__ cell_ptr, *__restrict__ cell_tri;
    int T, M;
    TriCube cube;
};
// the range of cell_tri of the consecutive rows first .. last, clamped to [0, M]
__device__ __forceinline__ void tri_rows(const TriGridView& v, int first, int last, int& kb, int& ke) {
    kb = max(v.cell_ptr[first], 0);
    ke = min(v.cell_ptr[last + 1], v.M);
}
__device__ __forceinline__ bool tri_face_ok(const TriGridView& v, int f) { return (unsigned)f < (unsigned)v.T; }

// ---- host side: the checks the entry points of the four files make before any HIP call ----
static inline bool tri_finite(double x) { return x >= -1e300 && x <= 1e300; }
static inline bool tri_count_ok(int32_t n) { return n >= 1 && n <= TT_MESH_MAX_ITEMS; }  // vertices, faces of a mesh
static inline bool tri_mesh_ok(int32_t V, int32_t T) { return tri_count_ok(V) && tri_count_ok(T); }
static inline bool tri_items_ok(int32_t n) { return n >= 0 && n <= TT_MESH_MAX_ITEMS; }  // points, rays: 0 does nothing

// (G, lo, ext, h, inv_h) as a cube, G in [1, max_G]; false for an argument out of range or not finite.  ext = 0 (a mesh
// without extent) is a grid whose every point and triangle lands in cell 0: h = inv_h = 0.
static inline bool tri_cube(int32_t G, int32_t max_G, float lo_x, float lo_y, float lo_z, float ext, float h,
                            float inv_h, TriCube* out) {
    if (!(G >= 1 && G <= max_G && tri_finite(lo_x) && tri_finite(lo_y) && tri_finite(lo_z) && tri_finite(ext) &&
          tri_finite(h) && tri_finite(inv_h) && ext >= 0.f && h >= 0.f && inv_h >= 0.f))
        return false;
    *out = TriCube{{lo_x, lo_y, lo_z}, ext, h, inv_h, (int)G};
    return true;
}

// the same for a built grid that serves N items: N, T, M and the cube in range; with N > 0 the three tables are there
static inline bool tri_view(int32_t N, const float* records, const int32_t* cell_ptr, const int32_t* cell_tri, int32_t T,
                            int32_t M, int32_t G, float lo_x, float lo_y, float lo_z, float ext, float h, float inv_h,
                            TriGridView* out) {
    TriCube cube;
    if (!tri_items_ok(N) || !tri_count_ok(T) || M < 1 ||
        !tri_cube(G, TT_DIST_MAX_GRID, lo_x, lo_y, lo_z, ext, h, inv_h, &cube))
        return false;
    if (N > 0 && (!records || !cell_ptr || !cell_tri)) return false;
    *out = TriGridView{(const float4*)records, (const int*)cell_ptr, (const int*)cell_tri, (int)T, (int)M, cube};
    return true;
}
