// tt_ray.hip -- ray casting against a triangle mesh over the distance grid (exact, watertight, deterministic) and the
// ambient-occlusion count built on it.  The contract (pair, answer, walk and its constants, entry points) is written in
// include/tt_abi.h, "ray casting".
//   k_ray_cast     one thread per ray: closest hit, the lexicographic minimum of (t, face) over ALL triangles
//   k_ray_any      one thread per ray: the same walk, left at the first accepted pair
//   k_ray_ao_init  one thread per point: hits = 0, or -1 for a point / normal that cannot be used
//   k_ray_ao       one thread per (point, direction): the any-hit walk; the hits of a point are counted by integer atomics
// ray_pair is the only place a (ray, triangle) pair is evaluated and ray_walk holds its only call; the three kernels
// instantiate that one walk.  Every product and difference of the pair is rounded on its own: a contracted a*b - c*d is
// not antisymmetric, and the two triangles of an edge must see the same magnitude.  __fmul_rn / __fsub_rn do not see to
// that: they are plain operators in a header compiled with contraction allowed, which the compiler fuses after
// inlining, and differently in each kernel.  So contraction is switched off for this whole file and the operations whose
// order the contract names go through ray_mul / ray_sub / ray_add below, compiled under that setting.  The grid itself
// (the cube, its cell rule, the view of the tables, the `order` lookup, the argument checks) is tt_trigrid.h, the one
// the triangles were binned with; nothing there depends on this file's contraction setting.
#include <math.h>

#include "tt_trigrid.h"

#pragma clang fp contract(off)
__device__ __forceinline__ float ray_mul(float x, float y) { return x * y; }
__device__ __forceinline__ float ray_sub(float x, float y) { return x - y; }
__device__ __forceinline__ float ray_add(float x, float y) { return x + y; }

#define RAY_BLOCK TT_ITEM_BLOCK
#define RAY_REL 1.52587890625e-05f  // 2^-16: relative dilation of a slice's interval, and tol / scale
#define RAY_FLT_MIN 1.17549435e-38f
#define RAY_FLT_MAX 3.4028235e38f

// component k of (x, y, z) by selects: a register array indexed at run time would live in scratch
__device__ __forceinline__ float ray_sel(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }
// argmax |d|, the lowest index at equal magnitude
__device__ __forceinline__ int ray_major(float dx, float dy, float dz) {
    int k = 0;
    float m = fabsf(dx);
    if (fabsf(dy) > m) {
        k = 1;
        m = fabsf(dy);
    }
    if (fabsf(dz) > m) k = 2;
    return k;
}
// a ray the kernels serve: finite, and a direction whose largest component is a normal fp32 number (1 / d is finite)
__device__ __forceinline__ bool ray_usable(float ox, float oy, float oz, float dx, float dy, float dz) {
    return tri_finite3(ox, oy, oz) && tri_finite3(dx, dy, dz) &&
           fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz))) >= RAY_FLT_MIN;
}

// ---------------------------------------------------------------------------------------------------------------
// the pair: watertight ray / triangle test (Woop, Benthin, Wald, JCGT 2013)
// ---------------------------------------------------------------------------------------------------------------
struct RayFrame {
    int kx, ky, kz;
    float Sx, Sy, Sz;
};
__device__ __forceinline__ RayFrame ray_frame(float dx, float dy, float dz) {
    RayFrame fr;
    fr.kz = ray_major(dx, dy, dz);
    fr.kx = fr.kz == 2 ? 0 : fr.kz + 1;
    fr.ky = fr.kx == 2 ? 0 : fr.kx + 1;
    const float dz_ = ray_sel(dx, dy, dz, fr.kz);
    if (dz_ < 0.f) {
        const int s = fr.kx;
        fr.kx = fr.ky;
        fr.ky = s;
    }
    fr.Sx = __fdiv_rn(ray_sel(dx, dy, dz, fr.kx), dz_);
    fr.Sy = __fdiv_rn(ray_sel(dx, dy, dz, fr.ky), dz_);
    fr.Sz = __fdiv_rn(1.f, dz_);
    return fr;
}

struct RayHit {
    float t, b0, b1, b2;
};

// true for a hit with 0 <= t <= t_max.  Never NaN in `hit` when it returns true; false for every NaN on the way.
__device__ __forceinline__ bool ray_pair(const RayFrame& fr, float ox, float oy, float oz, const float4 a,
                                         const float4 b, const float4 c, float t_max, RayHit& hit) {
    const float a0 = ray_sub(a.x, ox), a1 = ray_sub(a.y, oy), a2 = ray_sub(a.z, oz);
    const float b0 = ray_sub(b.x, ox), b1 = ray_sub(b.y, oy), b2 = ray_sub(b.z, oz);
    const float c0 = ray_sub(c.x, ox), c1 = ray_sub(c.y, oy), c2 = ray_sub(c.z, oz);
    const float Az = ray_sel(a0, a1, a2, fr.kz), Bz = ray_sel(b0, b1, b2, fr.kz), Cz = ray_sel(c0, c1, c2, fr.kz);
    const float Ax = ray_sub(ray_sel(a0, a1, a2, fr.kx), ray_mul(fr.Sx, Az));
    const float Ay = ray_sub(ray_sel(a0, a1, a2, fr.ky), ray_mul(fr.Sy, Az));
    const float Bx = ray_sub(ray_sel(b0, b1, b2, fr.kx), ray_mul(fr.Sx, Bz));
    const float By = ray_sub(ray_sel(b0, b1, b2, fr.ky), ray_mul(fr.Sy, Bz));
    const float Cx = ray_sub(ray_sel(c0, c1, c2, fr.kx), ray_mul(fr.Sx, Cz));
    const float Cy = ray_sub(ray_sel(c0, c1, c2, fr.ky), ray_mul(fr.Sy, Cz));
    float U = ray_sub(ray_mul(Cx, By), ray_mul(Cy, Bx));
    float V = ray_sub(ray_mul(Ax, Cy), ray_mul(Ay, Cx));
    float W = ray_sub(ray_mul(Bx, Ay), ray_mul(By, Ax));
    if (U == 0.f || V == 0.f || W == 0.f) {
        // on an edge or a vertex to fp32: the same operands in double (the products are exact there), rounded once
        U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
        V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
        W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
    }
    if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) return false;
    const float det = ray_add(ray_add(U, V), W);
    if (det == 0.f || !(fabsf(det) <= RAY_FLT_MAX)) return false;  // in the plane, no area; overflow and NaN
    const float num = ray_add(ray_add(ray_mul(U, ray_mul(fr.Sz, Az)), ray_mul(V, ray_mul(fr.Sz, Bz))),
                                ray_mul(W, ray_mul(fr.Sz, Cz)));
    const float t = __fdiv_rn(num, det);
    if (!(t >= 0.f && t <= t_max)) return false;  // NaN: a miss
    {
        // Rare path, an accepted pair only: a face whose edge vectors b - a and c - a (fp32) are exactly parallel has no
        // area; det is rounding noise there and would let a ray that passes within rounding of its line hit it.  The
        // products are exact in double, so this is an exact test of the fp32 edge vectors.
        const double px = (double)ray_sub(b.x, a.x), py = (double)ray_sub(b.y, a.y), pz = (double)ray_sub(b.z, a.z);
        const double qx = (double)ray_sub(c.x, a.x), qy = (double)ray_sub(c.y, a.y), qz = (double)ray_sub(c.z, a.z);
        if (py * qz == pz * qy && pz * qx == px * qz && px * qy == py * qx) return false;
    }
    hit.t = t;
    hit.b0 = __fdiv_rn(U, det);
    hit.b1 = __fdiv_rn(V, det);
    hit.b2 = __fdiv_rn(W, det);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// the walk: slices of cells along the dominant axis
// ---------------------------------------------------------------------------------------------------------------
// The grid's cell() is tri_cell (tt_trigrid.h), the function the triangles were binned with: monotone in x, and defined
// for +-inf and NaN (an overflowing ray), which land on a cell too.
// x - (2^-16 |x| + pad) and x + (...).  inf - inf is NaN here and stays: every use is an fmaxf / fminf, which drops it,
// or a compare, which is false -- both read it as "open", -inf below and +inf above (and no select on a NaN test joined
// with another condition is formed: tools/mask_hazard_lint.py)
__device__ __forceinline__ float ray_below(float x, float pad) { return x - (fabsf(x) * RAY_REL + pad); }
__device__ __forceinline__ float ray_above(float x, float pad) { return x + (fabsf(x) * RAY_REL + pad); }

struct RayBest {
    float t, b0, b1, b2;
    int f;
};

// ANY: return at the first accepted pair.  Else best = the lexicographic minimum of (t, f).  Returns "some pair hit".
template <bool ANY>
__device__ __forceinline__ bool ray_walk(float ox, float oy, float oz, float dx, float dy, float dz, float t_max,
                                         const TriGridView& grid, RayBest& best) {
    const RayFrame fr = ray_frame(dx, dy, dz);
    const TriCube& g = grid.cube;
    const int G = g.G;
    const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    // tol = 2^-16 (ext + max |o - centre| + max |centre|)
    float so = 0.f, sc = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float cen = g.lo[a] + 0.5f * g.ext;
        so = fmaxf(so, fabsf(o[a] - cen));
        sc = fmaxf(sc, fabsf(cen));
    }
    const float tol = RAY_REL * (g.ext + so + sc);
    // the ray's span inside the cube dilated by tol, clipped to [0, t_max]
    float t_lo = 0.f, t_hi = t_max;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p0 = g.lo[a] - tol, p1 = (g.lo[a] + g.ext) + tol;
        if (d[a] == 0.f) {
            if (o[a] < p0 || o[a] > p1) return false;
        } else {
            const float t0 = __fdiv_rn(p0 - o[a], d[a]), t1 = __fdiv_rn(p1 - o[a], d[a]);
            t_lo = fmaxf(t_lo, ray_below(fminf(t0, t1), 0.f));  // fmaxf / fminf drop a NaN
            t_hi = fminf(t_hi, ray_above(fmaxf(t0, t1), 0.f));
        }
    }
    if (!(t_lo <= t_hi)) return false;
    const int ka = fr.kz;                               // the dominant axis
    const int ku = ka == 0 ? 1 : 0, kv = ka == 2 ? 1 : 2;  // the lateral axes, ku < kv
    const int sa = ka == 0 ? G * G : (ka == 1 ? G : 1), su = ku == 0 ? G * G : G, sv = kv == 1 ? G : 1;
    const float oa = ray_sel(ox, oy, oz, ka), da = ray_sel(dx, dy, dz, ka), la = ray_sel(g.lo[0], g.lo[1], g.lo[2], ka);
    const float ou = ray_sel(ox, oy, oz, ku), du = ray_sel(dx, dy, dz, ku), lu = ray_sel(g.lo[0], g.lo[1], g.lo[2], ku);
    const float ov = ray_sel(ox, oy, oz, kv), dv = ray_sel(dx, dy, dz, kv), lv = ray_sel(g.lo[0], g.lo[1], g.lo[2], kv);
    const float tol_t = __fdiv_rn(tol, fabsf(da));
    const bool up = da > 0.f;
    const bool row = sv == 1;  // consecutive cells along kv are consecutive CSR rows: one range of cell_tri
    bool any = false;
    for (int j = 0; j < G; ++j) {
        const int k = up ? j : G - 1 - j;
        const float q0 = la + (float)k * g.h, q1 = la + (float)(k + 1) * g.h;
        const float tq0 = __fdiv_rn(q0 - oa, da), tq1 = __fdiv_rn(q1 - oa, da);
        float s = ray_below(up ? tq0 : tq1, tol_t), e = ray_above(up ? tq1 : tq0, tol_t);
        if (j == 0) s = -tri_inf();
        if (j == G - 1) e = tri_inf();
        if (s > t_hi) break;  // s does not decrease with j: every later slice is empty as well
        const float t0 = fmaxf(s, t_lo), t1 = fminf(e, t_hi);
        if (t0 <= t1) {
            const float xu0 = du == 0.f ? ou : ou + t0 * du, xu1 = du == 0.f ? ou : ou + t1 * du;
            const float xv0 = dv == 0.f ? ov : ov + t0 * dv, xv1 = dv == 0.f ? ov : ov + t1 * dv;
            const int u0 = tri_cell(fminf(xu0, xu1) - tol, lu, g.inv_h, G);
            const int u1 = max(u0, tri_cell(fmaxf(xu0, xu1) + tol, lu, g.inv_h, G));
            const int v0 = tri_cell(fminf(xv0, xv1) - tol, lv, g.inv_h, G);
            const int v1 = max(v0, tri_cell(fmaxf(xv0, xv1) + tol, lv, g.inv_h, G));
            for (int iu = u0; iu <= u1; ++iu) {
                for (int iv = v0; iv <= v1; iv = row ? v1 + 1 : iv + 1) {
                    const int c_first = k * sa + iu * su + iv * sv;  // all three coordinates are in [0, G)
                    const int c_last = row ? c_first + (v1 - v0) : c_first;
                    int pb, pe;
                    tri_rows(grid, c_first, c_last, pb, pe);
                    for (int p = pb; p < pe; ++p) {
                        const int f = grid.cell_tri[p];
                        if (!tri_face_ok(grid, f)) continue;
                        RayHit hit;
                        if (!ray_pair(fr, ox, oy, oz, grid.rec[(size_t)f * 3], grid.rec[(size_t)f * 3 + 1],
                                      grid.rec[(size_t)f * 3 + 2], t_max, hit))
                            continue;
                        if (ANY) return true;
                        any = true;
                        bool better = hit.t < best.t;
                        if (hit.t == best.t) better = f < best.f;
                        if (better) {
                            best.t = hit.t;
                            best.b0 = hit.b0;
                            best.b1 = hit.b1;
                            best.b2 = hit.b2;
                            best.f = f;
                        }
                    }
                }
            }
        }
        // every pair not yet met has its t in a later slice's interval, at or above that slice's start >= s: strictly
        // below s nothing unseen can win or tie
        if (!ANY && best.t < s) break;
    }
    return any;
}

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RAY_BLOCK) void k_ray_cast(const float* __restrict__ origins,
                                                        const float* __restrict__ dirs,
                                                        const long long* __restrict__ order, int N, float t_max,
                                                        TriGridView grid, float* __restrict__ out_t,
                                                        int* __restrict__ out_face, float* __restrict__ out_bary) {
    const int th = blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (th >= N) return;
    const long long i = tri_row(order, th, N);
    if (i < 0) return;
    const float ox = origins[(size_t)i * 3], oy = origins[(size_t)i * 3 + 1], oz = origins[(size_t)i * 3 + 2];
    const float dx = dirs[(size_t)i * 3], dy = dirs[(size_t)i * 3 + 1], dz = dirs[(size_t)i * 3 + 2];
    RayBest best{tri_inf(), 0.f, 0.f, 0.f, 0x7fffffff};
    if (!ray_usable(ox, oy, oz, dx, dy, dz)) {  // before the walk: no loop depends on such a row
        best.t = tri_nan();
    } else {
        ray_walk<false>(ox, oy, oz, dx, dy, dz, t_max, grid, best);
    }
    out_t[i] = best.t;
    out_face[i] = best.f == 0x7fffffff ? -1 : best.f;
    out_bary[(size_t)i * 3] = best.b0;
    out_bary[(size_t)i * 3 + 1] = best.b1;
    out_bary[(size_t)i * 3 + 2] = best.b2;
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_any(const float* __restrict__ origins,
                                                       const float* __restrict__ dirs,
                                                       const long long* __restrict__ order, int N, float t_max,
                                                       TriGridView grid, unsigned char* __restrict__ out_hit) {
    const int th = blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (th >= N) return;
    const long long i = tri_row(order, th, N);
    if (i < 0) return;
    const float ox = origins[(size_t)i * 3], oy = origins[(size_t)i * 3 + 1], oz = origins[(size_t)i * 3 + 2];
    const float dx = dirs[(size_t)i * 3], dy = dirs[(size_t)i * 3 + 1], dz = dirs[(size_t)i * 3 + 2];
    RayBest best{tri_inf(), 0.f, 0.f, 0.f, 0x7fffffff};
    bool hit = false;
    if (ray_usable(ox, oy, oz, dx, dy, dz))
        hit = ray_walk<true>(ox, oy, oz, dx, dy, dz, t_max, grid, best);
    out_hit[i] = hit ? 1 : 0;
}

// The unit normal of a point the AO kernels can use: scaled by its largest component first, so that any non-zero
// finite length works; every operation rounded on its own (a host restatement in fp32 gives the same bits).
__device__ __forceinline__ bool ray_ao_normal(const float* __restrict__ points, const float* __restrict__ normals,
                                              long long i, float p[3], float n[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = points[(size_t)i * 3 + a];
        n[a] = normals[(size_t)i * 3 + a];
    }
    const float m = fmaxf(fabsf(n[0]), fmaxf(fabsf(n[1]), fabsf(n[2])));
    // one compare decides: 0 * x is NaN for an x that is not finite and 0 otherwise, so q is m, or NaN
    const float q = m + ((0.f * p[0] + 0.f * p[1] + 0.f * p[2]) + (0.f * n[0] + 0.f * n[1] + 0.f * n[2]));
    if (!(q > 0.f)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = __fdiv_rn(n[a], m);
    const float len = __fsqrt_rn(ray_add(ray_add(ray_mul(n[0], n[0]), ray_mul(n[1], n[1])), ray_mul(n[2], n[2])));
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = __fdiv_rn(n[a], len);  // len >= 1
    return true;
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_ao_init(const float* __restrict__ points,
                                                           const float* __restrict__ normals, int N,
                                                           int* __restrict__ hits) {
    const int i = blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (i >= N) return;
    float p[3], n[3];
    hits[i] = ray_ao_normal(points, normals, i, p, n) ? 0 : -1;
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_ao(const float* __restrict__ points,
                                                      const float* __restrict__ normals,
                                                      const float* __restrict__ dirs_local, int N, int K, float bias,
                                                      float max_distance, TriGridView grid, int* __restrict__ hits) {
    const long long r = (long long)blockIdx.x * RAY_BLOCK + threadIdx.x;  // ray r = (point r / K, direction r % K)
    if (r >= (long long)N * K) return;
    const long long i = r / K;
    const int k = (int)(r - i * K);
    float p[3], n[3];
    if (!ray_ao_normal(points, normals, i, p, n)) return;  // hits[i] = -1 stands
    // Duff et al. 2017, "Building an Orthonormal Basis, Revisited": branch-free (T, B) about n
    const float sg = copysignf(1.f, n[2]);
    const float a = __fdiv_rn(-1.f, ray_add(sg, n[2]));
    const float b = ray_mul(ray_mul(n[0], n[1]), a);
    const float tx = ray_add(1.f, ray_mul(ray_mul(ray_mul(sg, n[0]), n[0]), a));
    const float ty = ray_mul(sg, b), tz = ray_mul(-sg, n[0]);
    const float bx = b, by = ray_add(sg, ray_mul(ray_mul(n[1], n[1]), a)), bz = -n[1];
    const float x = dirs_local[(size_t)k * 3], y = dirs_local[(size_t)k * 3 + 1], z = dirs_local[(size_t)k * 3 + 2];
    const float dx = ray_add(ray_add(ray_mul(x, tx), ray_mul(y, bx)), ray_mul(z, n[0]));
    const float dy = ray_add(ray_add(ray_mul(x, ty), ray_mul(y, by)), ray_mul(z, n[1]));
    const float dz = ray_add(ray_add(ray_mul(x, tz), ray_mul(y, bz)), ray_mul(z, n[2]));
    const float ox = ray_add(p[0], ray_mul(bias, n[0])), oy = ray_add(p[1], ray_mul(bias, n[1])),
                oz = ray_add(p[2], ray_mul(bias, n[2]));
    RayBest best{tri_inf(), 0.f, 0.f, 0.f, 0x7fffffff};
    if (!ray_usable(ox, oy, oz, dx, dy, dz)) return;  // such a ray hits nothing
    if (ray_walk<true>(ox, oy, oz, dx, dy, dz, max_distance, grid, best))
        atomicAdd(hits + i, 1);  // an integer count: the order of arrival cannot show
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
extern "C" int tt_ray_cast(const float* origins, const float* dirs, const int64_t* order, int32_t N, float t_max,
                           const float* records, const int32_t* cell_ptr, const int32_t* cell_tri, int32_t T, int32_t M,
                           int32_t grid, float lo_x, float lo_y, float lo_z, float ext, float h, float inv_h, float* t,
                           int32_t* face, float* bary, void* stream) {
    TriGridView g;
    if (!tri_view(N, records, cell_ptr, cell_tri, T, M, grid, lo_x, lo_y, lo_z, ext, h, inv_h, &g) || !(t_max >= 0.f))
        return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!origins || !dirs || !t || !face || !bary) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_ray_cast, dim3(tt_grid(N)), dim3(RAY_BLOCK), 0, (hipStream_t)stream, origins, dirs,
                       (const long long*)order, (int)N, t_max, g, t, (int*)face, bary);
    return tt_check_launch();
}

extern "C" int tt_ray_any(const float* origins, const float* dirs, const int64_t* order, int32_t N, float t_max,
                          const float* records, const int32_t* cell_ptr, const int32_t* cell_tri, int32_t T, int32_t M,
                          int32_t grid, float lo_x, float lo_y, float lo_z, float ext, float h, float inv_h,
                          uint8_t* hit, void* stream) {
    TriGridView g;
    if (!tri_view(N, records, cell_ptr, cell_tri, T, M, grid, lo_x, lo_y, lo_z, ext, h, inv_h, &g) || !(t_max >= 0.f))
        return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!origins || !dirs || !hit) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_ray_any, dim3(tt_grid(N)), dim3(RAY_BLOCK), 0, (hipStream_t)stream, origins, dirs,
                       (const long long*)order, (int)N, t_max, g, (unsigned char*)hit);
    return tt_check_launch();
}

extern "C" int tt_ray_ao(const float* points, const float* normals, const float* dirs_local, int32_t N, int32_t K,
                         float bias, float max_distance, const float* records, const int32_t* cell_ptr,
                         const int32_t* cell_tri, int32_t T, int32_t M, int32_t grid, float lo_x, float lo_y,
                         float lo_z, float ext, float h, float inv_h, int32_t* hits, void* stream) {
    TriGridView g;
    if (!tri_view(N, records, cell_ptr, cell_tri, T, M, grid, lo_x, lo_y, lo_z, ext, h, inv_h, &g) || K < 1 ||
        K > TT_RAY_MAX_DIRS || !tri_finite(bias) || !(max_distance >= 0.f))
        return TT_ERR_BAD_ARG;
    if (N == 0) return TT_OK;
    if (!points || !normals || !dirs_local || !hits) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ray_ao_init, dim3(tt_grid(N)), dim3(RAY_BLOCK), 0, s, points, normals, (int)N, (int*)hits);
    hipLaunchKernelGGL(k_ray_ao, dim3(tt_grid((long long)N * K)), dim3(RAY_BLOCK), 0, s, points, normals, dirs_local,
                       (int)N, (int)K, bias, max_distance, g, (int*)hits);
    return tt_check_launch();
}
