// tt_bake.hip -- vertex tangents and the tangent-space normal-map bake of the mesh exporter.  The contract (per-face
// tangent, groups, the degenerate rule, the projection step, the encode, determinism) is written in include/tt_abi.h,
// "tangents and normal-map baking".  The group -> corner CSR is one stable torch sort on the host side
// (ops.mesh_tangents); the field queries between the projection steps are tt_query_points; everything else is here:
//   k_bake_tangents   one thread per group: the per-face tangents of its corners added in ascending corner id,
//                     normalised, Gram-Schmidt against the group's normal, the fixed perpendicular where that fails
//   k_bake_project    one thread per point: one bounded Newton step towards the iso-surface
//   k_bake_encode     one thread per texel: interpolated (t, b, n) frame, the field normal written in it
// No float atomics (the back-facing count is an integer atomic); identical inputs give bit-identical outputs.
#include "tt_host.h"

// every product and sum below is rounded on its own, in the order written (tt_abi.h states the expressions)
#pragma clang fp contract(off)

#define BAKE_BLOCK TT_ITEM_BLOCK
#define BAKE_TINY_SQ 1e-20f  // a sum of tangents this short (squared) has no direction
#define BAKE_PERP_SQ 1e-12f  // a unit tangent this close (squared) to the normal's line is parallel to it

__device__ __forceinline__ float bake_dot(const float a[3], const float b[3]) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// x > lim for a finite x, false for NaN and +-inf, as ONE compare: x - x is 0 for a finite x and NaN otherwise.  The
// kernels below select on single compares only and chain conditions through the values they select, never through a
// scalar-ALU combination of compare masks (tools/mask_hazard_lint.py).
__device__ __forceinline__ bool bake_above(float x, float lim) { return x + (x - x) > lim; }

// 0 iff every index of idx is below n (n >= 1): unsigned max and a saturating difference, no compare
__device__ __forceinline__ unsigned bake_over(const unsigned idx[3], int n) {
    const unsigned m = max(max(idx[0], idx[1]), idx[2]);
    return m - min(m, (unsigned)n - 1u);
}

// the fixed unit vector perpendicular to unit n: e_a - (e_a . n) n normalised, a the first axis of smallest |n_a|
__device__ __forceinline__ void bake_perp(const float n[3], float out[3]) {
    const float ax = fabsf(n[0]), ay = fabsf(n[1]), az = fabsf(n[2]);
    const float sy = ay < ax ? 1.f : 0.f;
    const bool sz = az < fminf(ax, ay);
    const float e[3] = {sz ? 0.f : 1.f - sy, sz ? 0.f : sy, sz ? 1.f : 0.f};
    const float na = bake_dot(e, n);  // one term is n_a, the others are zeros
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = e[c] - na * n[c];
    const float rr = bake_dot(r, r);
    // |r|^2 = 1 - n_a^2 >= 2/3 for a unit n; a normal that is not unit or not finite gives +x
    const bool ok = bake_above(rr, 0.25f);
    const float inv = 1.f / sqrtf(ok ? rr : 1.f);
    out[0] = ok ? r[0] * inv : 1.f;
    out[1] = ok ? r[1] * inv : 0.f;
    out[2] = ok ? r[2] * inv : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// tangents
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BAKE_BLOCK) void k_bake_tangents(const float* __restrict__ v_pos,
                                                              const int* __restrict__ t_pos_idx,
                                                              const float* __restrict__ v_tex,
                                                              const int* __restrict__ t_tex_idx,
                                                              const float* __restrict__ v_nrm,
                                                              const int* __restrict__ grp_ptr,
                                                              const int* __restrict__ grp_corner, int V, int Vt, int T,
                                                              int G, int by_tex, float* __restrict__ out) {
    const int g = blockIdx.x * BAKE_BLOCK + threadIdx.x;
    if (g >= G) return;
    const int cb = min(max(grp_ptr[g], 0), 3 * T), ce = min(max(grp_ptr[g + 1], cb), 3 * T);
    float s[3] = {0.f, 0.f, 0.f};
    int nv = by_tex ? -1 : g;  // the position vertex whose normal the group takes
    for (int i = cb; i < ce; ++i) {
        const unsigned c = (unsigned)grp_corner[i];
        if (c >= 3u * (unsigned)T) continue;
        const unsigned f = c / 3u, k = c - 3u * f;
        unsigned ip[3], it[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            ip[j] = (unsigned)t_pos_idx[(size_t)f * 3 + j];
            it[j] = (unsigned)t_tex_idx[(size_t)f * 3 + j];
        }
        if (bake_over(ip, V) | bake_over(it, Vt)) continue;
        if (by_tex && nv < 0) nv = (int)(k == 0 ? ip[0] : (k == 1 ? ip[1] : ip[2]));
        float pe1[3], pe2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p0 = v_pos[(size_t)ip[0] * 3 + a];
            pe1[a] = v_pos[(size_t)ip[1] * 3 + a] - p0;
            pe2[a] = v_pos[(size_t)ip[2] * 3 + a] - p0;
        }
        const float u0 = v_tex[(size_t)it[0] * 2], w0 = v_tex[(size_t)it[0] * 2 + 1];
        const float e1x = v_tex[(size_t)it[1] * 2] - u0, e1y = v_tex[(size_t)it[1] * 2 + 1] - w0;
        const float e2x = v_tex[(size_t)it[2] * 2] - u0, e2y = v_tex[(size_t)it[2] * 2 + 1] - w0;
        const float denom = __fsub_rn(__fmul_rn(e1x, e2y), __fmul_rn(e1y, e2x));
        const float d = denom > 0.f ? fmaxf(denom, 1e-6f) : fminf(denom, -1e-6f);
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] += (pe1[a] * e2y - pe2[a] * e1y) / d;
    }
    float n[3] = {0.f, 0.f, 1.f};
    if (nv >= 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) n[a] = v_nrm[(size_t)nv * 3 + a];
    }
    float fb[3];
    bake_perp(n, fb);
    const float ss = bake_dot(s, s);  // 0 without a contributing corner
    const bool has = bake_above(ss, BAKE_TINY_SQ);
    const float inv = 1.f / sqrtf(has ? ss : 1.f);
    float t[3], r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = s[a] * inv;
    const float tn = bake_dot(t, n);
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] = t[a] - tn * n[a];
    const float rr = has ? bake_dot(r, r) : 0.f;
    const bool ok = bake_above(rr, BAKE_PERP_SQ);
    const float rinv = 1.f / sqrtf(ok ? rr : 1.f);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[(size_t)g * 3 + a] = ok ? r[a] * rinv : fb[a];
}

// ---------------------------------------------------------------------------------------------------------------
// projection step
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BAKE_BLOCK) void k_bake_project(float* __restrict__ points, const float* __restrict__ sdf,
                                                             const float* __restrict__ sdf_grad,
                                                             const unsigned char* __restrict__ mask, long long M,
                                                             float max_step) {
    const long long i = (long long)blockIdx.x * BAKE_BLOCK + threadIdx.x;
    if (i >= M) return;
    if (mask && !mask[i]) return;
    const float g[3] = {sdf_grad[i * 3], sdf_grad[i * 3 + 1], sdf_grad[i * 3 + 2]};
    const float gg = bake_dot(g, g);
    if (!bake_above(fabsf(sdf[i]) + gg, -1.f)) return;  // a sdf or gradient that is not finite moves nothing
    const float a = fminf(fmaxf(sdf[i] / fmaxf(gg, 1e-12f), -1.f), 1.f);
    const float len = fabsf(a) * sqrtf(gg);
    const float c = len > max_step ? a * (max_step / len) : a;
#pragma unroll
    for (int k = 0; k < 3; ++k) points[i * 3 + k] -= c * g[k];
}

// ---------------------------------------------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bake_interp3(const float* __restrict__ attr, const unsigned idx[3], float u, float v,
                                             float w2, float out[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out[a] = (u * attr[(size_t)idx[0] * 3 + a] + v * attr[(size_t)idx[1] * 3 + a]) + w2 * attr[(size_t)idx[2] * 3 + a];
}

__device__ __forceinline__ void bake_unit(const float x[3], const float fb[3], float out[3]) {
    const float xx = bake_dot(x, x);
    const bool ok = bake_above(xx, BAKE_TINY_SQ);
    const float inv = 1.f / sqrtf(ok ? xx : 1.f);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = ok ? x[a] * inv : fb[a];
}

__global__ __launch_bounds__(BAKE_BLOCK) void k_bake_encode(const float* __restrict__ rast,
                                                            const float* __restrict__ v_nrm,
                                                            const int* __restrict__ t_pos_idx,
                                                            const float* __restrict__ tng_tex,
                                                            const int* __restrict__ t_tex_idx,
                                                            const float* __restrict__ field_nrm, int V, int Vt, int T,
                                                            long long n_texels, float* __restrict__ out,
                                                            int* __restrict__ out_counts) {
    const long long p = (long long)blockIdx.x * BAKE_BLOCK + threadIdx.x;
    unsigned covered = 0, back = 0;
    if (p < n_texels) {
        const float4 r = reinterpret_cast<const float4*>(rast)[p];
        // id channel: face + 1, 0 = uncovered; anything that is not a valid id is uncovered (as interpolate reads it)
        const int t = (int)fminf(fmaxf(r.w, 0.f), 33554432.f) - 1;
        unsigned ip[3] = {0u, 0u, 0u}, it[3] = {0u, 0u, 0u}, bad = 1;
        if ((unsigned)t < (unsigned)T) {  // t = -1 wraps above every T
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ip[j] = (unsigned)t_pos_idx[(size_t)t * 3 + j];
                it[j] = (unsigned)t_tex_idx[(size_t)t * 3 + j];
            }
            bad = bake_over(ip, V) | bake_over(it, Vt);
        }
        float o[3] = {0.5f, 0.5f, 1.f};
        if (!bad) {
            covered = 1;
            const float w2 = 1.f - r.x - r.y;
            float n[3], tg[3], nh[3], th[3], q[3], fb[3];
            bake_interp3(v_nrm, ip, r.x, r.y, w2, n);
            bake_interp3(tng_tex, it, r.x, r.y, w2, tg);
            const float z[3] = {0.f, 0.f, 1.f};
            bake_unit(n, z, nh);
            const float tn = bake_dot(tg, nh);
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = tg[a] - tn * nh[a];
            bake_perp(nh, fb);
            bake_unit(q, fb, th);
            const float bh[3] = {th[1] * nh[2] - th[2] * nh[1], th[2] * nh[0] - th[0] * nh[2],
                                 th[0] * nh[1] - th[1] * nh[0]};
            float m[3], mh[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) m[a] = field_nrm[p * 3 + a];
            bake_unit(m, nh, mh);
            const float mn = bake_dot(mh, nh);
            o[0] = 0.5f + 0.5f * bake_dot(mh, th);
            o[1] = 0.5f + 0.5f * bake_dot(mh, bh);
            o[2] = 0.5f + 0.5f * mn;
            back = (unsigned)!(mn > 0.f);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) out[p * 3 + a] = o[a];
    }
    // (covered, back-facing) texels: one integer atomic pair per wave that has any
    const unsigned long long bc = __ballot(covered), bb = __ballot(back);
    if ((threadIdx.x & 63) == 0) {
        if (bc) atomicAdd(out_counts, __popcll(bc));
        if (bb) atomicAdd(out_counts + 1, __popcll(bb));
    }
}

__global__ void k_bake_zero_counts(int* __restrict__ out_counts) {
    if (threadIdx.x < 2) out_counts[threadIdx.x] = 0;
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
extern "C" int tt_bake_tangents(const float* v_pos, const int32_t* t_pos_idx, const float* v_tex,
                                const int32_t* t_tex_idx, const float* v_nrm, const int32_t* group_ptr,
                                const int32_t* group_corner, int32_t V, int32_t Vt, int32_t T, int32_t group,
                                float* out, void* stream) {
    if (group != TT_BAKE_GROUP_POS && group != TT_BAKE_GROUP_TEX) return TT_ERR_BAD_ARG;
    if (V < 0 || Vt < 0 || T < 0 || V > TT_MESH_MAX_ITEMS || Vt > TT_MESH_MAX_ITEMS || T > TT_MESH_MAX_ITEMS)
        return TT_ERR_BAD_ARG;
    if (T > 0 && (V < 1 || Vt < 1)) return TT_ERR_BAD_ARG;
    const int G = group == TT_BAKE_GROUP_TEX ? Vt : V;
    if (G == 0) return TT_OK;
    if (!group_ptr || !out || (V > 0 && (!v_pos || !v_nrm)) || (Vt > 0 && !v_tex)) return TT_ERR_BAD_ARG;
    if (T > 0 && (!t_pos_idx || !t_tex_idx || !group_corner)) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_bake_tangents, dim3(tt_grid(G)), dim3(BAKE_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, v_tex, (const int*)t_tex_idx, v_nrm, (const int*)group_ptr,
                       (const int*)group_corner, (int)V, (int)Vt, (int)T, G, (int)(group == TT_BAKE_GROUP_TEX), out);
    return tt_check_launch();
}

extern "C" int tt_bake_project(float* points, const float* sdf, const float* sdf_grad, const uint8_t* mask, int64_t M,
                               float max_step, void* stream) {
    if (M < 0 || M > TT_BAKE_MAX_POINTS || !(max_step >= 0.f) || !(max_step <= 3.0e38f)) return TT_ERR_BAD_ARG;
    if (M == 0) return TT_OK;
    if (!points || !sdf || !sdf_grad) return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_bake_project, dim3(tt_grid(M)), dim3(BAKE_BLOCK), 0, (hipStream_t)stream, points, sdf,
                       sdf_grad, (const unsigned char*)mask, (long long)M, max_step);
    return tt_check_launch();
}

extern "C" int tt_bake_encode(const float* rast, const float* v_nrm, const int32_t* t_pos_idx, const float* tng_tex,
                              const int32_t* t_tex_idx, const float* field_nrm, int32_t V, int32_t Vt, int32_t T,
                              int32_t H, int32_t W, float* out, int32_t* out_counts, void* stream) {
    if (V < 0 || Vt < 0 || T < 0 || H < 0 || W < 0) return TT_ERR_BAD_ARG;
    if (V > TT_MESH_MAX_ITEMS || Vt > TT_MESH_MAX_ITEMS || T >= TT_RAST_MAX_TRIS) return TT_ERR_BAD_ARG;
    if (T > 0 && (V < 1 || Vt < 1)) return TT_ERR_BAD_ARG;
    const long long n = (long long)H * W;
    if (n > TT_BAKE_MAX_POINTS || !out_counts) return TT_ERR_BAD_ARG;
    if (n > 0 && (!rast || !field_nrm || !out)) return TT_ERR_BAD_ARG;
    if (n > 0 && T > 0 && (!t_pos_idx || !t_tex_idx || !v_nrm || !tng_tex)) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bake_zero_counts, dim3(1), dim3(64), 0, s, (int*)out_counts);
    if (n == 0) return tt_check_launch();
    hipLaunchKernelGGL(k_bake_encode, dim3(tt_grid(n)), dim3(BAKE_BLOCK), 0, s, rast, v_nrm, (const int*)t_pos_idx,
                       tng_tex, (const int*)t_tex_idx, field_nrm, (int)V, (int)Vt, (int)T, n, out, (int*)out_counts);
    return tt_check_launch();
}
