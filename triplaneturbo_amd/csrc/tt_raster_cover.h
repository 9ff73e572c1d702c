// tt_raster_cover.h -- the rasterizer's triangle setup and pixel-centre coverage test (include/tt_abi.h, "rasterize"),
// shared by tt_raster.hip and the UV-atlas overlap guard of tt_uv.hip, so that both decide whether a pixel centre lies
// in a triangle with the same edge functions and the same tie rule, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)  // edge functions exactly as written: shared edges must see exactly negated values

// ---------------------------------------------------------------------------------------------------------------
// triangle setup shared by every kernel (one function, so that coverage, resolve and backward agree bit for bit)

struct TriSetup {
    int idx[3];
    float x[3], y[3], z[3], w[3];
    bool homog;     // some w <= 0: homogeneous edge functions (but an edge with both endpoints at w > 0 is decided by
                    // the screen-space form: tri_cover); else screen-space ones (all w > 0, the common case)
    float X[3], Y[3], ZW[3];  // screen path: NDC x/w, y/w, z/w of the vertices
    float n[3][3];  // homogeneous path: canonical edge k (opposite vertex k) v_lo x v_hi over (x, y, w)
    float XL[3], YL[3];       // their rounding residuals (x/w = X + XL to about twice float precision)
    float ex[3][4];  // screen path: canonical endpoints of edge k (X, Y of the lower vertex index, then the higher)
    float el[3][4];  // and their residuals
    float sg[3];    // +-1: sign of the true edge function (cyclic order) relative to the canonical one, times sign(D)
    float sd;       // sign(D), D = det[v0, v1, v2] over (x, y, w) (= sign of the screen area when all w > 0)
};

__device__ __forceinline__ void cross3(float ax, float ay, float aw, float bx, float by, float bw, float* o) {
    o[0] = ay * bw - aw * by;
    o[1] = aw * bx - ax * bw;
    o[2] = ax * by - ay * bx;
}

__device__ __forceinline__ bool tri_indices(const int* __restrict__ tri, long long t, int V, int* idx) {
#pragma unroll
    for (int k = 0; k < 3; ++k) idx[k] = tri[t * 3 + k];
    return (unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V;
}

__device__ __forceinline__ float4 vtx(const float* __restrict__ pos, int b, int V, int i) {
    return reinterpret_cast<const float4*>(pos)[(long long)b * V + i];
}

// orientation sign of triangle t in view b (0: degenerate / invalid indices)
__device__ __forceinline__ float tri_orient(const float* __restrict__ pos, const int* __restrict__ tri, int b, int t,
                                            int V) {
    int idx[3];
    if (!tri_indices(tri, t, V, idx)) return 0.f;
    const float4 a = vtx(pos, b, V, idx[0]), c = vtx(pos, b, V, idx[1]), e = vtx(pos, b, V, idx[2]);
    float n[3];
    cross3(a.x, a.y, a.w, c.x, c.y, c.w, n);
    const float D = n[0] * e.x + n[1] * e.y + n[2] * e.w;
    return D > 0.f ? 1.f : (D < 0.f ? -1.f : 0.f);
}

// false: the triangle never produces fragments (invalid or repeated indices, non-finite positions, zero area)
__device__ __forceinline__ bool tri_setup(const float* __restrict__ pos, const int* __restrict__ tri, int b, int t, int V,
                          TriSetup& s) {
    if (!tri_indices(tri, t, V, s.idx)) return false;
    if (s.idx[0] == s.idx[1] || s.idx[1] == s.idx[2] || s.idx[0] == s.idx[2]) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 p = vtx(pos, b, V, s.idx[k]);
        s.x[k] = p.x;
        s.y[k] = p.y;
        s.z[k] = p.z;
        s.w[k] = p.w;
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w))) return false;
    }
    s.homog = !(fminf(fminf(s.w[0], s.w[1]), s.w[2]) > 0.f);  // one compare (finite here): see pix_tri
    // screen-space edge functions from coordinate differences when all w > 0: accurate for triangles of a few pixels,
    // where the homogeneous cross products lose the small area to cancellation (the homogeneous path uses them on the
    // edges whose two endpoints have w > 0; a quotient by w <= 0 stays in its own vertex's entries, which no such
    // edge reads)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.X[k] = s.x[k] / s.w[k];
        s.Y[k] = s.y[k] / s.w[k];
        s.ZW[k] = s.z[k] / s.w[k];
        // the quotient's residual: the edge functions of sliver triangles subtract nearly equal coordinates
        s.XL[k] = fmaf(-s.X[k], s.w[k], s.x[k]) / s.w[k];
        s.YL[k] = fmaf(-s.Y[k], s.w[k], s.y[k]) / s.w[k];
    }
    float n01[3];
    cross3(s.x[0], s.y[0], s.w[0], s.x[1], s.y[1], s.w[1], n01);
    const float Dh = n01[0] * s.x[2] + n01[1] * s.y[2] + n01[2] * s.w[2];
    const float Ds = (s.X[1] - s.X[0]) * (s.Y[2] - s.Y[0]) - (s.Y[1] - s.Y[0]) * (s.X[2] - s.X[0]);
    const float D = s.homog ? Dh : Ds;
    if (!(D != 0.f) || !isfinite(D)) return false;
    s.sd = D > 0.f ? 1.f : -1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const bool fwd = s.idx[i] < s.idx[j];
        // (selects between the two compile-time vertex numbers: no dynamically indexed private arrays)
        // (both forms, unconditionally: a store into one of two private arrays chosen at run time goes to scratch)
        cross3(fwd ? s.x[i] : s.x[j], fwd ? s.y[i] : s.y[j], fwd ? s.w[i] : s.w[j], fwd ? s.x[j] : s.x[i],
               fwd ? s.y[j] : s.y[i], fwd ? s.w[j] : s.w[i], s.n[k]);
        s.ex[k][0] = fwd ? s.X[i] : s.X[j];
        s.ex[k][1] = fwd ? s.Y[i] : s.Y[j];
        s.ex[k][2] = fwd ? s.X[j] : s.X[i];
        s.ex[k][3] = fwd ? s.Y[j] : s.Y[i];
        s.el[k][0] = fwd ? s.XL[i] : s.XL[j];
        s.el[k][1] = fwd ? s.YL[i] : s.YL[j];
        s.el[k][2] = fwd ? s.XL[j] : s.XL[i];
        s.el[k][3] = fwd ? s.YL[j] : s.YL[i];
        s.sg[k] = fwd ? s.sd : -s.sd;
    }
    return true;
}

// NDC of pixel centre (px, py): x = (2 px + 1) / W - 1, y = (2 py + 1) / H - 1
__device__ __forceinline__ float pix_ndc(int p, int N) { return (float)(2 * p + 1) / (float)N - 1.f; }
// its rounding residual: the exact value is pix_ndc + pix_ndc_lo to about twice float precision
__device__ __forceinline__ float pix_ndc_lo(int p, int N) {
    const float n = (float)(2 * p + 1), q = n / (float)N;
    const float rq = fmaf(-q, (float)N, n) / (float)N;  // q + rq = n / N
    const float hi = q - 1.f;
    const float err = q - (hi + 1.f);                      // Fast2Sum of q + (-1): |-1| >= |q| for q < 1
    return err + rq;
}

// coverage test + perspective-correct (u, v, z/w) at NDC (X, Y).  S = the sum of the three homogeneous oriented edge
// values sign(D) (v_i x v_j) . (X, Y, 1) (= |D| / interpolated w), which the backward divides by.
__device__ __forceinline__ bool tri_cover(const TriSetup& s, float X, float XL, float Y, float YL, float& u, float& v,
                                          float& zw, float& S) {
    float te[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // An edge whose endpoints both have w > 0 is decided (sign and tie) by the screen-space form, on either path:
        // its neighbour across the edge may be a screen-path triangle, and the two forms, which differ by the factor
        // w_lo w_hi > 0 in exact arithmetic, are not each other's negation in float.  The same operands in the same
        // order on both sides are.
        float c, gx, gy;
        // (ex / el of such an edge hold quotients by its own two w only: nothing of a vertex at w <= 0 reaches it)
        const bool scr = fminf(s.w[(k + 1) % 3], s.w[(k + 2) % 3]) > 0.f;  // one compare; every edge of the screen path
        if (scr) {
            const float ax = (s.ex[k][0] - X) + (s.el[k][0] - XL), ay = (s.ex[k][1] - Y) + (s.el[k][1] - YL);
            const float bx = (s.ex[k][2] - X) + (s.el[k][2] - XL), by = (s.ex[k][3] - Y) + (s.el[k][3] - YL);
            c = ax * by - ay * bx;
            gx = s.ex[k][1] - s.ex[k][3];
            gy = s.ex[k][2] - s.ex[k][0];
        } else {
            c = (s.n[k][0] * X + s.n[k][1] * Y) + s.n[k][2];
            gx = s.n[k][0];
            gy = s.n[k][1];
        }
        const float t = s.sg[k] * c;
        if (t < 0.f) return false;
        if (t == 0.f) {  // on the edge: the triangle owns it iff its inward normal points to +x (or +y if vertical)
            gx *= s.sg[k];
            gy *= s.sg[k];
            if (!(gx > 0.f || (gx == 0.f && gy > 0.f))) return false;
        }
        if (!(t >= 0.f)) return false;  // NaN
        te[k] = t;
        if (s.homog) {
            if (scr) {
                // (u, v, z/w) of a homogeneous-path triangle weigh every edge by its homogeneous value; where rounding
                // puts it on the other side of the edge than the deciding screen-space form, the weight is 0
                const float th = s.sg[k] * ((s.n[k][0] * X + s.n[k][1] * Y) + s.n[k][2]);
                if (th != th) return false;
                te[k] = fmaxf(th, 0.f);
            }
        }
    }
    if (s.homog) {
        const float sum = (te[0] + te[1]) + te[2];
        if (!(sum > 0.f)) return false;
        const float den = (te[0] * s.w[0] + te[1] * s.w[1]) + te[2] * s.w[2];
        if (!(den > 0.f)) return false;
        const float num = (te[0] * s.z[0] + te[1] * s.z[1]) + te[2] * s.z[2];
        zw = num / den;
        u = te[0] / sum;
        v = te[1] / sum;
        S = sum;
    } else {
        const float sum = (te[0] + te[1]) + te[2];  // screen area: z/w is affine in screen space
        if (!(sum > 0.f)) return false;
        zw = ((te[0] * s.ZW[0] + te[1] * s.ZW[1]) + te[2] * s.ZW[2]) / sum;
        const float l0 = te[0] / s.w[0], l1 = te[1] / s.w[1], l2 = te[2] / s.w[2];
        const float L = (l0 + l1) + l2;
        u = l0 / L;
        v = l1 / L;
        S = ((s.w[0] * s.w[1]) * s.w[2]) * L;
    }
    if (!(zw >= -1.f && zw <= 1.f)) return false;
    return true;
}
