// tt_texture.hip -- 2-D texture sampling and its backward: the drop-in for nvdiffrast's `texture` (CUDA-only) without
// mipmaps, which closes the rasterize / interpolate / texture / antialias set of tt_raster.hip.  The contract (texel
// centres, the four taps, the boundary rules, non-finite uv) is written in include/tt_abi.h, "texture sampling".
//
// One thread per pixel: the taps and weights of both axes are computed once, then the channels are looped over (C is
// contiguous: one float4 / float2 per tap for C = 4 / 2).  Tap indices are formed as floats (wrapped by a floating-point
// modulo, then clamped to [0, size - 1] by fmin / fmax) and only then converted, so no uv value, however large or
// non-finite, reaches an address outside the texture.  The forward and grad_uv are gathers (bit-identical across
// launches); grad_tex is scattered with fp32 atomic adds.
#include "tt_host.h"
#include "tt_mask.h"

#pragma clang fp contract(off)  // x = u * size - 0.5 as written

#define TX_BLOCK 256

// one axis of a sample: the two taps, their weights and d weight / d x (x in texels)
struct TexAxis {
    int i0, i1;
    float w0, w1, d0, d1;
};

// LINEAR: taps floor(x), floor(x) + 1 of x = u n - 0.5 with weights 1 - f, f.  Nearest: the one tap floor(u n), weight 1
// (i1 = i0, w1 = d0 = d1 = 0).  Selects depend on one compare each (tt_mask.h); the in-range test of the zero boundary
// is |i - (n-1)/2| <= (n-1)/2.
template <int LINEAR>
__device__ __forceinline__ TexAxis tex_axis(float u, int n, int boundary) {
    const float fn = (float)n, last = fn - 1.f;
    // wrap: whole periods are taken off first (exact in fp32, and no compare), so x keeps its precision at large |u|
    if (boundary == TT_TEX_BOUNDARY_WRAP) u = u - truncf(u);
    const float x = LINEAR ? u * fn - 0.5f : u * fn;
    const float xf = floorf(x);
    const float f = LINEAR ? x - xf : 0.f;
    float a = xf, b = xf + 1.f, in0 = 1.f, in1 = 1.f;
    if (boundary == TT_TEX_BOUNDARY_WRAP) {
        a = xf - floorf(xf / fn) * fn;  // exact below 2^24 up to the quotient's rounding, which the next two lines undo
        a = a < 0.f ? a + fn : a;
        a = a >= fn ? a - fn : a;
        b = a + 1.f;
        b = b >= fn ? b - fn : b;
    } else if (boundary == TT_TEX_BOUNDARY_ZERO) {
        const float c = 0.5f * last;
        in0 = fabsf(a - c) <= c ? 1.f : 0.f;
        in1 = fabsf(b - c) <= c ? 1.f : 0.f;
    }
    TexAxis t;
    t.i0 = (int)fminf(fmaxf(a, 0.f), last);  // fmax(NaN, 0) = 0: every float lands in [0, n - 1]
    t.i1 = LINEAR ? (int)fminf(fmaxf(b, 0.f), last) : t.i0;
    t.w0 = LINEAR ? (1.f - f) * in0 : in0;
    t.w1 = LINEAR ? f * in1 : 0.f;
    t.d0 = LINEAR ? -in0 : 0.f;
    t.d1 = LINEAR ? in1 : 0.f;
    return t;
}

__device__ __forceinline__ bool tex_finite(float u, float v) {
    return fabsf(u) + fabsf(v) < __builtin_inff();  // one compare: false for NaN and +-inf in either component
}

// CT > 0: C = CT known at compile time and every pointer aligned for CT-wide (and uv for 2-wide) vector access;
// CT = 0: any C, scalar access.
template <int CT>
__device__ __forceinline__ void tex_load(const float* __restrict__ p, float (&v)[CT ? CT : 1]) {
    if constexpr (CT == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else if constexpr (CT == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p);
        v[0] = q.x, v[1] = q.y;
    } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) v[c] = p[c];
    }
}

template <int CT>
__device__ __forceinline__ void tex_store(float* __restrict__ p, const float (&v)[CT ? CT : 1]) {
    if constexpr (CT == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (CT == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) p[c] = v[c];
    }
}

template <int CT>
__device__ __forceinline__ void tex_load_uv(const float* __restrict__ uv, long long p, float& u, float& v) {
    if constexpr (CT > 0) {
        const float2 q = reinterpret_cast<const float2*>(uv)[p];
        u = q.x, v = q.y;
    } else {
        u = uv[2 * p], v = uv[2 * p + 1];
    }
}

struct TexArgs {
    const float* tex;
    const float* uv;
    long long npix, pix_per_image;  // B H W, H W
    int tex_batch, TH, TW, C, boundary;
};

// the four tap rows of pixel p: element offsets (64-bit) of (y0,x0), (y0,x1), (y1,x0), (y1,x1) in the pixel's image
struct TexTaps {
    long long o00, o01, o10, o11;
};

__device__ __forceinline__ TexTaps tex_taps(const TexArgs& a, long long p, const TexAxis& ax, const TexAxis& ay, int C) {
    const long long n = a.tex_batch == 1 ? 0 : p / a.pix_per_image;
    const long long r0 = (n * a.TH + ay.i0) * a.TW, r1 = (n * a.TH + ay.i1) * a.TW;
    TexTaps t;
    t.o00 = (r0 + ax.i0) * C;
    t.o01 = (r0 + ax.i1) * C;
    t.o10 = (r1 + ax.i0) * C;
    t.o11 = (r1 + ax.i1) * C;
    return t;
}

template <int LINEAR, int CT>
__global__ __launch_bounds__(TX_BLOCK) void k_tex_fwd(TexArgs a, float* __restrict__ out) {
    const long long p = (long long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (p >= a.npix) return;
    const int C = CT ? CT : a.C;
    float u, v;
    tex_load_uv<CT>(a.uv, p, u, v);
    float* o = out + p * C;
    if (!tex_finite(u, v)) {
        if constexpr (CT > 0) {
            const float z[CT ? CT : 1] = {};
            tex_store<CT>(o, z);
        } else {
            for (int c = 0; c < C; ++c) o[c] = 0.f;
        }
        return;
    }
    const TexAxis ax = tex_axis<LINEAR>(u, a.TW, a.boundary), ay = tex_axis<LINEAR>(v, a.TH, a.boundary);
    const TexTaps t = tex_taps(a, p, ax, ay, C);
    const float w00 = ay.w0 * ax.w0, w01 = ay.w0 * ax.w1, w10 = ay.w1 * ax.w0, w11 = ay.w1 * ax.w1;
    if constexpr (CT > 0) {
        float t00[CT ? CT : 1], t01[CT ? CT : 1], t10[CT ? CT : 1], t11[CT ? CT : 1], r[CT ? CT : 1];
        tex_load<CT>(a.tex + t.o00, t00);
        if (LINEAR) {
            tex_load<CT>(a.tex + t.o01, t01);
            tex_load<CT>(a.tex + t.o10, t10);
            tex_load<CT>(a.tex + t.o11, t11);
        }
#pragma unroll
        for (int c = 0; c < CT; ++c)
            r[c] = LINEAR ? (w00 * t00[c] + w01 * t01[c]) + (w10 * t10[c] + w11 * t11[c]) : w00 * t00[c];
        tex_store<CT>(o, r);
    } else {
        const float *t00 = a.tex + t.o00, *t01 = a.tex + t.o01, *t10 = a.tex + t.o10, *t11 = a.tex + t.o11;
        for (int c = 0; c < C; ++c)
            o[c] = LINEAR ? (w00 * t00[c] + w01 * t01[c]) + (w10 * t10[c] + w11 * t11[c]) : w00 * t00[c];
    }
}

// one channel of a pixel's contribution to grad_tex.  A zero term is not added: the background pixels of a masked
// render (grad_out = 0, uv = 0) would otherwise all meet in one texel, and a tap of weight 0 is no tap.
template <int LINEAR>
__device__ __forceinline__ void tex_scatter(float* __restrict__ grad_tex, const TexTaps& t, float w00, float w01,
                                            float w10, float w11, float g) {
    const float v00 = w00 * g, v01 = w01 * g, v10 = w10 * g, v11 = w11 * g;
    if (v00 != 0.f) atomicAdd(grad_tex + t.o00, v00);
    if (LINEAR) {
        if (v01 != 0.f) atomicAdd(grad_tex + t.o01, v01);
        if (v10 != 0.f) atomicAdd(grad_tex + t.o10, v10);
        if (v11 != 0.f) atomicAdd(grad_tex + t.o11, v11);
    }
}

// grad_tex (zeroed by the entry point) += weight x grad_out at the taps; grad_uv = (TW d/dx, TH d/dy) of the sample,
// zero under nearest and at non-finite uv.  Either output may be null.
template <int LINEAR, int CT>
__global__ __launch_bounds__(TX_BLOCK) void k_tex_bwd(TexArgs a, const float* __restrict__ grad_out,
                                                      float* __restrict__ grad_tex, float* __restrict__ grad_uv) {
    const long long p = (long long)blockIdx.x * TX_BLOCK + threadIdx.x;
    if (p >= a.npix) return;
    const int C = CT ? CT : a.C;
    float u, v, gu = 0.f, gv = 0.f;
    tex_load_uv<CT>(a.uv, p, u, v);
    if (tex_finite(u, v)) {
        const TexAxis ax = tex_axis<LINEAR>(u, a.TW, a.boundary), ay = tex_axis<LINEAR>(v, a.TH, a.boundary);
        const TexTaps t = tex_taps(a, p, ax, ay, C);
        const float w00 = ay.w0 * ax.w0, w01 = ay.w0 * ax.w1, w10 = ay.w1 * ax.w0, w11 = ay.w1 * ax.w1;
        const float* go = grad_out + p * C;
        const bool want_uv = LINEAR && grad_uv != nullptr;
        if constexpr (CT > 0) {
            float g[CT ? CT : 1];
            tex_load<CT>(go, g);
            if (want_uv) {
                float t00[CT ? CT : 1], t01[CT ? CT : 1], t10[CT ? CT : 1], t11[CT ? CT : 1];
                tex_load<CT>(a.tex + t.o00, t00);
                tex_load<CT>(a.tex + t.o01, t01);
                tex_load<CT>(a.tex + t.o10, t10);
                tex_load<CT>(a.tex + t.o11, t11);
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    gu += g[c] * (ay.w0 * (ax.d0 * t00[c] + ax.d1 * t01[c]) + ay.w1 * (ax.d0 * t10[c] + ax.d1 * t11[c]));
                    gv += g[c] * (ay.d0 * (ax.w0 * t00[c] + ax.w1 * t01[c]) + ay.d1 * (ax.w0 * t10[c] + ax.w1 * t11[c]));
                }
            }
            if (grad_tex) {
#pragma unroll
                for (int c = 0; c < CT; ++c) tex_scatter<LINEAR>(grad_tex + c, t, w00, w01, w10, w11, g[c]);
            }
        } else {
            const float *t00 = a.tex + t.o00, *t01 = a.tex + t.o01, *t10 = a.tex + t.o10, *t11 = a.tex + t.o11;
            for (int c = 0; c < C; ++c) {
                const float g = go[c];
                if (want_uv) {
                    gu += g * (ay.w0 * (ax.d0 * t00[c] + ax.d1 * t01[c]) + ay.w1 * (ax.d0 * t10[c] + ax.d1 * t11[c]));
                    gv += g * (ay.d0 * (ax.w0 * t00[c] + ax.w1 * t01[c]) + ay.d1 * (ax.w0 * t10[c] + ax.w1 * t11[c]));
                }
                if (grad_tex) tex_scatter<LINEAR>(grad_tex + c, t, w00, w01, w10, w11, g);
            }
        }
        gu *= (float)a.TW;
        gv *= (float)a.TH;
    }
    if (grad_uv) {
        if constexpr (CT > 0) {
            reinterpret_cast<float2*>(grad_uv)[p] = make_float2(gu, gv);
        } else {
            grad_uv[2 * p] = gu;
            grad_uv[2 * p + 1] = gv;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI

static bool tx_dims_ok(int tex_batch, int B, int H, int W, int TH, int TW, int C, int filter, int boundary) {
    return B >= 0 && H >= 0 && W >= 0 && (long long)B * H * W < (1ll << 40) && TH >= 1 && TW >= 1 &&
           TH <= TT_TEX_MAX_SIZE && TW <= TT_TEX_MAX_SIZE && C >= 1 && tex_batch >= 1 &&
           (tex_batch == 1 || tex_batch == B) &&
           (filter == TT_TEX_FILTER_NEAREST || filter == TT_TEX_FILTER_LINEAR) &&
           (boundary == TT_TEX_BOUNDARY_WRAP || boundary == TT_TEX_BOUNDARY_CLAMP || boundary == TT_TEX_BOUNDARY_ZERO);
}

static bool tx_aligned(const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// the compile-time channel count of a launch: C itself for C <= 4 when every per-pixel / per-texel row (C floats) and
// the uv pairs sit on their vector alignment, else 0 (scalar access)
static int tx_ct(int C, const void* uv, const void* grad_uv, const void* r0, const void* r1, const void* r2) {
    if (C > 4 || !tx_aligned(uv, 8) || !tx_aligned(grad_uv, 8)) return 0;
    const size_t row = C == 4 ? 16 : (C == 2 ? 8 : 4);
    return tx_aligned(r0, row) && tx_aligned(r1, row) && tx_aligned(r2, row) ? C : 0;
}

// calls f(LINEAR, CT) as std::integral_constant<int, .>
template <class F>
static void tx_dispatch(int filter, int ct, F&& f) {
    auto by_ct = [&](auto L) {
        switch (ct) {
            case 1: f(L, std::integral_constant<int, 1>{}); break;
            case 2: f(L, std::integral_constant<int, 2>{}); break;
            case 3: f(L, std::integral_constant<int, 3>{}); break;
            case 4: f(L, std::integral_constant<int, 4>{}); break;
            default: f(L, std::integral_constant<int, 0>{}); break;
        }
    };
    if (filter == TT_TEX_FILTER_LINEAR)
        by_ct(std::integral_constant<int, 1>{});
    else
        by_ct(std::integral_constant<int, 0>{});
}

static unsigned tx_blocks(long long n) { return (unsigned)((n + TX_BLOCK - 1) / TX_BLOCK); }

extern "C" int tt_tex_fwd(const float* tex, int32_t tex_batch, const float* uv, int32_t B, int32_t H, int32_t W,
                          int32_t TH, int32_t TW, int32_t C, int32_t filter, int32_t boundary, float* out,
                          void* stream) {
    if (!tx_dims_ok(tex_batch, B, H, W, TH, TW, C, filter, boundary)) return TT_ERR_BAD_ARG;
    const long long npix = (long long)B * H * W;
    if (npix == 0) return TT_OK;
    if (!tex || !uv || !out) return TT_ERR_BAD_ARG;
    const TexArgs a{tex, uv, npix, (long long)H * W, tex_batch, TH, TW, C, boundary};
    tx_dispatch(filter, tx_ct(C, uv, nullptr, tex, out, nullptr), [&](auto L, auto CT) {
        hipLaunchKernelGGL((k_tex_fwd<decltype(L)::value, decltype(CT)::value>), dim3(tx_blocks(npix)), dim3(TX_BLOCK),
                           0, (hipStream_t)stream, a, out);
    });
    return tt_check_launch();
}

extern "C" int tt_tex_bwd(const float* tex, int32_t tex_batch, const float* uv, const float* grad_out, int32_t B,
                          int32_t H, int32_t W, int32_t TH, int32_t TW, int32_t C, int32_t filter, int32_t boundary,
                          float* grad_tex, float* grad_uv, void* stream) {
    if (!tx_dims_ok(tex_batch, B, H, W, TH, TW, C, filter, boundary)) return TT_ERR_BAD_ARG;
    const long long npix = (long long)B * H * W;
    if (npix > 0 && (!tex || !uv || !grad_out)) return TT_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (grad_tex && hipMemsetAsync(grad_tex, 0, (size_t)tex_batch * TH * TW * C * 4, st) != hipSuccess)
        return TT_ERR_LAUNCH;
    if (npix == 0 || (!grad_tex && !grad_uv)) return tt_check_launch();
    const TexArgs a{tex, uv, npix, (long long)H * W, tex_batch, TH, TW, C, boundary};
    tx_dispatch(filter, tx_ct(C, uv, grad_uv, tex, grad_out, grad_tex), [&](auto L, auto CT) {
        hipLaunchKernelGGL((k_tex_bwd<decltype(L)::value, decltype(CT)::value>), dim3(tx_blocks(npix)), dim3(TX_BLOCK),
                           0, st, a, grad_out, grad_tex, grad_uv);
    });
    return tt_check_launch();
}
