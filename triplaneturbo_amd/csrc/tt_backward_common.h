// tt_backward_common.h -- what the two translation units of the fused render backward share: the LDS transposition /
// outer-product / matrix-core scatter building blocks, the per-launch bound reductions and small host helpers.
// tt_backward.hip holds the geometry half, tt_backward_tex.hip the texture half (separate units: each kernel is
// ~9000 instructions per loop body, and the texture unit is compiled with its own scheduler strategy, _lib.py).
#pragma once
#include "tt_device.h"
#include "tt_mfma16.h"
#include "tt_alpha.h"
#include "tt_launch.h"
#include <type_traits>

typedef int i32x4 __attribute__((ext_vector_type(4)));

// tuning build only: cycles per phase of the texture backward, summed over waves into p.phase_cycles[16]
#ifdef TT_TUNING
#define TT_PHASE(k)                                              \
    do {                                                         \
        __builtin_amdgcn_sched_barrier(0);                       \
        const unsigned long long t_now = __builtin_amdgcn_s_memtime(); \
        ph_acc[k] += t_now - ph_t;                               \
        ph_t = t_now;                                            \
        __builtin_amdgcn_sched_barrier(0);                       \
    } while (0)
#else
#define TT_PHASE(k) \
    do {            \
    } while (0)
#endif
#define XS 36  // row stride (floats) of the [index][sample] transposition scratch

// ---- LDS transposition helpers (wave-private scratch; DS ops of one wave execute in order) ----------
template <int N>
__device__ __forceinline__ void stage_rows(float* S, const float (&v)[N / 2], int j, int hi) {
#pragma unroll
    for (int r = 0; r < N / 2; ++r) S[LIDX(r, hi) * XS + j] = v[r];
}
// stage the N-element slice of a longer register vector that starts at register OFF
template <int N, int OFF, int TOT>
__device__ __forceinline__ void stage_rows_sub(float* S, const float (&v)[TOT], int j, int hi) {
#pragma unroll
    for (int r = 0; r < N / 2; ++r) S[LIDX(r, hi) * XS + j] = v[OFF + r];
}
// the 0/1 mask (v > 0) of a register vector as 1.0f / 0.0f rows: one compare + one select per entry (tt_mask.h)
template <int N>
__device__ __forceinline__ void stage_rows_mask(float* S, const float (&v)[N / 2], int j, int hi) {
#pragma unroll
    for (int r = 0; r < N / 2; ++r) S[LIDX(r, hi) * XS + j] = v[r] > 0.f ? 1.f : 0.f;
}

// acc[m][n] += X[32m.., s] * Y[32n.., s]^T summed over the 32 samples s of the tile
template <int NX, int NY>
__device__ __forceinline__ void wgrad(f32x16 (&acc)[NX / 32][NY / 32], const float* Xs, const float* Ys, int i,
                                      int hi) {
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
        f32x4 xa[NX / 32], yb[NY / 32];
#pragma unroll
        for (int m = 0; m < NX / 32; ++m)
            xa[m] = *reinterpret_cast<const f32x4*>(Xs + (32 * m + i) * XS + 16 * hi + 4 * t4);
#pragma unroll
        for (int n = 0; n < NY / 32; ++n)
            yb[n] = *reinterpret_cast<const f32x4*>(Ys + (32 * n + i) * XS + 16 * hi + 4 * t4);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int m = 0; m < NX / 32; ++m)
#pragma unroll
                for (int n = 0; n < NY / 32; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[m][k], yb[n][k], acc[m][n], 0, 0, 0);
    }
}

// one 32-row slice of the left operand: acc[n] += X[0..31, s] * Y[32n.., s]^T
template <int NY>
__device__ __forceinline__ void wgrad_row(f32x16 (&acc)[NY / 32], const float* Xs, const float* Ys, int i, int hi) {
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
        f32x4 yb[NY / 32];
        const f32x4 xa = *reinterpret_cast<const f32x4*>(Xs + i * XS + 16 * hi + 4 * t4);
#pragma unroll
        for (int n = 0; n < NY / 32; ++n)
            yb[n] = *reinterpret_cast<const f32x4*>(Ys + (32 * n + i) * XS + 16 * hi + 4 * t4);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int n = 0; n < NY / 32; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k], yb[n][k], acc[n], 0, 0, 0);
    }
}

// ---- weight-gradient outer products on the fp16 pipe -----------------------------------------------------------------
// acc[m][n] += X[32m.., s] Y[32n.., s]^T over the 32 samples of the tile, as 2-term split-fp16 products (tt_mfma16.h)
// with PER-LAUNCH operand scales (powers of two from rigorous magnitude bounds, wg16_scale below): nothing is ever
// rescaled inside the sample loop, so the persistent accumulators are touched by MFMAs only (per-tile or per-wave
// "sticky" scales need in-loop arithmetic on the 96-160 accumulator registers, which makes the allocator spill: measured
// in round 2).  An operand entry v is staged as ONE dword (hi | lo << 16), hi = f16(v sc), lo = f16(v sc - hi), in the
// same [index][sample] scratch as the fp32 form.  The two halves of a dword are fed to the MFMA as two ADJACENT k-slots:
// a k-step of 16 slots is 8 samples, slot 2d = hi, slot 2d + 1 = lo of the lane's d-th sample, for both operands -- so
//     mfma(A, B)          = sum_s (hi_x hi_y + lo_x lo_y)
//     mfma(A, rot16(B))   = sum_s (hi_x lo_y + lo_x hi_y)
// together the FULL product of the two split numbers: 8 MFMAs of 32 cycles per 32 x 32 tile instead of 16 fp32 MFMAs of
// 64, no de-interleaving, one v_alignbit per B dword.  Error per product term <= 2^-22 of the operands' global maxima:
// fp32-grade for a sum over all samples (the fp32 accumulator itself resolves 2^-24 of the running sum).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 2^(141 - E) for a bound with biased exponent E: maps [0, bound] into the fp16 range (bound -> [2^14, 2^15))
__device__ __forceinline__ float wg16_scale(float bound) {
    int E = (int)(__builtin_bit_cast(unsigned, bound * 1.0001f) >> 23) & 0xff;
    E = E < 16 ? 16 : (E > 240 ? 240 : E);
    return __builtin_bit_cast(float, (unsigned)(268 - E) << 23);
}
__device__ __forceinline__ unsigned wg16_pack(float x) {  // (hi | lo << 16), both round-to-nearest-even: hi + lo ~ x
    // three instructions in one block (see split_pair, tt_mfma16.h): hi = f16(x); r = x * 1.0 - hi (exact); pack(x, r)
    unsigned out;
    float r;
    asm("v_cvt_pk_f16_f32 %0, %2, 0\n\t"
        "v_fma_mix_f32 %1, %2, 1.0, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_cvt_pk_f16_f32 %0, %2, %1"
        : "=&v"(out), "=&v"(r)
        : "v"(x));
    return out;
}
template <int N>
__device__ __forceinline__ void stage_rows16(float* S, const float (&v)[N / 2], int j, int hi, float sc) {
    unsigned* U = reinterpret_cast<unsigned*>(S);
#pragma unroll
    for (int r = 0; r < N / 2; ++r) U[LIDX(r, hi) * XS + j] = wg16_pack(v[r] * sc);
}
template <int N, int OFF, int TOT>
__device__ __forceinline__ void stage_rows16_sub(float* S, const float (&v)[TOT], int j, int hi, float sc) {
    unsigned* U = reinterpret_cast<unsigned*>(S);
#pragma unroll
    for (int r = 0; r < N / 2; ++r) U[LIDX(r, hi) * XS + j] = wg16_pack(v[OFF + r] * sc);
}
// the same rows from a vector already split by split16_vec (tt_mfma16.h): one v_perm per staged dword
template <int N, int PAIR, int NT>
__device__ __forceinline__ void stage_rows16_pre(float* S, const Split16<N, PAIR, NT>& v, int j, int hi) {
    unsigned* U = reinterpret_cast<unsigned*>(S);
#pragma unroll
    for (int t = 0; t < N / 4; ++t) {  // dword t of the split holds registers pair_reg<PAIR>(t, 0 / 1)
        U[LIDX(pair_reg<PAIR>(t, 0), hi) * XS + j] = __builtin_amdgcn_perm(v.l[t], v.h[t], 0x05040100u);  // (hi | lo << 16)
        U[LIDX(pair_reg<PAIR>(t, 1), hi) * XS + j] = __builtin_amdgcn_perm(v.l[t], v.h[t], 0x07060302u);
    }
}
// the 0/1 mask of a register vector as the X operand of wgrad16_mask: 1.0 is exact in ONE fp16 piece, and the dword
// (1.0 | 1.0 << 16) puts it into both k-slots of the sample.  The mask comes as the fp16 pairs of mask16_pairs
// (tt_mfma16.h; dword t <-> registers 2 t, 2 t + 1): one v_perm per entry replicates the entry's half
template <int N>
__device__ __forceinline__ void stage_rows16_mask(float* S, const unsigned (&mb)[N / 4], int j, int hi) {
    unsigned* U = reinterpret_cast<unsigned*>(S);
#pragma unroll
    for (int t = 0; t < N / 4; ++t) {
        U[LIDX(2 * t, hi) * XS + j] = __builtin_amdgcn_perm(0u, mb[t], 0x01000100u);
        U[LIDX(2 * t + 1, hi) * XS + j] = __builtin_amdgcn_perm(0u, mb[t], 0x03020302u);
    }
}
__device__ __forceinline__ h8_t wg16_frag(const float* S, int row, int t, int hi) {
    return __builtin_bit_cast(h8_t, *reinterpret_cast<const u32x4*>(S + row * XS + 8 * t + 4 * hi));
}
__device__ __forceinline__ h8_t wg16_swap(h8_t v) {
    u32x4 u = __builtin_bit_cast(u32x4, v);
#pragma unroll
    for (int d = 0; d < 4; ++d) u[d] = __builtin_amdgcn_alignbit(u[d], u[d], 16);
    return __builtin_bit_cast(h8_t, u);
}
template <int NX, int NY>
__device__ __forceinline__ void wgrad16(f32x16 (&acc)[NX / 32][NY / 32], const float* Xs, const float* Ys, int i,
                                        int hi) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {  // k-step: samples 8 t .. 8 t + 7 (this half-wave: 8 t + 4 hi .. + 3)
        h8_t xa[NX / 32], yb[NY / 32], ys[NY / 32];
#pragma unroll
        for (int m = 0; m < NX / 32; ++m) xa[m] = wg16_frag(Xs, 32 * m + i, t, hi);
#pragma unroll
        for (int n = 0; n < NY / 32; ++n) {
            yb[n] = wg16_frag(Ys, 32 * n + i, t, hi);
            ys[n] = wg16_swap(yb[n]);
        }
#pragma unroll
        for (int m = 0; m < NX / 32; ++m)
#pragma unroll
            for (int n = 0; n < NY / 32; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[m], yb[n], acc[m][n], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NX / 32; ++m)
#pragma unroll
            for (int n = 0; n < NY / 32; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[m], ys[n], acc[m][n], 0, 0, 0);
    }
}
// X staged by stage_rows16_mask: mfma(A, B) = sum_s m (hi_y + lo_y) is already the full product, so the pass with the
// rotated B operand falls away -- 4 MFMAs per 32 x 32 tile
template <int NX, int NY>
__device__ __forceinline__ void wgrad16_mask(f32x16 (&acc)[NX / 32][NY / 32], const float* Xs, const float* Ys, int i,
                                             int hi) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        h8_t xa[NX / 32], yb[NY / 32];
#pragma unroll
        for (int m = 0; m < NX / 32; ++m) xa[m] = wg16_frag(Xs, 32 * m + i, t, hi);
#pragma unroll
        for (int n = 0; n < NY / 32; ++n) yb[n] = wg16_frag(Ys, 32 * n + i, t, hi);
#pragma unroll
        for (int m = 0; m < NX / 32; ++m)
#pragma unroll
            for (int n = 0; n < NY / 32; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[m], yb[n], acc[m][n], 0, 0, 0);
    }
}
// one 32-row slice of the left operand (see wgrad_row)
template <int NY>
__device__ __forceinline__ void wgrad16_row(f32x16 (&acc)[NY / 32], const float* Xs, const float* Ys, int i, int hi) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const h8_t xa = wg16_frag(Xs, i, t, hi);
        h8_t yb[NY / 32], ys[NY / 32];
#pragma unroll
        for (int n = 0; n < NY / 32; ++n) {
            yb[n] = wg16_frag(Ys, 32 * n + i, t, hi);
            ys[n] = wg16_swap(yb[n]);
        }
#pragma unroll
        for (int n = 0; n < NY / 32; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa, yb[n], acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < NY / 32; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa, ys[n], acc[n], 0, 0, 0);
    }
}

// workgroup-wide max of a per-thread value through a shared word (all threads call; v >= 0)
__device__ __forceinline__ float block_max(float v, unsigned* word) {
    __syncthreads();
    if (threadIdx.x == 0) *word = 0u;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) atomicMax(word, __builtin_bit_cast(unsigned, v));
    __syncthreads();
    const float r = __builtin_bit_cast(float, *word);
    __syncthreads();
    return r;
}

// Workgroup pre-reduction of one 32 x 32 accumulator tile at kernel end: the four waves' copies are summed through LDS
// (R: 2 x 4096 floats, alternating by `parity` so that one barrier per tile is enough) and wave w adds registers
// 4 w .. 4 w + 3 of the sum to memory -- a quarter of the same-address float atomics, which serialise at the memory side
// (~1 000 waves add into the same 66 KB).  All 256 threads call it, in the same order, after the main loop.
// What is added is acc * ux * uy (ux, uy: the inverse operand scales of the fp16 outer products, 1 for the fp32 ones; two
// factors so that extreme scales cannot overflow their product).
template <class Addr>
__device__ __forceinline__ void flush_tile_reduced(float* R, int parity, const f32x16& acc, int wave, int lane,
                                                   float ux, float uy, Addr addr) {
    float* B = R + parity * 4096;
#pragma unroll
    for (int r = 0; r < 16; ++r) B[(wave * 16 + r) * 64 + lane] = (acc[r] * ux) * uy;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 4 * wave + q;
        const float v = (B[r * 64 + lane] + B[(16 + r) * 64 + lane]) + (B[(32 + r) * 64 + lane] + B[(48 + r) * 64 + lane]);
        atomicAdd(addr(r), v);
    }
}
template <int NX, int NY>
__device__ __forceinline__ void flush_wgrad_reduced(float* R, int& parity, const f32x16 (&acc)[NX / 32][NY / 32],
                                                    float* __restrict__ dst, int wave, int lane, float ux, float uy) {
    const int i = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int m = 0; m < NX / 32; ++m)
#pragma unroll
        for (int n = 0; n < NY / 32; ++n) {
            flush_tile_reduced(R, parity, acc[m][n], wave, lane, ux, uy,
                               [&](int r) { return dst + (32 * m + LIDX(r, hi)) * NY + 32 * n + i; });
            parity ^= 1;
        }
}

// The last layer of a bias-free ReLU net from ONE accumulator: acc = D = sum_samples m v^T with m the 0/1 mask of the
// layer's output (tt_backward.hip, "row-scaling identity").  Per reduced 32 x 32 tile of D * uy:
//     dW[row][col] += wo[row] * D[row][col]          dwo[row] += sum_col W[row][col] * D[row][col]
// W (NX x NY) and wo (NX) are read in fp32 from memory (L2-resident, once per workgroup).  A thread holds the same four
// rows in every column tile, so the row sums are carried over n and leave as one atomic per row and workgroup.
template <int NX, int NY>
__device__ __forceinline__ void flush_d_reduced(float* R, int& parity, const f32x16 (&acc)[NX / 32][NY / 32],
                                                const float* __restrict__ W, const float* __restrict__ wo,
                                                float* __restrict__ dW, float* __restrict__ dwo, int wave, int lane,
                                                float uy) {
    const int i = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int m = 0; m < NX / 32; ++m) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < NY / 32; ++n) {
            float* B = R + parity * 4096;
#pragma unroll
            for (int r = 0; r < 16; ++r) B[(wave * 16 + r) * 64 + lane] = acc[m][n][r] * uy;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * wave + q, at = (32 * m + LIDX(r, hi)) * NY + 32 * n + i;
                const float d = (B[r * 64 + lane] + B[(16 + r) * 64 + lane]) + (B[(32 + r) * 64 + lane] + B[(48 + r) * 64 + lane]);
                atomicAdd(dW + at, wo[32 * m + LIDX(r, hi)] * d);
                part[q] = fmaf(W[at], d, part[q]);
            }
            parity ^= 1;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float s = part[q];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);  // over the 32 columns of this half-wave's row
            if (i == 0) atomicAdd(dwo + 32 * m + LIDX(4 * wave + q, hi), s);
        }
    }
}

#define ZERO16 \
    { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }

// ---- plane-gradient scatter, combined on the matrix cores --------------------------------------------------
// fp32 global atomics are THE bottleneck of the backward on MI355X (~325 G atomic float-adds/s chip-wide,
// pattern-independent; LDS fp32 atomics are even slower: one ds_add_f32 wave-instruction per ~190 cycles per CU,
// both measured with tools/atomic_bench.hip / tools/lds_atomic_bench.hip).  A tile is 32 adjacent rays at one
// depth, so its 128 (sample, corner) references per plane touch only ~25-70 distinct texels.  Per plane the
// tile's gradient is
//        G[row][ch] = sum_j M[row][j] * Q[j][ch]        (64 texel rows x 32 samples x 32 channels)
// with M the sparse matrix of corner coefficients -- a GEMM on the matrix cores.  Every distinct texel of the tile gets a
// row of M (the 4 corners of one sample never share one, so M is filled with plain stores): a texel is claimed with one
// integer LDS CAS per reference in a 16 x 16 torus hash table of the texel coordinates, and a reference that loses its
// entry to a different texel (footprint wider than 16 texels) falls back to direct global atomics.  The MFMA C/D layout
// (lane <-> channel, register <-> row) is exactly what a coalesced 128-byte global atomic needs, so every
// occupied row is flushed with ONE atomic instruction per half-wave straight from the accumulator registers.
// Everything except the rare lost-reference path is straight-line code (no per-reference branches: inactive references
// CAS a per-lane dummy word and store to a dump row of M), so that plane p's MFMAs (one wave per SIMD: nothing else would
// fill them) run over plane p+1's corner set-up, claims and M fill.
#define MS XS  // row stride of M (floats): same conflict-free stride as the transposition scratch

// M region: either the fp32 matrix (65 rows x MS floats, EXACT) or its split-fp16 image -- two planes (hi, lo) of
// 65 rows x M16_RS halves (32 samples + pad: 80-byte rows keep the 16-byte A-operand reads spread over the banks)
#define M16_RS 40
#define M16_PLANE (65 * M16_RS)
#define SCATTER_M_FLOATS 2624 /* >= max(65 * MS, 2 * M16_PLANE / 2), multiple of 64 */
template <bool EXACT>
__device__ __forceinline__ void scatter_clear(float* M, int lane) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (EXACT) {  // 64 rows of the fp32 matrix (the dump row is never read)
#pragma unroll
        for (int g = 0; g < MS / 4; ++g) *reinterpret_cast<f32x4*>(M + lane * MS + 4 * g) = z;
    } else {
#pragma unroll
        for (int g = 0; g < SCATTER_M_FLOATS / 256; ++g) *reinterpret_cast<f32x4*>(M + (g * 64 + lane) * 4) = z;
        if (lane < (SCATTER_M_FLOATS % 256) / 4)
            *reinterpret_cast<f32x4*>(M + ((SCATTER_M_FLOATS / 256) * 64 + lane) * 4) = z;
    }
}

// LDS per wave: M = 64 rows + 1 dump row (stride MS), and SCATTER_TAG_INTS ints of which the first 32 are the dummy words
// (scatter_init_tags) and the next 96 the three planes' factor tables of the register-form B operand (sc2_regs_b: 32 floats
// per plane, 16-byte aligned; the rest is unused since the texel table moved behind the lost-reference lists).
#define SCATTER_TAG_INTS 160
__device__ __forceinline__ float* sc2_factor_table(int* tags, int pl) { return reinterpret_cast<float*>(tags + 32) + 32 * pl; }

struct PlaneRefs {  // the two corners (2hi, 2hi+1) of this lane's sample in one plane
    float c0, c1;   // coefficient (0: no reference), normalised per sample unless EXACT
    int o0, o1;     // absolute texel index (prompt and plane included)
    int h0, h1;     // entry of the texel table: 16x16 torus hash of the texel coordinates
    float qs;       // factor the sample's row of Q must be staged with (inverse of the coefficient normalisation)
};
// NORM: the sample's four coefficients are scaled by the power of two that brings the largest into [2^14, 2^15) -- the
// top of the fp16 range, as tt_mfma16.h does for every split operand -- and the sample's row of Q by its inverse:
// M Q is unchanged (exactly), column j of M and row j of Q belong to the same sample.
template <bool NORM>
__device__ __forceinline__ PlaneRefs plane_refs(const float (&coef)[4], const int (&aoff)[4], const int (&hs)[4],
                                                int hi) {
    PlaneRefs r;
    float cn = 1.f;
    r.qs = 1.f;
    if (NORM) {
        const float m = fmaxf(fmaxf(__builtin_fabsf(coef[0]), __builtin_fabsf(coef[1])),
                              fmaxf(__builtin_fabsf(coef[2]), __builtin_fabsf(coef[3])));
        int E = (int)(__builtin_bit_cast(unsigned, m) >> 23);
        E = E < 16 ? 16 : (E > 240 ? 240 : E);
        cn = __builtin_bit_cast(float, (unsigned)(268 - E) << 23);    // 2^(141 - E)
        r.qs = __builtin_bit_cast(float, (unsigned)(E - 14) << 23);   // 1 / cn
    }
    r.c0 = (hi ? coef[2] : coef[0]) * cn;
    r.c1 = (hi ? coef[3] : coef[1]) * cn;
    r.o0 = hi ? aoff[2] : aoff[0];
    r.o1 = hi ? aoff[3] : aoff[1];
    r.h0 = hi ? hs[2] : hs[0];
    r.h1 = hi ? hs[3] : hs[1];
    return r;
}
__device__ __forceinline__ void scatter_init_tags(int* tags, int lane) {
    if (lane < 32) tags[lane] = -2;  // the dummy words inactive references CAS: never empty, never equal to a texel index
}

// Column of M that sample s goes to.  fp32 matrix (EXACT): s itself.  Split-fp16 image: bits 2 and 3 of s exchanged -- the
// order in which the B operand comes out of the TRANSPOSED last product (tt_mfma16.h, SWAP): k-slot j of k-step ks of lane
// (ch, hi) is register 8 ks + j of that product = sample 16 ks + 8 (j >> 2) + 4 hi + (j & 3), and sc2_load_a hands the same
// slot the column 16 ks + 8 hi + j.  A permutation of the 32 samples inside the reduction: M Q is the same sum, added by the
// MFMA in another order (fp32 rounding of the sum only).
template <bool EXACT>
__device__ __forceinline__ int sc2_col(int s) {
    return EXACT ? s : ((s & ~12) | ((s & 4) << 1) | ((s & 8) >> 1));
}
// store / clear one coefficient of M (column i = sc2_col of this lane's sample; row 64 = dump row)
template <bool EXACT>
__device__ __forceinline__ void m_store(float* M, int row, int i, float c) {
    if (EXACT) {
        M[row * MS + i] = c;
    } else {
        half_t h, l;
        split16(c, h, l);
        half_t* Mh = reinterpret_cast<half_t*>(M);
        Mh[row * M16_RS + i] = h;
        Mh[M16_PLANE + row * M16_RS + i] = l;
    }
}
template <bool EXACT>
__device__ __forceinline__ void m_zero(float* M, int row, int i) {
    if (EXACT) {
        M[row * MS + i] = 0.f;
    } else {
        half_t* Mh = reinterpret_cast<half_t*>(M);
        Mh[row * M16_RS + i] = (half_t)0.f;
        Mh[M16_PLANE + row * M16_RS + i] = (half_t)0.f;
    }
}

// references that lost their table entry (tile footprint wider than the texel table: sparse rays) go straight to global
// memory, one half-wave per reference (lanes <-> channels: a coalesced 128-byte atomic each).
// stage_q(): called (wave-uniformly) only when the plane has a lost reference, before Qs is read -- the register form of
// the B operand writes its [sample][33] rows of Q there and then, so the common case never stages them.
template <class StageQ>
__device__ __forceinline__ void scatter_lost(const PlaneRefs& r, bool l0, bool l1, const float* Qs, float* Ls,
                                             __amdgpu_buffer_rsrc_t grsrc, int i, int hi, StageQ&& stage_q) {
    const float lc0 = l0 ? r.c0 : 0.f, lc1 = l1 ? r.c1 : 0.f;  // coefficient of a lost corner, else 0
    const unsigned long long bal = __ballot(__builtin_fabsf(lc0) + __builtin_fabsf(lc1) != 0.f);
    if (bal == 0) return;
    stage_q();
    float* Lc = Ls;                                 // [sample][4] coefficient of a lost corner, else 0
    int* Lo = reinterpret_cast<int*>(Ls + 32 * 4);  // [sample][4] absolute texel index
    Lc[4 * i + 2 * hi] = lc0;
    Lc[4 * i + 2 * hi + 1] = lc1;
    Lo[4 * i + 2 * hi] = r.o0;
    Lo[4 * i + 2 * hi + 1] = r.o1;
    // walk only the samples that lost something, two per step (one per half-wave)
    unsigned todo = (unsigned)(bal & 0xffffffffull) | (unsigned)(bal >> 32);
    while (todo) {
        const int s0 = __builtin_ctz(todo);
        todo &= todo - 1;
        int s1 = -1;
        if (todo) {
            s1 = __builtin_ctz(todo);
            todo &= todo - 1;
        }
        const int sidx2 = hi ? s1 : s0;
        if (sidx2 >= 0) {
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(Lc + 4 * sidx2);
            const i32x4 o4 = *reinterpret_cast<const i32x4*>(Lo + 4 * sidx2);
            const float v = Qs[sidx2 * 33 + i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned tex = c4[q] != 0.f ? (unsigned)o4[q] : ~0u;  // ~0: beyond num_records, dropped
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v * c4[q], grsrc, (int)((tex << 7) | (4u * (unsigned)i)),
                                                                0, 0);
            }
        }
    }
}

// =====================================================================================================================
// Texel table -> DENSE ranks -> short flush, up to 128 distinct texels per plane-tile (two 64-row passes).
//
// Measured / simulated (tools/scatter_sim.py, profiles/r06_scatter_*.txt): a plane-tile of the headline scene holds 25-34
// DISTINCT texels, one of the reference's sparse training renders 63-73 (up to 128).  (Rounds 2-5 hashed straight into 64
// rows and flushed all of them: profiles/experiments/README.md.)
//   * claims go into a 16 x 16 torus table (256 entries; 4 % of the training shape's references collide there, 0.1 % of
//     the headline's) -- one LDS CAS per reference;
//   * the distinct texels are RANKED: the winner of an entry (exactly one reference per distinct texel) takes the next rank
//     r < n (two ballots + mbcnt over the winner flags), copies the tag to ctag[r] and leaves r in the entry for the
//     references that share the texel;
//   * M row = rank.  Ranks 0..63 are combined and flushed by pass A, ranks 64..127 (n > 64: wave-uniform branch) by a
//     second pass over the SAME 64-row M buffer and accumulators (32 samples x 4 corners = 128 references: n <= 128 always);
//   * the flush issues 4 ceil(n / 8) atomic instructions, not 32 (wave-uniform branches per group of 8 rows;
//     ctag[n .. n+7] = -1 keeps the tail of the last group out of range).
// The table needs no double buffer: a plane's entries go back to empty right after they were ranked (DS
// operations of a wave execute in order), only the compacted tags (read by the flush after the next plane's claims) alternate.
// LDS per wave (ints, behind the lost-reference lists at Ls + 256; all inside the kernels' existing scratch):
//   htab[256] | ctag[2][136] | cdump[64]          dummies: tags[0..31] (scatter_init_tags)
#define SC2_HT 256
#define SC2_CT 136
#define SC2_INTS (SC2_HT + 2 * SC2_CT + 64)

struct Sc2State {
    int rx0, rx1;  // dense rank of the lane's two references; 255 = not in the table (inactive, or lost to another texel)
    bool l0, l1;   // not in the table (LOST if the coefficient is non-zero: scatter_lost tests that)
    int n;         // wave-uniform: distinct texels of this plane-tile in the table
};

// claims of one plane, ranking, compacted tags into ct[0 .. n-1] (+ 8 x -1), table back to empty.
// The WINNER of an entry (its CAS found it empty: exactly one reference per distinct texel) takes the next rank -- two
// ballots + mbcnt over the winner flags, no pass over the table --, leaves it in the entry (as -2 - rank: never "empty",
// never a texel index) for the references that share the texel to read, copies the tag to ct[rank], and puts the entry
// back to empty once everybody has read (DS operations of a wave execute in order).
// st (tuning build): per-wave counters [0] active references, [1] lost references, [2] plane-tiles
__device__ __forceinline__ Sc2State sc2_claim_rank(const PlaneRefs& r, int* htab, int* ct, int* cdump, int* dummy,
                                                   int lane, unsigned long long* st = nullptr) {
    Sc2State s;
    const bool a0 = r.c0 != 0.f, a1 = r.c1 != 0.f;
    int* const e0 = a0 ? htab + r.h0 : dummy;
    int* const e1 = a1 ? htab + r.h1 : dummy;
    const int old0 = atomicCAS(e0, -1, r.o0);
    const int old1 = atomicCAS(e1, -1, r.o1);
    const bool w0 = tt_eq_either(old0, -1, r.o0), w1 = tt_eq_either(old1, -1, r.o1);  // the entry holds this texel
    s.l0 = !w0;
    s.l1 = !w1;
    const bool m0 = old0 == -1, m1 = old1 == -1;
    const unsigned long long b0 = __ballot(m0), b1 = __ballot(m1);
    const int n0 = __popcll(b0);
    const int r0 = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b0, 0u));
    const int r1 = n0 + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b1, 0u));
    s.n = n0 + __popcll(b1);
    int* const x0 = m0 ? e0 : dummy;  // (a value <= -2 in a dummy word is as good as the -2 it starts with)
    int* const x1 = m1 ? e1 : dummy;
    *x0 = -2 - r0;
    *x1 = -2 - r1;
    *(m0 ? ct + r0 : cdump + lane) = r.o0;
    *(m1 ? ct + r1 : cdump + lane) = r.o1;
    *(lane < 8 ? ct + s.n + lane : cdump + lane) = -1;  // the tail of the last flush group: out of range, dropped
    const int q0 = -2 - *e0, q1 = -2 - *e1;
    *x0 = m0 ? -1 : -2;  // the table back to empty
    *x1 = m1 ? -1 : -2;
    s.rx0 = w0 ? q0 : 255;
    s.rx1 = w1 ? q1 : 255;
#ifdef TT_TUNING
    if (st) {  // wave-uniform values, flushed once per wave with the phase timers
        st[0] += __popcll(__ballot(a0)) + __popcll(__ballot(a1));
        st[1] += __popcll(__ballot((s.l0 ? r.c0 : 0.f) != 0.f)) + __popcll(__ballot((s.l1 ? r.c1 : 0.f) != 0.f));
        st[2] += 1;
    }
#endif
    return s;
}
// M rows of a lane's two references in pass A (ranks 0..63) / pass B (ranks 64..127); 64 = the dump row
__device__ __forceinline__ int sc2_row_a(int rx) { return rx < 64 ? rx : 64; }
__device__ __forceinline__ int sc2_row_b(int rx) {
    const unsigned d = (unsigned)(rx - 64);
    return (int)(d < 64u ? d : 64u);
}

// operands of the combine GEMM G[64 rows x 32 ch] = M[64 x 32 samples] Q[32 x 32]: A from the rows of M, B from Qs
struct ScA16 {
    h8_t ah[2][2], al[2][2];  // [row tile][k-step]: 8 samples 16 ks + 8 hi .. + 7 of row 32 m + i
};
struct ScB16 {
    float bs[2][8];  // raw (dead after sc2_split_b)
    h8_t bh[2], bl[2];
    float bun;
};
struct ScA32 {
    f32x4 a4[2][4];
};
struct ScB32 {
    float bq[16];
};
// (n: rows in use, wave-uniform -- the second row tile is read / multiplied only when n > 32)
__device__ __forceinline__ void sc2_load_a(const float* M, int i, int hi, int n, ScA16& A) {
    const half_t* Mh = reinterpret_cast<const half_t*>(M);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m == 1 && n <= 32) break;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const half_t* a = Mh + (32 * m + i) * M16_RS + 16 * ks + 8 * hi;
            A.ah[m][ks] = *reinterpret_cast<const h8_t*>(a);
            A.al[m][ks] = *reinterpret_cast<const h8_t*>(a + M16_PLANE);
        }
    }
}
__device__ __forceinline__ void sc2_load_a(const float* M, int i, int hi, int n, ScA32& A) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m == 1 && n <= 32) break;
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4)
            A.a4[m][t4] = *reinterpret_cast<const f32x4*>(M + (32 * m + i) * MS + 16 * hi + 4 * t4);
    }
}
__device__ __forceinline__ void sc2_load_b(const float* Qs, int i, int hi, ScB16& B) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) B.bs[ks][j] = Qs[(16 * ks + 8 * hi + j) * 33 + i];
}
__device__ __forceinline__ void sc2_load_b(const float* Qs, int i, int hi, ScB32& B) {
#pragma unroll
    for (int t = 0; t < 16; ++t) B.bq[t] = Qs[(t + 16 * hi) * 33 + i];
}
// The B operand straight from the registers of the transposed last product (qt[16]: lane (ch, hi), register r <-> sample
// (r&3) + 8(r>>2) + 4hi; raw accumulators) and the plane's factor table T[32] (per sample: the product's deferred factor
// times refs.qs, both powers of two, written by the lane that owns the sample): four broadcast ds_read_b128 and 16
// multiplies give the numbers the LDS round trip through Qs gave.  M's columns are in the matching order (sc2_col).
__device__ __forceinline__ void sc2_regs_b(const float* qt, const float* T, int hi, ScB16& B) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(T + 8 * g + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) B.bs[g >> 1][4 * (g & 1) + e] = qt[4 * g + e] * t4[e];
    }
}
// ... and the [sample][33] rows of Q that scatter_lost reads, from the same registers (16 conflict-free stores)
__device__ __forceinline__ void sc2_regs_stage_q(const float* qt, const float* T, float* Qs, int i, int hi) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(T + 8 * g + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) Qs[LIDX(4 * g + e, hi) * 33 + i] = qt[4 * g + e] * t4[e];
    }
}
// The hand-over of the last product to the combine GEMM's B operand.  `tile`: the 16 registers of that product that belong to
// plane pl; qs: the plane's PlaneRefs::qs of this lane's sample.  Qs: 32 rows of Q, stride 33; tags: scatter_init_tags.
//   fp32 form (EXACT; tile = the SAMPLE's row of Q): hand_over stages the row, scaled by qs, into Qs (the previous plane's B
//     operand is in registers by then; one row pointer: profiles/bwd_handover_ab.txt), load_b reads the operand back.
//   register form (tile = the transposed tile of sc2_regs_b): hand_over stores ONE number, the product's deferred factor times
//     qs, into slot i of the plane's factor table; stage_q writes the plane's rows of Q, only when it has a lost reference.
template <bool EXACT>
struct ScatterQ {
    float* Qs;
    int* tags;
    int i, hi;
    __device__ __forceinline__ void hand_over(int pl, const float* tile, float factor, float qs) const {
        if constexpr (EXACT) {
            float* const row = Qs + i * 33;
#pragma unroll
            for (int r = 0; r < 16; ++r) row[LIDX(r, hi)] = tile[r] * qs;
        } else {  // (both half-waves: the same value)
            sc2_factor_table(tags, pl)[i] = factor * qs;
        }
    }
    template <class BOp>
    __device__ __forceinline__ void load_b(int pl, const float* tile, BOp& B) const {
        if constexpr (EXACT)
            sc2_load_b(Qs, i, hi, B);
        else
            sc2_regs_b(tile, sc2_factor_table(tags, pl), hi, B);
    }
    __device__ __forceinline__ void stage_q(int pl, const float* tile) const {
        if constexpr (!EXACT) sc2_regs_stage_q(tile, sc2_factor_table(tags, pl), Qs, i, hi);
    }
};
__device__ __forceinline__ void sc2_split_b(ScB32&) {}
// per-channel normalisation of the B operand to the top of the fp16 range (column = this lane and lane ^ 32) + split
__device__ __forceinline__ void sc2_split_b(ScB16& B) {
    const float (&bs)[2][8] = B.bs;
    float mx = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, __builtin_fabsf(bs[ks][j]));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    int E = (int)(__builtin_bit_cast(unsigned, mx) >> 23);
    E = E < 16 ? 16 : (E > 240 ? 240 : E);
    const float bsc = __builtin_bit_cast(float, (unsigned)(268 - E) << 23);
    B.bun = __builtin_bit_cast(float, (unsigned)(E - 14) << 23);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x0 = bs[ks][2 * j] * bsc, x1 = bs[ks][2 * j + 1] * bsc;
            h2_t ph, pq;
            split_pair(x0, x1, ph, pq);
            B.bh[ks][2 * j] = ph.x;
            B.bh[ks][2 * j + 1] = ph.y;
            B.bl[ks][2 * j] = pq.x;
            B.bl[ks][2 * j + 1] = pq.y;
        }
}
__device__ __forceinline__ void sc2_gemm(const ScA16& A, const ScB16& B, int n, f32x16& acc0, f32x16& acc1) {
    acc0 = f32x16 ZERO16;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.ah[0][ks], B.bh[ks], acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.ah[0][ks], B.bl[ks], acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.al[0][ks], B.bh[ks], acc0, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] *= B.bun;
    if (n > 32) {
        acc1 = f32x16 ZERO16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.ah[1][ks], B.bh[ks], acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.ah[1][ks], B.bl[ks], acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.al[1][ks], B.bh[ks], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[r] *= B.bun;
    }
}
__device__ __forceinline__ void sc2_gemm(const ScA32& A, const ScB32& B, int n, f32x16& acc0, f32x16& acc1) {
    acc0 = f32x16 ZERO16;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a4[0][t >> 2][t & 3], B.bq[t], acc0, 0, 0, 0);
    if (n > 32) {
        acc1 = f32x16 ZERO16;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(A.a4[1][t >> 2][t & 3], B.bq[t], acc1, 0, 0, 0);
    }
}
// flush rows 0 .. n-1 (rounded up to a group of 8): one 128-byte atomic per row pair, straight from the accumulators
// (row of register 4 g + e = LIDX: e + 8 g + 4 hi); ct: the compacted tags of these rows
__device__ __forceinline__ void sc2_flush(const f32x16& acc0, const f32x16& acc1, const int* ct, int n,
                                          __amdgpu_buffer_rsrc_t grsrc, unsigned lane_b, int hi) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (n > 8 * g) {
            const i32x4 k0 = *reinterpret_cast<const i32x4*>(ct + 8 * g + 4 * hi);
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2)
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc0[4 * g + e2], grsrc,
                                                                (int)(((unsigned)k0[e2] << 7) | lane_b), 0, 0);
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (n > 32 + 8 * g) {
            const i32x4 k1 = *reinterpret_cast<const i32x4*>(ct + 32 + 8 * g + 4 * hi);
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2)
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc1[4 * g + e2], grsrc,
                                                                (int)(((unsigned)k1[e2] << 7) | lane_b), 0, 0);
        }
    }
}

// What both scatter drivers start from: the gradient copy as a buffer resource, this lane's places in the per-wave tables
// (sq.tags: the 32 dummy words, scatter_init_tags; Ls: 256 floats of lost-reference lists, followed by SC2_INTS ints), the
// texel table cleared (its LDS is shared with the other phases of the tile step) and this lane's column of M.
struct ScatterCtx {
    __amdgpu_buffer_rsrc_t grsrc;
    unsigned lane_b;
    int lane, mc;
    int *dummy, *htab, *ctag, *cdump;
};
template <bool EXACT>
__device__ __forceinline__ ScatterCtx scatter_ctx(float* __restrict__ grad, unsigned grad_bytes, const ScatterQ<EXACT>& sq, float* Ls) {
    ScatterCtx cx;
    // BUFFER atomics with a 32-bit BYTE offset (texel << 7 | channel * 4) from the gradient copy: a tag of -1 gives the
    // offset 0xFFFFFF80 + 4 ch, beyond num_records (the host refuses gradient buffers of 4 GB - 256 B and more), and the
    // hardware range check drops the atomic -- no compare, no exec-mask branch per row.
    cx.grsrc = __builtin_amdgcn_make_buffer_rsrc(grad, 0, (int)grad_bytes, 0x00020000);
    cx.lane_b = 4u * (unsigned)sq.i;
    cx.lane = sq.i + 32 * sq.hi;
    cx.dummy = sq.tags + sq.i;
    cx.htab = reinterpret_cast<int*>(Ls + 256);
    cx.ctag = cx.htab + SC2_HT;
    cx.cdump = cx.ctag + 2 * SC2_CT;
    *reinterpret_cast<i32x4*>(cx.htab + 4 * cx.lane) = i32x4{-1, -1, -1, -1};
    cx.mc = sc2_col<EXACT>(sq.i);
    return cx;
}

// corners(pl, refs): the kernel's corner set-up of plane pl for this lane's sample, ending in plane_refs<!EXACT>.
// tile(pl): the 16 registers of the last product that belong to plane pl; factor: that product's deferred factor (1 in the
// fp32 form) -- what sq, the kernel's ScatterQ, hands over (both by reference, as the kernels' lambdas captured them: by value
// hipcc allocates the kernels differently, profiles/bwd_handover_ab.txt).  M: all-zero on entry and on exit.  Ls: ScatterCtx.
// Pipeline per plane p:  operands A(p) -> registers, M rows back to zero, [n > 64: rows of pass B -> M]; prep(p+1) = corners
//   + hand-over; GEMM A(p); [pass B: flush A(p), operands B(p) -> registers, M back to zero]; claims + ranks(p+1), lost
//   references of p+1 (under the MFMAs); [pass B: GEMM B(p), flush B(p) | else: flush A(p)]; rows of pass A(p+1) -> M.
template <bool EXACT, class Corners, class Tile>
__device__ __forceinline__ void scatter_planes(float* __restrict__ grad, unsigned grad_bytes, const ScatterQ<EXACT>& sq, float* M,
                                               float* Ls, Corners&& corners, Tile&& tile, const float& factor,
                                               unsigned long long* st = nullptr) {
    float* const Qs = sq.Qs;
    const int i = sq.i, hi = sq.hi;
    auto prep = [&](int pl, PlaneRefs& refs) {
        corners(pl, refs);
        sq.hand_over(pl, tile(pl), factor, refs.qs);
    };
    typedef typename std::conditional<EXACT, ScA32, ScA16>::type AOp;
    typedef typename std::conditional<EXACT, ScB32, ScB16>::type BOp;
#ifdef TT_TUNING  // sub-phase cycles of the epilogue (st[3..5] = operands+prep / GEMM+claim / flush+reset+lost)
    unsigned long long sp_t = __builtin_amdgcn_s_memtime();
#define TT_SUBPHASE(k)                                                    \
    do {                                                                  \
        if (st) {                                                         \
            __builtin_amdgcn_sched_barrier(0);                            \
            const unsigned long long t_now = __builtin_amdgcn_s_memtime(); \
            st[k] += t_now - sp_t;                                        \
            sp_t = t_now;                                                 \
            __builtin_amdgcn_sched_barrier(0);                            \
        }                                                                 \
    } while (0)
#else
#define TT_SUBPHASE(k) \
    do {               \
    } while (0)
#endif
    const ScatterCtx cx = scatter_ctx<EXACT>(grad, grad_bytes, sq, Ls);  // (inside sub-phase 3)
    PlaneRefs rc, rn;
    Sc2State sc, sn;
    prep(0, rc);
    sc = sc2_claim_rank(rc, cx.htab, cx.ctag, cx.cdump, cx.dummy, cx.lane, st);
    scatter_lost(rc, sc.l0, sc.l1, Qs, Ls, cx.grsrc, i, hi, [&]() { sq.stage_q(0, tile(0)); });
    m_store<EXACT>(M, sc2_row_a(sc.rx0), cx.mc, rc.c0);
    m_store<EXACT>(M, sc2_row_a(sc.rx1), cx.mc, rc.c1);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const int* const ct = cx.ctag + SC2_CT * (pl & 1);
        int* const ct_next = cx.ctag + SC2_CT * ((pl + 1) & 1);
        const bool pass_b = sc.n > 64;  // wave-uniform
        f32x16 acc0, acc1;
        AOp A;
        BOp B;
        sc2_load_a(M, i, hi, sc.n, A);
        m_zero<EXACT>(M, sc2_row_a(sc.rx0), cx.mc);
        m_zero<EXACT>(M, sc2_row_a(sc.rx1), cx.mc);
        if (pass_b) {
            m_store<EXACT>(M, sc2_row_b(sc.rx0), cx.mc, rc.c0);
            m_store<EXACT>(M, sc2_row_b(sc.rx1), cx.mc, rc.c1);
        }
        sq.load_b(pl, tile(pl), B);
        if (pl < 2) prep(pl + 1, rn);
        sc2_split_b(B);
        sc2_gemm(A, B, sc.n, acc0, acc1);
        TT_SUBPHASE(3);
        if (pass_b) {  // (rare on dense rays: the first pass is flushed before the next plane's claims)
            sc2_flush(acc0, acc1, ct, 64, cx.grsrc, cx.lane_b, hi);
            sc2_load_a(M, i, hi, sc.n - 64, A);
            m_zero<EXACT>(M, sc2_row_b(sc.rx0), cx.mc);
            m_zero<EXACT>(M, sc2_row_b(sc.rx1), cx.mc);
        }
        if (pl < 2) sn = sc2_claim_rank(rn, cx.htab, ct_next, cx.cdump, cx.dummy, cx.lane, st);
        TT_SUBPHASE(4);
        if (pass_b) {
            sc2_gemm(A, B, sc.n - 64, acc0, acc1);
            sc2_flush(acc0, acc1, ct + 64, sc.n - 64, cx.grsrc, cx.lane_b, hi);
        } else {
            sc2_flush(acc0, acc1, ct, sc.n, cx.grsrc, cx.lane_b, hi);
        }
        if (pl < 2) {
            scatter_lost(rn, sn.l0, sn.l1, Qs, Ls, cx.grsrc, i, hi, [&]() { sq.stage_q(pl + 1, tile(pl + 1)); });
            m_store<EXACT>(M, sc2_row_a(sn.rx0), cx.mc, rn.c0);
            m_store<EXACT>(M, sc2_row_a(sn.rx1), cx.mc, rn.c1);
            rc = rn;
            sc = sn;
        }
        TT_SUBPHASE(5);
    }
}

// ---- one plane only (single-plane tile steps: the plane mask of the gather has one bit, tt_device.h) -------------------------
// The other two planes' coefficients are exact zeros there: their claims are all inactive, n = 0, nothing is flushed.  This
// is plane `pl` (wave-uniform, known at run time) of scatter_planes with nothing to overlap it with, so the pieces run in
// their plain order: corners, hand-over, claims + ranks, lost references, rows -> M; operands -> registers, M back to zero; GEMM; flush
// (and the second 64-row pass when n > 64).  Same arguments and the same state on exit as scatter_planes: M all-zero, the
// table empty, the dummy words <= -2.
template <bool EXACT, class Corners>
__device__ __forceinline__ void scatter_one_plane(float* __restrict__ grad, unsigned grad_bytes, const ScatterQ<EXACT>& sq, float* M,
                                                  float* Ls, int pl, Corners&& corners, const float* tile,
                                                  const float& factor, unsigned long long* st = nullptr) {
    float* const Qs = sq.Qs;
    const int i = sq.i, hi = sq.hi;
    const ScatterCtx cx = scatter_ctx<EXACT>(grad, grad_bytes, sq, Ls);
    typename std::conditional<EXACT, ScA32, ScA16>::type A;
    typename std::conditional<EXACT, ScB32, ScB16>::type B;
    PlaneRefs rc;
    corners(pl, rc);
    sq.hand_over(pl, tile, factor, rc.qs);
    const Sc2State sc = sc2_claim_rank(rc, cx.htab, cx.ctag, cx.cdump, cx.dummy, cx.lane, st);
    scatter_lost(rc, sc.l0, sc.l1, Qs, Ls, cx.grsrc, i, hi, [&]() { sq.stage_q(pl, tile); });
    m_store<EXACT>(M, sc2_row_a(sc.rx0), cx.mc, rc.c0);
    m_store<EXACT>(M, sc2_row_a(sc.rx1), cx.mc, rc.c1);
    const bool pass_b = sc.n > 64;  // wave-uniform
    f32x16 acc0, acc1;
    sc2_load_a(M, i, hi, sc.n, A);
    m_zero<EXACT>(M, sc2_row_a(sc.rx0), cx.mc);
    m_zero<EXACT>(M, sc2_row_a(sc.rx1), cx.mc);
    if (pass_b) {
        m_store<EXACT>(M, sc2_row_b(sc.rx0), cx.mc, rc.c0);
        m_store<EXACT>(M, sc2_row_b(sc.rx1), cx.mc, rc.c1);
    }
    sq.load_b(pl, tile, B);
    sc2_split_b(B);
    sc2_gemm(A, B, sc.n, acc0, acc1);
    if (pass_b) {
        sc2_flush(acc0, acc1, cx.ctag, 64, cx.grsrc, cx.lane_b, hi);
        sc2_load_a(M, i, hi, sc.n - 64, A);
        m_zero<EXACT>(M, sc2_row_b(sc.rx0), cx.mc);
        m_zero<EXACT>(M, sc2_row_b(sc.rx1), cx.mc);
        sc2_gemm(A, B, sc.n - 64, acc0, acc1);
        sc2_flush(acc0, acc1, cx.ctag + 64, sc.n - 64, cx.grsrc, cx.lane_b, hi);
    } else {
        sc2_flush(acc0, acc1, cx.ctag, sc.n, cx.grsrc, cx.lane_b, hi);
    }
}

// ---- texture half: parameters of tt_backward_tex.hip ----
struct BwdTexParams {
    const float* packed;
    MlpPtrs w;
    const float* rays_o;
    const float* rays_d;
    const float* t_starts;
    const float* t_ends;
    tt_render_cfg cfg;
    const float* weights;
    const float* features;
    const float* g_rgb;
    const float* g_features;
    TileGeom geom;
    long long n_items;
    int* queue;  // per-XCD item counters (tt_queue_counters)
    int n_copies;
    float* grad_packed;
    MlpGradPtrs grads;
    unsigned long long* phase_cycles;  // tuning build only (TT_PHASE), else null
};

// =====================================================================================================
// host side
// =====================================================================================================
// the scatter addresses texels with 32-bit byte offsets from the (copy of the) gradient buffer
static inline bool grad_buffer_too_large(const tt_render_cfg* cfg) {
    return (long long)cfg->n_prompts * 6 * cfg->plane_h * cfg->plane_w * TT_C * 4 >= (1LL << 32) - 256;
}

#ifdef TT_TUNING
extern unsigned long long* g_phase_cycles;  // tt_backward.hip (tuning build only)
#endif
// ---- per-launch magnitude bounds for the fp16 outer products (tt_host.h: TT_SLOT_BOUNDS) --------------------------
// max |x| over flat float4 data, raised into *out with one atomicMax per workgroup (non-negative floats order like their
// bit patterns; NaN / Inf patterns order above every finite value and end up clamped by wg16_scale).
static __global__ __launch_bounds__(256) void k_absmax4(const f32x4* __restrict__ x, long long seg4, long long seg_stride4,
                                                 unsigned* __restrict__ out0, unsigned* __restrict__ out1) {
    // gridDim.y segments of seg4 float4 elements that start seg_stride4 apart; four independent loads in flight per lane.
    // out0 <- max |.x| (and, if out1 is null, of the other three components as well); out1 <- max |.y|, |.z|, |.w|
    const f32x4* seg = x + (long long)blockIdx.y * seg_stride4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    float m0 = 0.f, m1 = 0.f;
    long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (; e + 3 * stride < seg4; e += 4 * stride) {
        const f32x4 a = seg[e], b = seg[e + stride], c = seg[e + 2 * stride], d = seg[e + 3 * stride];
        m0 = fmaxf(fmaxf(m0, __builtin_fabsf(a[0])), fmaxf(__builtin_fabsf(b[0]), fmaxf(__builtin_fabsf(c[0]), __builtin_fabsf(d[0]))));
#pragma unroll
        for (int k = 1; k < 4; ++k)
            m1 = fmaxf(fmaxf(m1, __builtin_fabsf(a[k])), fmaxf(__builtin_fabsf(b[k]), fmaxf(__builtin_fabsf(c[k]), __builtin_fabsf(d[k]))));
    }
    for (; e < seg4; e += stride) {
        const f32x4 v = seg[e];
        m0 = fmaxf(m0, __builtin_fabsf(v[0]));
        m1 = fmaxf(m1, fmaxf(__builtin_fabsf(v[1]), fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3]))));
    }
    if (!out1) m0 = fmaxf(m0, m1);
    __shared__ unsigned w[2];
    if (threadIdx.x < 2) w[threadIdx.x] = 0u;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        m0 = fmaxf(m0, __shfl_xor(m0, o));
        m1 = fmaxf(m1, __shfl_xor(m1, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&w[0], __builtin_bit_cast(unsigned, m0));
        atomicMax(&w[1], __builtin_bit_cast(unsigned, m1));
    }
    __syncthreads();
    // same-address atomics serialise at ~11 ns each (4096 workgroups x 2 words: 90 us, measured): the words only grow, so
    // a workgroup first LOOKS (L2-coherent load) and raises a word only if that changes it
    if (threadIdx.x == 0) {
        if (w[0] > __hip_atomic_load(out0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out0, w[0]);
        if (out1 && w[1] > __hip_atomic_load(out1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out1, w[1]);
    }
}
// flat float data of any length (g_rgb: n_rays x 3, g_features: n x 3): scalar loads
static __global__ __launch_bounds__(256) void k_absmax1(const float* __restrict__ x, long long n, unsigned* __restrict__ out) {
    float m = 0.f;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        m = fmaxf(m, __builtin_fabsf(x[e]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ unsigned w;
    if (threadIdx.x == 0) w = 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) atomicMax(&w, __builtin_bit_cast(unsigned, m));
    __syncthreads();
    if (threadIdx.x == 0 && w > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, w);
}
static inline unsigned absmax_blocks(long long n) {  // >= 8 elements per thread, at most 1024 workgroups
    long long b = (n + 256 * 8 - 1) / (256 * 8);
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}
// max |texel| of planes first_plane .. first_plane + 2 of every prompt of the packed buffer
static inline void launch_planes_bound(const float* packed, const tt_render_cfg& cfg, int first_plane, unsigned* out,
                                hipStream_t s) {
    const long long hw4 = (long long)cfg.plane_h * cfg.plane_w * TT_C / 4;  // float4s per plane
    hipLaunchKernelGGL(k_absmax4, dim3(absmax_blocks(3 * hw4), (unsigned)cfg.n_prompts), dim3(256), 0, s,
                       reinterpret_cast<const f32x4*>(packed) + first_plane * hw4, 3 * hw4, 6 * hw4, out,
                       (unsigned*)nullptr);
}

// outer products on the fp16 pipe: both split modes (the fp32 MFMA mode uses fp32 outer products)
static inline bool use_wg16(const tt_render_cfg& cfg) { return !(cfg.flags & TT_R_EXACT_F32); }

static inline int points_cfg(tt_render_cfg* c, int32_t n_batch, int64_t n_points, int32_t n_prompts,
                      int32_t views_per_prompt, int32_t plane_h, int32_t plane_w, float radius, float sdf_bias_radius,
                      int32_t grad_copies, int32_t q_flags) {
    if (!tt_points_counts_ok(n_batch, n_points, n_prompts, views_per_prompt, q_flags) || n_points > 0x7fffffffLL)
        return TT_ERR_BAD_ARG;
    c->n_prompts = n_prompts;
    c->views_per_prompt = views_per_prompt;
    c->plane_h = plane_h;
    c->plane_w = plane_w;
    c->rays_per_view = (int32_t)n_points;
    c->n_samples = 1;
    c->n_rays = (int64_t)n_batch * n_points;
    c->radius = radius;
    c->sdf_bias_radius = sdf_bias_radius;
    c->inv_std = 1.f;  // unused by the decode kernels
    c->inv_std_dev = nullptr;
    c->stats = nullptr;
    c->cos_anneal_ratio = 1.f;
    c->rgb_grad_shrink = 1.f;
    c->flags = (q_flags & TT_Q_EXACT_F32) ? TT_R_EXACT_F32 : ((q_flags & TT_Q_SPLIT2) ? TT_R_SPLIT2 : 0);
    c->image_w = 0;
    c->tile_sb = 1;
    c->tile_chunk = 0;
    c->grad_copies = grad_copies;
    c->skip_eps_tex = 0.f;
    c->skip_eps_geo = 0.f;
    return tt_validate_cfg(c);
}

