// tt_scan.h -- the only prefix scans and the fixed-order wave sum of the mesh stages (tt_isosurface.hip, tt_mesh.hip,
// tt_simplify.hip, tt_raster.hip, tt_uv.hip):
//   wave_inclusive_scan / tt_block_exclusive_scan   the building blocks
//   tt_wave_sum            64-lane sum by a fixed shuffle tree
//   tt_exclusive_scan      exclusive scan of an int / long long array in three launches; the caller owns the input, the
//                          block-sum scratch (tt_xscan_blocks(n) elements) and the slot of the total
// The two-counter compaction (both scan levels, its workspace sections, the decoding of its result) is tt_compact.h, on
// these blocks; its callers own their counts and the slot of the two totals.  Fixed summation order (lanes, then waves,
// then blocks, each ascending) and no atomics: identical inputs give bit-identical offsets.
#pragma once
#include <hip/hip_runtime.h>

#define TT_SCAN_BLOCK 1024  // threads of a one-block scan of block totals (tt_compact.h)

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T x = __shfl_up(v, d, 64);
        if (lane >= d) v += x;
    }
    return v;
}

// sum over the 64 lanes in a fixed order (the result is valid in lane 0)
template <typename T>
__device__ __forceinline__ T tt_wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// Exclusive scan of one value per thread over a block of BLOCK threads (all of them must call it); returns the prefix,
// *total = the block's sum.  There is no barrier after the wave totals are read: a kernel that calls the same
// instantiation again (a loop) puts a __syncthreads() between the calls, or the next call's writes race these reads.
template <typename T, int BLOCK>
__device__ __forceinline__ T tt_block_exclusive_scan(T v, T* total) {
    __shared__ T wave_tot[BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_scan(v, lane);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    T before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < BLOCK / 64; ++q) {
        before += q < wave ? wave_tot[q] : T(0);
        tot += wave_tot[q];
    }
    *total = tot;
    return before + incl - v;
}

// ---------------------------------------------------------------------------------------------------------------
// exclusive scan of n elements of T (int, long long): per-block sums, one block scans them, apply
#define TT_XSCAN_BLOCK 256
#define TT_XSCAN_ITEMS 4  // elements per thread
#define TT_XSCAN_SPAN (TT_XSCAN_BLOCK * TT_XSCAN_ITEMS)

template <typename T>
__global__ __launch_bounds__(TT_XSCAN_BLOCK) void k_xscan_reduce(const T* __restrict__ in, long long n,
                                                                 T* __restrict__ bsum) {
    const long long base = (long long)blockIdx.x * TT_XSCAN_SPAN + threadIdx.x * TT_XSCAN_ITEMS;
    T v = 0;
#pragma unroll
    for (int k = 0; k < TT_XSCAN_ITEMS; ++k) v += base + k < n ? in[base + k] : T(0);
    T tot;
    tt_block_exclusive_scan<T, TT_XSCAN_BLOCK>(v, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one block: the block sums scanned in place, in chunks of TT_XSCAN_BLOCK with a running carry; total[0] = their sum
template <typename T>
__global__ __launch_bounds__(TT_XSCAN_BLOCK) void k_xscan_blocks(T* __restrict__ bsum, long long nblk,
                                                                 T* __restrict__ total) {
    T carry = 0;
    for (long long base = 0; base < nblk; base += TT_XSCAN_BLOCK) {
        const long long i = base + threadIdx.x;
        const T v = i < nblk ? bsum[i] : T(0);
        T tot;
        const T ex = tt_block_exclusive_scan<T, TT_XSCAN_BLOCK>(v, &tot);
        if (i < nblk) bsum[i] = carry + ex;
        carry += tot;
        __syncthreads();  // the scan's wave totals are rewritten by the next chunk
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// in and out may be the same array (hence no __restrict__ on them): a thread reads its elements before it writes them
template <typename T>
__global__ __launch_bounds__(TT_XSCAN_BLOCK) void k_xscan_apply(const T* in, long long n, const T* __restrict__ bsum,
                                                                T* out) {
    const long long base = (long long)blockIdx.x * TT_XSCAN_SPAN + threadIdx.x * TT_XSCAN_ITEMS;
    T c[TT_XSCAN_ITEMS], v = 0;
#pragma unroll
    for (int k = 0; k < TT_XSCAN_ITEMS; ++k) {
        c[k] = base + k < n ? in[base + k] : T(0);
        v += c[k];
    }
    T tot;
    T run = bsum[blockIdx.x] + tt_block_exclusive_scan<T, TT_XSCAN_BLOCK>(v, &tot);
#pragma unroll
    for (int k = 0; k < TT_XSCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = run;
        run += c[k];
    }
}

static inline long long tt_xscan_blocks(long long n) { return (n + TT_XSCAN_SPAN - 1) / TT_XSCAN_SPAN; }

// out[i] = sum of in[0 .. i) for i < n (n >= 1), total[0] = the sum of all n; everything in device memory, on stream s.
// In place (out == in) is allowed.  total is written before out: it may be out + n (the rasterizer's offs[n]) or any
// other address outside in / out / bsum.  bsum: scratch of tt_xscan_blocks(n) elements.
template <typename T>
static void tt_exclusive_scan(const T* in, long long n, T* out, T* bsum, T* total, hipStream_t s) {
    const long long nb = tt_xscan_blocks(n);
    hipLaunchKernelGGL(k_xscan_reduce<T>, dim3((unsigned)nb), dim3(TT_XSCAN_BLOCK), 0, s, in, n, bsum);
    hipLaunchKernelGGL(k_xscan_blocks<T>, dim3(1), dim3(TT_XSCAN_BLOCK), 0, s, bsum, nb, total);
    hipLaunchKernelGGL(k_xscan_apply<T>, dim3((unsigned)nb), dim3(TT_XSCAN_BLOCK), 0, s, in, n, (const T*)bsum, out);
}
