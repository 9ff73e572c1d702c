// tt_scan.h -- the two-level exclusive scan shared by the compaction kernels (tt_isosurface.hip, tt_mesh.hip):
// an in-block wave/LDS scan of two 16-bit counters packed in one 32-bit word (the caller's kernel), then one block
// that scans the block totals in 64 bits (low half: first counter, high half: second) in fixed order.  No atomics:
// identical inputs give bit-identical offsets.
#pragma once
#include <hip/hip_runtime.h>

#define TT_SCAN_BLOCK 1024

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T x = __shfl_up(v, d, 64);
        if (lane >= d) v += x;
    }
    return v;
}

// One block of TT_SCAN_BLOCK threads: boff[b] = exclusive prefix of the unpacked block totals bsum[b] (lo | hi << 16
// -> lo | hi << 32); the grand totals go to tot[0..1] and out_totals[0..1] (lo, hi).
__device__ __forceinline__ void tt_scan_block_totals(const unsigned* __restrict__ bsum, int nblk,
                                                     unsigned long long* __restrict__ boff, int* __restrict__ tot,
                                                     int* __restrict__ out_totals) {
    __shared__ unsigned long long wave_tot[TT_SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (int base = 0; base < nblk; base += TT_SCAN_BLOCK) {
        const int b = base + threadIdx.x;
        const unsigned s = b < nblk ? bsum[b] : 0u;
        const unsigned long long v = (unsigned long long)(s & 0xffffu) | ((unsigned long long)(s >> 16) << 32);
        const unsigned long long incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < TT_SCAN_BLOCK / 64; ++q) {
            before += q < wave ? wave_tot[q] : 0ull;
            total += wave_tot[q];
        }
        if (b < nblk) boff[b] = carry + before + incl - v;
        carry += total;
        __syncthreads();  // wave_tot is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        const int lo = (int)(carry & 0xffffffffull), hi = (int)(carry >> 32);
        tot[0] = lo;
        tot[1] = hi;
        out_totals[0] = lo;
        out_totals[1] = hi;
    }
}
