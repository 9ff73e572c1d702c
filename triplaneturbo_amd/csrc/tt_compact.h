// tt_compact.h -- the one two-counter stream compaction of the mesh stages (tt_isosurface.hip: vertices | triangles,
// tt_mesh.hip: kept vertices | kept faces, tt_simplify.hip: marked clusters | kept faces).  Item i adds a count to a
// low and to a high output stream; the result is its exclusive offset in both streams and the two grand totals (the host
// reads those 8 bytes and sizes the outputs: count -> read-back -> emit).  Two launches:
//   first level    a block of TT_COMPACT_BLOCK items scans both counts packed in one 32-bit word, lo | hi << 16
//                  (tt_compact2_first_level from the caller's kernel, or k_compact2_flags for two 0/1 byte arrays)
//   second level   k_compact2_blocks: one block scans the block totals in 64 bits, lo | hi << 32
// The invariants of the packing live here and nowhere else: carve, first level and lookups share TT_COMPACT_BLOCK; a
// block's total fits 16 bits per counter (the first level asserts TT_COMPACT_BLOCK x MAX_COUNT < 65536); bsum holds
// 16-bit halves, boff 32-bit halves, and tt_compact2_lo / tt_compact2_hi are the only decoders.  Fixed summation order
// and no atomics (tt_scan.h): identical inputs give bit-identical offsets.
#pragma once
#include "tt_host.h"
#include "tt_scan.h"

#define TT_COMPACT_BLOCK TT_ITEM_BLOCK

struct TtCompact2 {
    int* local;                // [n] in-block exclusive prefix: lo | hi << 16
    unsigned* bsum;            // [nblk] block totals, same packing
    unsigned long long* boff;  // [nblk] block offsets: lo | hi << 32
    int* tot;                  // [2] grand totals (lo, hi): a slot of the caller's workspace
    int n, nblk;               // items, blocks of TT_COMPACT_BLOCK of them
};

// the sections of a compaction of n items; c may carve from a null base for the size alone
static inline TtCompact2 tt_compact2_carve(TtCarver& c, long long n, int* tot) {
    TtCompact2 k;
    k.n = (int)n;
    k.nblk = (int)tt_grid(n);
    k.local = c.take<int>(k.n);
    k.bsum = c.take<unsigned>(k.nblk);
    k.boff = c.take<unsigned long long>(k.nblk);
    k.tot = tot;
    return k;
}

// First level: every thread of a TT_COMPACT_BLOCK-thread block of an nblk-block grid calls it with the two counts of
// item blockIdx.x * TT_COMPACT_BLOCK + threadIdx.x (0, 0 past n), each at most MAX_COUNT.
template <int MAX_COUNT>
__device__ __forceinline__ void tt_compact2_first_level(const TtCompact2& c, unsigned lo, unsigned hi) {
    static_assert(TT_COMPACT_BLOCK * MAX_COUNT < 65536, "a block's total must fit 16 bits per counter");
    const int i = blockIdx.x * TT_COMPACT_BLOCK + threadIdx.x;
    unsigned total;
    const unsigned before = tt_block_exclusive_scan<unsigned, TT_COMPACT_BLOCK>(lo | (hi << 16), &total);
    if (i < c.n) c.local[i] = (int)before;
    if (threadIdx.x == 0) c.bsum[blockIdx.x] = total;
}

// first level for two arrays of 0/1 flags, lo_flag[n_lo] and hi_flag[n_hi] (a template: only its users carry a copy)
template <typename Flag>
__global__ __launch_bounds__(TT_COMPACT_BLOCK) void k_compact2_flags(const Flag* __restrict__ lo_flag, int n_lo,
                                                                     const Flag* __restrict__ hi_flag, int n_hi,
                                                                     TtCompact2 c) {
    const int i = blockIdx.x * TT_COMPACT_BLOCK + threadIdx.x;
    const unsigned lo = i < n_lo ? (unsigned)(lo_flag[i] != 0) : 0u, hi = i < n_hi ? (unsigned)(hi_flag[i] != 0) : 0u;
    tt_compact2_first_level<1>(c, lo, hi);
}

// Second level, one block of TT_SCAN_BLOCK threads: boff[b] = exclusive prefix of the unpacked block totals, in chunks
// of TT_SCAN_BLOCK blocks with a running carry; the grand totals go to tot[0..1] and out_totals[0..1] (lo, hi).
static __global__ __launch_bounds__(TT_SCAN_BLOCK) void k_compact2_blocks(TtCompact2 c, int* __restrict__ out_totals) {
    unsigned long long carry = 0;
    for (int base = 0; base < c.nblk; base += TT_SCAN_BLOCK) {
        const int b = base + threadIdx.x;
        const unsigned s = b < c.nblk ? c.bsum[b] : 0u;
        const unsigned long long v = (unsigned long long)(s & 0xffffu) | ((unsigned long long)(s >> 16) << 32);
        unsigned long long total;
        const unsigned long long before = tt_block_exclusive_scan<unsigned long long, TT_SCAN_BLOCK>(v, &total);
        if (b < c.nblk) c.boff[b] = carry + before;
        carry += total;
        __syncthreads();  // the scan's wave totals are rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        const int lo = (int)(carry & 0xffffffffull), hi = (int)(carry >> 32);
        c.tot[0] = lo;
        c.tot[1] = hi;
        out_totals[0] = lo;
        out_totals[1] = hi;
    }
}

static inline void tt_compact2_scan_blocks(const TtCompact2& c, int* out_totals, hipStream_t s) {
    hipLaunchKernelGGL(k_compact2_blocks, dim3(1), dim3(TT_SCAN_BLOCK), 0, s, c, out_totals);
}

// both levels for two flag arrays
template <typename Flag>
static void tt_compact2_scan_flags(const Flag* lo_flag, int n_lo, const Flag* hi_flag, int n_hi, const TtCompact2& c,
                                   int* out_totals, hipStream_t s) {
    hipLaunchKernelGGL(k_compact2_flags<Flag>, dim3((unsigned)c.nblk), dim3(TT_COMPACT_BLOCK), 0, s, lo_flag, n_lo,
                       hi_flag, n_hi, c);
    tt_compact2_scan_blocks(c, out_totals, s);
}

// global exclusive offset of item i (0 <= i < n) in the low / in the high stream
__device__ __forceinline__ int tt_compact2_lo(const TtCompact2& c, int i) {
    return (int)(unsigned)(c.boff[(unsigned)i / TT_COMPACT_BLOCK] & 0xffffffffull) + (c.local[i] & 0xffff);
}
__device__ __forceinline__ int tt_compact2_hi(const TtCompact2& c, int i) {
    return (int)(unsigned)(c.boff[(unsigned)i / TT_COMPACT_BLOCK] >> 32) + (c.local[i] >> 16);
}
