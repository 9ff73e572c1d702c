// tt_decimate.h -- what the round-based edge operators of the mesh stage share (tt_decimate.hip: quadric collapse;
// tt_remesh.hip: split, midpoint collapse, flip, relax): the CSR tables of one round, the fp64 vector helpers, the
// fixed integer hash of the priorities, the flip test of a collapse and the walk over a closed neighbourhood.  The
// contracts are in include/tt_abi.h, "mesh decimation" and "isotropic remeshing".
#pragma once
#include "tt_compact.h"

#define DEC_BLOCK TT_ITEM_BLOCK
#define DEC_INVALID 0xffffffffu

// the CSR tables of one round: rows of vertices, clamped where they are read
struct DecTopo {
    const int* __restrict__ nbr_ptr;  // [V+1]
    const int* __restrict__ nbr_col;  // [NN] ascending inside a row
    const int* __restrict__ vf_ptr;   // [V+1]
    const int* __restrict__ vf_col;   // [3T] face corners 3f + k, ascending inside a row
    int V, T, NN;
};

struct DecP {
    double x, y, z;
};

__device__ __forceinline__ DecP dec_pos(const float* __restrict__ v_pos, unsigned v) {
    return DecP{(double)v_pos[(size_t)v * 3], (double)v_pos[(size_t)v * 3 + 1], (double)v_pos[(size_t)v * 3 + 2]};
}
__device__ __forceinline__ DecP dec_sub(DecP a, DecP b) { return DecP{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dec_dot(DecP a, DecP b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ DecP dec_cross(DecP a, DecP b) {
    return DecP{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ int dec_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the fixed integer mix of the priorities (tt_abi.h)
__device__ __forceinline__ unsigned dec_hash(unsigned a, unsigned b, unsigned round) {
    unsigned h = (a * 0x9E3779B1u) ^ ((b + 0x7F4A7C15u) * 0x85EBCA77u) ^ ((round + 1u) * 0xC2B2AE3Du);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}

// 1 when no face of star(v) without `other` flips past the bound with v moved to x, else 0
__device__ __forceinline__ unsigned dec_star_ok(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                const DecTopo& t, unsigned v, unsigned other, DecP x) {
    unsigned ok = 1;
    const int rb = dec_clamp(t.vf_ptr[v], 0, 3 * t.T), re = dec_clamp(t.vf_ptr[v + 1], 0, 3 * t.T);
    for (int i = rb; i < re; ++i) {
        const unsigned f = (unsigned)t.vf_col[i] / 3u;
        if (f >= (unsigned)t.T) continue;
        const unsigned i0 = (unsigned)tri[(size_t)f * 3], i1 = (unsigned)tri[(size_t)f * 3 + 1],
                       i2 = (unsigned)tri[(size_t)f * 3 + 2];
        if (max(i0, max(i1, i2)) >= (unsigned)t.V) continue;
        if (i0 == other || i1 == other || i2 == other) continue;  // holds both endpoints: the collapse removes it
        const DecP p0 = dec_pos(v_pos, i0), p1 = dec_pos(v_pos, i1), p2 = dec_pos(v_pos, i2);
        const DecP n_old = dec_cross(dec_sub(p1, p0), dec_sub(p2, p0));
        const DecP r0 = i0 == v ? x : p0, r1 = i1 == v ? x : p1, r2 = i2 == v ? x : p2;
        const DecP n_new = dec_cross(dec_sub(r1, r0), dec_sub(r2, r0));
        const double oo = dec_dot(n_old, n_old), nn = dec_dot(n_new, n_new), on = dec_dot(n_old, n_new);
        // ONE compare: n_new == 0 gives 0 > 0, a NaN compares false
        ok &= (unsigned)(on > 0.2 * (sqrt(oo) * sqrt(nn)));
    }
    return ok;
}

// f(w) for every w of {a, b} + N(a) + N(b) (a vertex may come more than once)
template <class F>
__device__ __forceinline__ void dec_neighbourhood(const DecTopo& t, unsigned a, unsigned b, F f) {
    f(a);
    f(b);
    for (int side = 0; side < 2; ++side) {
        const unsigned v = side ? b : a;
        const int rb = dec_clamp(t.nbr_ptr[v], 0, t.NN), re = dec_clamp(t.nbr_ptr[v + 1], 0, t.NN);
        for (int i = rb; i < re; ++i) {
            const unsigned w = (unsigned)t.nbr_col[i];
            if (w < (unsigned)t.V) f(w);
        }
    }
}

static bool dec_sizes_ok(int32_t V, int32_t T) {
    return V >= 1 && T >= 1 && V <= TT_MESH_MAX_ITEMS && T <= TT_MESH_MAX_ITEMS;
}
// E unique edges of T faces
static bool dec_edges_ok(int32_t T, int32_t E) { return E >= 1 && (long long)E <= 3ll * T; }

static DecTopo dec_topo(const int32_t* nbr_ptr, const int32_t* nbr_col, const int32_t* vf_ptr, const int32_t* vf_col,
                        int32_t V, int32_t T, int32_t E) {
    return DecTopo{(const int*)nbr_ptr, (const int*)nbr_col, (const int*)vf_ptr, (const int*)vf_col, (int)V, (int)T,
                   (int)(2 * E)};
}
