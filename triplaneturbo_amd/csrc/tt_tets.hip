// tt_tets.hip -- marching tetrahedra (DMTet) with a backward pass: the drop-in for the reference's
// `MarchingTetrahedraHelper._forward`
//   threestudio/models/isosurface.py:126-327 (helper; :231-301 the extraction, :141-169 the case table)
// The tet grid is static, so what the reference recomputes per call with torch.unique(dim=0) -- the unique sorted edges
// and each tet's row in them -- is built once per grid (ops.TetGrid: edges, tet_edge, vertex -> incident-edge CSR).
// The output contract (occupied = level > 0, vertex = crossing edge in `edges` order, one-triangle tets before
// two-triangle tets, the interpolation formula) is written in include/tt_abi.h.
//
// Five launches, no atomics (identical launches give bit-identical results), wave64, 256 threads = 256 consecutive
// items per block, int32 indices:
//   k_mt_classify      item i is edge i and tet i: the edge's crossing flag, the tet's case; first level of two
//                      compactions of tt_compact.h (edges: crossing | unused; tets: one-triangle | two-triangle)
//   k_compact2_blocks  (tt_compact.h, once per compaction) block offsets and grand totals (the host reads those 12
//                      bytes: the only round trip)
//   k_mt_emit          item i: the vertex of crossing edge i, the one or two faces of tet i (vertex ids via tet_edge)
//   k_mt_bwd           one thread per grid vertex gathers over its CSR row: dense grad_level and grad_pos, no scatter
#include "tt_compact.h"
#include "tt_mask.h"

#pragma clang fp contract(off)  // the interpolation exactly as written in tt_abi.h (the numpy oracle replays it)

#define MT_BLOCK TT_COMPACT_BLOCK

// isosurface.py:141-169: per case (sum of occupied corner k << k) the triangles as local edge numbers (base edges
// 01 02 03 12 13 23), and how many
static __constant__ const signed char k_mt_tri_edges[16][6] = {
    {-1, -1, -1, -1, -1, -1}, {1, 0, 2, -1, -1, -1}, {4, 0, 3, -1, -1, -1}, {1, 4, 2, 1, 3, 4},
    {3, 1, 5, -1, -1, -1},    {2, 3, 0, 2, 5, 3},    {1, 4, 0, 1, 5, 4},    {4, 2, 5, -1, -1, -1},
    {4, 5, 2, -1, -1, -1},    {4, 1, 0, 4, 5, 1},    {3, 2, 0, 3, 5, 2},    {1, 3, 5, -1, -1, -1},
    {4, 1, 2, 4, 3, 1},       {3, 0, 4, -1, -1, -1}, {2, 0, 1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}};
static __constant__ const unsigned char k_mt_tri_count[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};

struct MtWs {
    unsigned char *cross, *cas;
    TtCompact2 ce;  // items: edges; low counter: crossing edges = vertices, high: unused
    TtCompact2 ct;  // items: tets; low counter: one-triangle tets, high: two-triangle tets (TETS, two face rows each)
};

struct MtLayout {
    MtWs w;
    long long bytes;  // size of the workspace
};

// the workspace sections (tt_mt_workspace_bytes); base may be null for the size alone
static MtLayout mt_layout(void* base, int n_edges, int n_tets) {
    TtCarver c{(char*)base};
    MtLayout l;
    l.w.cross = c.take<unsigned char>(n_edges);  // [Ne] 1: exactly one end of the edge is occupied
    l.w.cas = c.take<unsigned char>(n_tets);     // [Nt] case index of the tet
    l.w.ce = tt_compact2_carve(c, n_edges, nullptr);
    l.w.ct = tt_compact2_carve(c, n_tets, nullptr);
    int* tot = c.take<int>(64);  // [4] grand totals: vertices, unused | one-triangle tets, two-triangle tets
    l.w.ce.tot = tot;
    l.w.ct.tot = tot ? tot + 2 : nullptr;
    l.bytes = c.bytes();
    return l;
}

static inline unsigned mt_grid(const MtWs& w) { return (unsigned)max(w.ce.nblk, w.ct.nblk); }

// occupied = level > 0 (isosurface.py:236; the opposite of marching cubes' level < iso); a NaN level is not.  A 0/1
// integer the compiler cannot see through (tt_mask.h): the flags of an edge's or a tet's corners are combined by integer
// arithmetic, never as lane masks on the scalar ALU.
__device__ __forceinline__ unsigned mt_occ(const float* __restrict__ level, int v) {
    return tt_opaque_t(level[v] > 0.f ? 1u : 0u);
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_classify(const float* __restrict__ level,
                                                          const int2* __restrict__ edges,
                                                          const int4* __restrict__ tets, MtWs w) {
    const int i = blockIdx.x * MT_BLOCK + threadIdx.x;
    unsigned cross = 0, one = 0, two = 0;
    if (i < w.ce.n) {
        const int2 e = edges[i];
        cross = mt_occ(level, e.x) ^ mt_occ(level, e.y);
        w.cross[i] = (unsigned char)cross;
    }
    if (i < w.ct.n) {
        const int4 t = tets[i];
        const unsigned cas = mt_occ(level, t.x) | (mt_occ(level, t.y) << 1) | (mt_occ(level, t.z) << 2) |
                             (mt_occ(level, t.w) << 3);
        w.cas[i] = (unsigned char)cas;
        const unsigned nt = k_mt_tri_count[cas];
        one = nt == 1;
        two = nt == 2;
    }
    // every counter adds at most 1 per item (the two-triangle counter counts tets, not face rows), so a block's total is
    // at most TT_COMPACT_BLOCK = 256 and fits the 16 bits tt_compact.h packs it in (first_level<1> asserts it).  The
    // grid covers the longer of the two item lists; a block past the end of the other one has no slot in its bsum.
    if (blockIdx.x < w.ce.nblk) tt_compact2_first_level<1>(w.ce, cross, 0u);
    __syncthreads();  // both calls share the scan's wave totals (tt_scan.h)
    if (blockIdx.x < w.ct.nblk) tt_compact2_first_level<1>(w.ct, one, two);
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_emit(const float* __restrict__ pos, const float* __restrict__ level,
                                                      const int2* __restrict__ edges,
                                                      const int* __restrict__ tet_edge, MtWs w,
                                                      float* __restrict__ v_pos, int* __restrict__ t_pos_idx) {
    const int i = blockIdx.x * MT_BLOCK + threadIdx.x;
    // bounds of every write: the counts the scan produced
    const int n_vert = w.ce.tot[0], n_one = w.ct.tot[0], n_two = w.ct.tot[1];
    if (i < w.ce.n && w.cross[i]) {
        const int vid = tt_compact2_lo(w.ce, i);
        if (vid < n_vert) {
            const int2 e = edges[i];
            const float sa = level[e.x], sb = level[e.y];
            const float den = sa - sb;  // like-signed magnitudes: never cancels
            const float wa = -sb / den, wb = sa / den;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v_pos[(size_t)vid * 3 + c] = pos[(size_t)e.x * 3 + c] * wa + pos[(size_t)e.y * 3 + c] * wb;
        }
    }
    if (i >= w.ct.n) return;
    const int cas = w.cas[i];
    const int nt = k_mt_tri_count[cas];
    if (nt == 0) return;
    // one-triangle tets first, in tet order; then two rows per two-triangle tet, in tet order (isosurface.py:285-299)
    const int rank = nt == 1 ? tt_compact2_lo(w.ct, i) : tt_compact2_hi(w.ct, i);
    if (rank >= (nt == 1 ? n_one : n_two)) return;
    const size_t row = nt == 1 ? (size_t)rank : (size_t)n_one + 2 * (size_t)rank;
    for (int j = 0; j < 3 * nt; ++j) {
        const int e = tet_edge[(size_t)i * 6 + k_mt_tri_edges[cas][j]];
        t_pos_idx[row * 3 + j] = tt_compact2_lo(w.ce, e);
    }
}

__global__ __launch_bounds__(MT_BLOCK) void k_mt_bwd(const float* __restrict__ pos, const float* __restrict__ level,
                                                     const int2* __restrict__ edges, const int* __restrict__ vert_ptr,
                                                     const int* __restrict__ vert_col, int n_vertices, MtWs w,
                                                     const float* __restrict__ grad_v, float* __restrict__ grad_level,
                                                     float* __restrict__ grad_pos) {
    const int v = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (v >= n_vertices) return;
    const int n_vert = w.ce.tot[0];
    float gl = 0.f, gp[3] = {0.f, 0.f, 0.f};
    // fixed order: the incident edges ascending (the CSR row)
    for (int k = vert_ptr[v]; k < vert_ptr[v + 1]; ++k) {
        const int e = vert_col[k];
        if (!w.cross[e]) continue;
        const int vid = tt_compact2_lo(w.ce, e);
        if (vid >= n_vert) continue;
        const int2 ab = edges[e];
        const float sa = level[ab.x], sb = level[ab.y];
        const float den = sa - sb;
        float gd = 0.f, g[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g[c] = grad_v[(size_t)vid * 3 + c];
            gd = gd + g[c] * (pos[(size_t)ab.y * 3 + c] - pos[(size_t)ab.x * 3 + c]);
        }
        // dv/ds_a = (p_b - p_a) (-s_b) / den^2, dv/ds_b = (p_b - p_a) s_a / den^2; dv/dp_a = w_a, dv/dp_b = w_b
        const bool is_a = v == ab.x;
        gl = gl + gd * ((is_a ? -sb : sa) / (den * den));
        const float wgt = (is_a ? -sb : sa) / den;
#pragma unroll
        for (int c = 0; c < 3; ++c) gp[c] = gp[c] + g[c] * wgt;
    }
    grad_level[v] = gl;
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_pos[(size_t)v * 3 + c] = gp[c];
}

static bool mt_counts_ok(int n_edges, int n_tets) {
    return n_edges >= 1 && n_tets >= 1 && n_edges <= TT_MESH_MAX_ITEMS && n_tets <= TT_MESH_MAX_ITEMS;
}

extern "C" int64_t tt_mt_workspace_bytes(int32_t n_edges, int32_t n_tets) {
    if (!mt_counts_ok(n_edges, n_tets)) return TT_ERR_BAD_ARG;
    return mt_layout(nullptr, n_edges, n_tets).bytes;
}

extern "C" int tt_mt_count(const float* level, const int32_t* edges, const int32_t* tets, int32_t n_edges,
                           int32_t n_tets, void* workspace, int32_t* out_totals, void* stream) {
    if (!mt_counts_ok(n_edges, n_tets) || !level || !edges || !tets || !workspace || !out_totals)
        return TT_ERR_BAD_ARG;
    const MtWs w = mt_layout(workspace, n_edges, n_tets).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mt_classify, dim3(mt_grid(w)), dim3(MT_BLOCK), 0, s, level, (const int2*)edges,
                       (const int4*)tets, w);
    // out_totals = (vertices, one-triangle tets, two-triangle tets): the edge compaction's unused high total lands in
    // slot 1 first and the tet compaction, next on the stream, overwrites it
    tt_compact2_scan_blocks(w.ce, (int*)out_totals, s);
    tt_compact2_scan_blocks(w.ct, (int*)out_totals + 1, s);
    return tt_check_launch();
}

extern "C" int tt_mt_emit(const float* pos, const float* level, const int32_t* edges, const int32_t* tet_edge,
                          int32_t n_edges, int32_t n_tets, void* workspace, float* v_pos, int32_t* t_pos_idx,
                          void* stream) {
    if (!mt_counts_ok(n_edges, n_tets) || !pos || !level || !edges || !tet_edge || !workspace || !v_pos || !t_pos_idx)
        return TT_ERR_BAD_ARG;
    const MtWs w = mt_layout(workspace, n_edges, n_tets).w;
    hipLaunchKernelGGL(k_mt_emit, dim3(mt_grid(w)), dim3(MT_BLOCK), 0, (hipStream_t)stream, pos, level,
                       (const int2*)edges, (const int*)tet_edge, w, v_pos, (int*)t_pos_idx);
    return tt_check_launch();
}

extern "C" int tt_mt_bwd(const float* pos, const float* level, const int32_t* edges, const int32_t* vert_ptr,
                         const int32_t* vert_col, int32_t n_vertices, int32_t n_edges, int32_t n_tets, void* workspace,
                         const float* grad_v, float* grad_level, float* grad_pos, void* stream) {
    if (!mt_counts_ok(n_edges, n_tets) || n_vertices < 1 || n_vertices > TT_MESH_MAX_ITEMS) return TT_ERR_BAD_ARG;
    if (!pos || !level || !edges || !vert_ptr || !vert_col || !workspace || !grad_v || !grad_level || !grad_pos)
        return TT_ERR_BAD_ARG;
    const MtWs w = mt_layout(workspace, n_edges, n_tets).w;
    hipLaunchKernelGGL(k_mt_bwd, dim3(tt_grid(n_vertices)), dim3(MT_BLOCK), 0, (hipStream_t)stream, pos, level,
                       (const int2*)edges, (const int*)vert_ptr, (const int*)vert_col, n_vertices, w, grad_v,
                       grad_level, grad_pos);
    return tt_check_launch();
}
