// tt_isosurface.hip -- marching-cubes isosurface extraction with a backward pass: the drop-in for the reference's
// `diso.DiffMC` (a CUDA-only extension) behind DiffMarchingCubeHelper
//   triplaneturbo_executable/utils/mesh_exporter.py:29-75 (helper), :78-141 (isosurface(), 160^3)
//   threestudio/models/isosurface.py:18-65 (the training-time mesh renderer's helper, 128^3)
// The output contract (inside = level < iso, shared vertices owned by grid points, canonical order, orientation) is
// written in include/tt_abi.h; the case tables are generated (tools/gen_mc_tables.py -> tt_mc_tables.h).
//
// Four launches, no atomics (identical launches give bit-identical results), wave64, 256 threads = 256 consecutive
// grid points per block (k fastest, so every level load is coalesced):
//   k_mc_classify     per point: 3-bit crossing mask of its +x/+y/+z edges; per cell origin: case index and triangle
//                     count; first level of the compaction of tt_compact.h (vertices low, triangles high)
//   k_compact2_blocks (tt_compact.h) block offsets and grand totals (the host reads those 8 bytes: the only round trip)
//   k_mc_emit         per point: its vertices (interpolated, optionally deformed) and its cell's triangles, vertex ids
//                     via table edge -> (owner point, axis) -> the owner's vertex offset + rank of the axis
//   k_mc_bwd          gather per point over its 6 incident edges: dense grad_level and grad_deformation, no scatter
#include "tt_compact.h"

#pragma clang fp contract(off)  // the interpolation exactly as written in tt_abi.h (the numpy oracle replays it)

#define TT_MC_TABLE static __constant__ const
#include "tt_mc_tables.h"

#define MC_BLOCK TT_COMPACT_BLOCK
static_assert(TT_MC_MAX_TRIS >= 3, "a point owns up to 3 vertices: the larger per-item count bounds both counters");

// base-corner offset (di | dj << 1 | dk << 2) of each of the 12 cube edges (tools/gen_mc_tables.py)
static __constant__ const unsigned char k_edge_base[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};

struct McWs {
    unsigned char *mask, *cas;
    TtCompact2 c;  // items: grid points; low counter: vertices, high: triangles
};

struct McLayout {
    McWs w;
    long long bytes;  // size of the workspace
};

// the workspace sections (tt_mc_workspace_bytes); base may be null for the size alone
static McLayout mc_layout(void* base, int res) {
    TtCarver c{(char*)base};
    McLayout l;
    const long long n = (long long)res * res * res;
    l.w.mask = c.take<unsigned char>(n);  // [n] bit a: the edge p -> p + e_a crosses
    l.w.cas = c.take<unsigned char>(n);   // [n] case index of the cell with origin p (0: no cell origin)
    l.w.c = tt_compact2_carve(c, n, nullptr);
    l.w.c.tot = c.take<int>(64);  // [2] grand totals: vertices, triangles (behind the compaction's sections, as ever)
    l.bytes = c.bytes();
    return l;
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_classify(const float* __restrict__ level, int R, float iso, McWs w) {
    const int n = R * R * R;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    unsigned n_vert = 0, n_tri = 0;
    if (p < n) {
        const int k = p % R, j = (p / R) % R, i = p / (R * R);
        // neighbour strides, 0 on the far boundary (the point is then its own neighbour: no crossing, no cell)
        const int sx = i < R - 1 ? R * R : 0, sy = j < R - 1 ? R : 0, sz = k < R - 1 ? 1 : 0;
        int cas = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int idx = p + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? sz : 0);
            cas |= (level[idx] < iso ? 1 : 0) << c;
        }
        const int mask = ((cas ^ (cas >> 1)) & 1) | (((cas ^ (cas >> 2)) & 1) << 1) | (((cas ^ (cas >> 4)) & 1) << 2);
        const int origin = max(max(i, j), k) < R - 1 ? cas : 0;
        w.mask[p] = (unsigned char)mask;
        w.cas[p] = (unsigned char)origin;
        n_vert = (unsigned)__popc(mask);
        n_tri = (unsigned)tt_mc_tri_count[origin];
    }
    tt_compact2_first_level<TT_MC_MAX_TRIS>(w.c, n_vert, n_tri);
}

// vertex id of the edge (owner point q, axis a): requires bit a of mask[q]
__device__ __forceinline__ int mc_vertex_id(const McWs& w, int q, int a) {
    const int m = w.mask[q];
    return tt_compact2_lo(w.c, q) + __popc(m & ((1 << a) - 1));
}

template <bool DEF>
__global__ __launch_bounds__(MC_BLOCK) void k_mc_emit(const float* __restrict__ level, const float* __restrict__ deform,
                                                      int R, float iso, McWs w, float* __restrict__ v_pos,
                                                      int* __restrict__ t_pos_idx) {
    const int n = R * R * R;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int n_vert = w.c.tot[0], n_tri = w.c.tot[1];  // bound of every write: the counts the scan produced
    const int m = w.mask[p];
    if (m) {
        const int coord[3] = {p / (R * R), (p / R) % R, p % R};
        const int stride[3] = {R * R, R, 1};
        const float s0 = level[p];
        float d0[3] = {0.f, 0.f, 0.f};
        if (DEF) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d0[c] = deform[(size_t)p * 3 + c];
        }
        const float inv_den = (float)(R - 1);
        int vid = mc_vertex_id(w, p, 0);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((m >> a) & 1)) continue;
            const int q = p + stride[a];
            const float s1 = level[q];
            const float t = (iso - s0) / (s1 - s0);
            if (vid < n_vert) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float d1 = DEF ? deform[(size_t)q * 3 + c] : 0.f;
                    const float A = (float)coord[c] + d0[c];
                    const float B = (float)(coord[c] + (c == a ? 1 : 0)) + d1;
                    v_pos[(size_t)vid * 3 + c] = (A + t * (B - A)) / inv_den;
                }
            }
            ++vid;
        }
    }
    const int cas = w.cas[p];
    const int nt = tt_mc_tri_count[cas];
    if (nt == 0) return;
    const int tb = tt_compact2_hi(w.c, p);
    for (int t = 0; t < TT_MC_MAX_TRIS; ++t) {
        if (t >= nt) break;
        int ids[3];
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            const int e = tt_mc_tri_edges[cas][3 * t + jj];
            const int bc = k_edge_base[e];
            const int q = p + (bc & 1) * R * R + ((bc >> 1) & 1) * R + ((bc >> 2) & 1);
            ids[jj] = mc_vertex_id(w, q, e >> 2);
        }
        if (tb + t < n_tri) {
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) t_pos_idx[(size_t)(tb + t) * 3 + jj] = ids[jj];
        }
    }
}

// d loss / d (level, deformation) of one endpoint of a crossing edge p0 -> p1 (END = 0: this point is p0, 1: p1)
template <bool DEF, int END>
__device__ __forceinline__ void mc_edge_grad(const float* __restrict__ level, const float* __restrict__ deform,
                                             const float* __restrict__ grad_v, int R, float iso, int p0, int p1, int a,
                                             int vid, const int* coord0, float& gl, float* gd) {
    const float s0 = level[p0], s1 = level[p1];
    const float den = s1 - s0;
    const float t = (iso - s0) / den;
    const float inv = 1.f / (float)(R - 1);
    float gt = 0.f;
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g[c] = grad_v[(size_t)vid * 3 + c];
        const float d0 = DEF ? deform[(size_t)p0 * 3 + c] : 0.f;
        const float d1 = DEF ? deform[(size_t)p1 * 3 + c] : 0.f;
        const float A = (float)coord0[c] + d0;
        const float B = (float)(coord0[c] + (c == a ? 1 : 0)) + d1;
        gt = gt + g[c] * ((B - A) * inv);
    }
    // dt/ds0 = (iso - s1) / den^2, dt/ds1 = -(iso - s0) / den^2
    const float dts = END == 0 ? (iso - s1) / (den * den) : -(iso - s0) / (den * den);
    gl = gl + gt * dts;
    if (DEF) {
        const float wgt = (END == 0 ? 1.f - t : t) * inv;
#pragma unroll
        for (int c = 0; c < 3; ++c) gd[c] = gd[c] + g[c] * wgt;
    }
}

template <bool DEF>
__global__ __launch_bounds__(MC_BLOCK) void k_mc_bwd(const float* __restrict__ level, const float* __restrict__ deform,
                                                     int R, float iso, McWs w, const float* __restrict__ grad_v,
                                                     float* __restrict__ grad_level, float* __restrict__ grad_deform) {
    const int n = R * R * R;
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int n_vert = w.c.tot[0];
    const int coord[3] = {p / (R * R), (p / R) % R, p % R};
    const int stride[3] = {R * R, R, 1};
    float gl = 0.f, gd[3] = {0.f, 0.f, 0.f};
    const int m = w.mask[p];
    // fixed order: per axis x, y, z the edge this point owns (it is p0), then the edge that ends here (it is p1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if ((m >> a) & 1) {
            const int vid = mc_vertex_id(w, p, a);
            if (vid < n_vert) mc_edge_grad<DEF, 0>(level, deform, grad_v, R, iso, p, p + stride[a], a, vid, coord, gl, gd);
        }
        const int q = coord[a] > 0 ? p - stride[a] : p;
        const int mq = coord[a] > 0 ? (int)w.mask[q] : 0;
        if ((mq >> a) & 1) {
            const int vid = mc_vertex_id(w, q, a);
            int cq[3] = {coord[0], coord[1], coord[2]};
            cq[a] -= 1;
            if (vid < n_vert) mc_edge_grad<DEF, 1>(level, deform, grad_v, R, iso, q, p, a, vid, cq, gl, gd);
        }
    }
    grad_level[p] = gl;
    if (DEF) {
#pragma unroll
        for (int c = 0; c < 3; ++c) grad_deform[(size_t)p * 3 + c] = gd[c];
    }
}

static bool mc_res_ok(int res) { return res >= 2 && res <= TT_MC_MAX_RES; }

extern "C" int64_t tt_mc_workspace_bytes(int32_t res) {
    if (!mc_res_ok(res)) return TT_ERR_BAD_ARG;
    return mc_layout(nullptr, res).bytes;
}

extern "C" int tt_mc_count(const float* level, int32_t res, float isovalue, void* workspace, int32_t* out_totals,
                           void* stream) {
    if (!mc_res_ok(res) || !level || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    const McWs w = mc_layout(workspace, res).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_classify, dim3((unsigned)w.c.nblk), dim3(MC_BLOCK), 0, s, level, res, isovalue, w);
    tt_compact2_scan_blocks(w.c, out_totals, s);
    return tt_check_launch();
}

extern "C" int tt_mc_emit(const float* level, const float* deformation, int32_t res, float isovalue, void* workspace,
                          float* v_pos, int32_t* t_pos_idx, void* stream) {
    if (!mc_res_ok(res) || !level || !workspace || !v_pos || !t_pos_idx) return TT_ERR_BAD_ARG;
    const McWs w = mc_layout(workspace, res).w;
    hipStream_t s = (hipStream_t)stream;
    if (deformation)
        hipLaunchKernelGGL(k_mc_emit<true>, dim3((unsigned)w.c.nblk), dim3(MC_BLOCK), 0, s, level, deformation, res,
                           isovalue, w, v_pos, (int*)t_pos_idx);
    else
        hipLaunchKernelGGL(k_mc_emit<false>, dim3((unsigned)w.c.nblk), dim3(MC_BLOCK), 0, s, level, nullptr, res,
                           isovalue, w, v_pos, (int*)t_pos_idx);
    return tt_check_launch();
}

extern "C" int tt_mc_bwd(const float* level, const float* deformation, int32_t res, float isovalue, void* workspace,
                         const float* grad_v, float* grad_level, float* grad_deformation, void* stream) {
    if (!mc_res_ok(res) || !level || !workspace || !grad_v || !grad_level) return TT_ERR_BAD_ARG;
    if ((deformation == nullptr) != (grad_deformation == nullptr)) return TT_ERR_BAD_ARG;
    const McWs w = mc_layout(workspace, res).w;
    hipStream_t s = (hipStream_t)stream;
    if (deformation)
        hipLaunchKernelGGL(k_mc_bwd<true>, dim3((unsigned)w.c.nblk), dim3(MC_BLOCK), 0, s, level, deformation, res,
                           isovalue, w, grad_v, grad_level, grad_deformation);
    else
        hipLaunchKernelGGL(k_mc_bwd<false>, dim3((unsigned)w.c.nblk), dim3(MC_BLOCK), 0, s, level, nullptr, res,
                           isovalue, w, grad_v, grad_level, nullptr);
    return tt_check_launch();
}
