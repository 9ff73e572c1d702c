// tt_mesh.hip -- the threestudio Mesh regularisers and outlier removal on the GPU
//   threestudio/models/mesh.py:255-308  normal_consistency(), laplacian() (the system's lambda_normal_consistency /
//                                       lambda_laplacian_smoothness terms, multiprompt_dual_renderer_multistep_generator.py
//                                       :716-757)
//   threestudio/models/mesh.py:31-95    remove_outlier() (trimesh split + filter on the host in the reference)
// The contract (adjacency rule, labels, output order, threshold, loss formulas, determinism) is written in
// include/tt_abi.h, "mesh regularisers and outlier removal".  The topology (sorted unique edges, face pairs, the
// vertex -> neighbour CSR) is built once per mesh by ops.mesh_topology with torch sorts.
//
// Components: lock-free union-find over faces (ECL-CC / Jayanti-Tarjan style): parent[x] <= x always, a root is
// hooked under the smaller root with atomicCAS, finds halve the path.  The surviving root of a component is its
// smallest face (nothing smaller can be hooked on), so the flattened labels do not depend on scheduling.
//   k_uf_init     parent[f] = f, count[f] = 0
//   k_uf_hook     per face pair: union
//   k_uf_flatten  label[f] = root(f) (path halving), count[label] += 1 (integer atomics)
//   k_uf_max      max count over the roots (integer atomicMax)
// Compaction (count -> 8-byte read-back -> emit, as tt_mc_count / tt_mc_emit):
//   k_cc_keep     threshold on the device, fkeep[f], vmark[v] = 0
//   k_cc_mark     vmark[v] = 1 for the vertices of kept faces
//   k_compact2_flags / k_compact2_blocks   (tt_compact.h) offsets of the marked vertices and kept faces, (V', T')
//   k_cc_emit     kept vertices and remapped kept faces, in their original order
// Losses: per-item kernels write fixed-order block partials, one block sums them in fixed order; the gradients are
// CSR gathers (no atomics).  Every value is bit-identical from launch to launch.
#include "tt_compact.h"

#define MESH_BLOCK TT_ITEM_BLOCK
#define MESH_FINAL_BLOCK 256

struct MeshWs {
    int *parent, *count, *misc;
    unsigned char *fkeep, *vmark;
    TtCompact2 c;  // items: max(V, T); low counter: marked vertices, high: kept faces; totals in misc[2..3]
    float *part, *w;
};

struct MeshLayout {
    MeshWs w;
    long long bytes;  // size of the workspace
};

// the sections tt_mesh_components touches: they sit first and depend on T only, so a workspace of
// tt_mesh_components_bytes(T) is enough for it (tt_uv.hip nests one)
static MeshWs mesh_components_ws(TtCarver& c, long long T) {
    MeshWs w{};
    w.parent = c.take<int>(T);  // [T] union-find forest
    w.count = c.take<int>(T);   // [T] faces per component, at its label
    w.misc = c.take<int>(64);   // [0] max faces of a component, [2..3] (V', T')
    return w;
}

long long tt_mesh_components_bytes(long long T) {
    TtCarver c{nullptr};
    mesh_components_ws(c, T);
    return c.bytes();
}

// the workspace sections (tt_mesh_workspace_bytes); base may be null for the size alone
static MeshLayout mesh_layout(void* base, long long V, long long T) {
    TtCarver c{(char*)base};
    MeshLayout l;
    const long long nl = V > 3 * T ? V : 3 * T;  // items of a loss reduction: V vertices or E <= 3T edges
    l.w = mesh_components_ws(c, T);
    l.w.fkeep = c.take<unsigned char>(T);  // [T] face kept
    l.w.vmark = c.take<unsigned char>(V);  // [V] vertex referenced by a kept face
    l.w.c = tt_compact2_carve(c, V > T ? V : T, base ? l.w.misc + 2 : nullptr);
    l.w.part = c.take<float>(tt_grid(nl));  // [blocks of nl items] loss partials
    l.w.w = c.take<float>(3 * V);           // [3V] Laplacian backward: d loss / d r
    l.bytes = c.bytes();
    return l;
}

// ---------------------------------------------------------------------------------------------------------------
// union-find
// ---------------------------------------------------------------------------------------------------------------
// Device-scope relaxed accesses: the forest is read and rewritten by waves on every XCD within one launch.
__device__ __forceinline__ int uf_load(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uf_store(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving.  Every value ever stored obeys parent[x] <= x, and a halving store replaces a parent
// by one of its ancestors (never touching a root), so the walk strictly decreases and the forest keeps its sets.
__device__ int uf_find(int* parent, int x) {
    int p = uf_load(parent + x);
    while (p != x) {
        const int gp = uf_load(parent + p);
        if (gp == p) return p;
        uf_store(parent + x, gp);
        x = gp;
        p = uf_load(parent + x);
    }
    return x;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_uf_init(int T, MeshWs w) {
    const int f = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f < T) {
        w.parent[f] = f;
        w.count[f] = 0;
    }
    if (f == 0) w.misc[0] = 0;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_uf_hook(const int* __restrict__ pairs, int P, int T, MeshWs w) {
    const int e = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (e >= P) return;
    const int a = pairs[2 * e], b = pairs[2 * e + 1];
    if ((unsigned)a >= (unsigned)T || (unsigned)b >= (unsigned)T) return;
    int ra = uf_find(w.parent, a), rb = uf_find(w.parent, b);
    while (ra != rb) {
        const int lo = min(ra, rb), hi = max(ra, rb);
        const int old = atomicCAS(w.parent + hi, hi, lo);  // hook the larger root under the smaller one
        if (old == hi) break;
        ra = uf_find(w.parent, old);  // hi stopped being a root: retry from where it went
        rb = uf_find(w.parent, lo);
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_uf_flatten(int T, MeshWs w, int* __restrict__ labels) {
    const int f = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f >= T) return;
    // the forest's sets and roots are final after k_uf_hook; halving here only shortens the walks of other faces
    const int x = uf_find(w.parent, f);
    labels[f] = x;
    atomicAdd(w.count + x, 1);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_uf_max(const int* __restrict__ labels, int T, MeshWs w) {
    const int f = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f < T && labels[f] == f) atomicMax(w.misc, w.count[f]);
}

// ---------------------------------------------------------------------------------------------------------------
// compaction
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MESH_BLOCK) void k_cc_keep(const int* __restrict__ tri, const int* __restrict__ labels,
                                                        int V, int T, int frac_mode, double frac, long long thr_int,
                                                        MeshWs w) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < V) w.vmark[i] = 0;
    if (i >= T) return;
    // Python's int(max_faces * t): a double product truncated toward zero; both forms clamped to +-2^62 (any value
    // beyond T acts the same), so that neither the conversion nor thr - 1 below can overflow
    const double lim = 4611686018427387904.0;
    const long long thr = frac_mode ? (long long)fmin(fmax((double)w.misc[0] * frac, -lim), lim)
                                    : max(min(thr_int, (long long)lim), -(long long)lim);
    // sign-bit arithmetic instead of `a && b ? 1 : 0` (the lane-mask shape of DESIGN.md section 6,
    // tools/mask_hazard_lint.py): each term is negative iff its condition holds
    long long in_range = (long long)(unsigned)labels[i] - T;
#pragma unroll
    for (int k = 0; k < 3; ++k) in_range &= (long long)(unsigned)tri[(size_t)i * 3 + k] - V;
    const int lab = min((unsigned)labels[i], (unsigned)(T - 1));  // read in bounds; in_range discards a bad one
    const long long big_enough = thr - 1 - (long long)w.count[lab];  // < 0 iff count >= thr
    w.fkeep[i] = (unsigned char)(((unsigned long long)(in_range & big_enough)) >> 63);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cc_mark(const int* __restrict__ tri, int T, MeshWs w) {
    const int f = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (f >= T || !w.fkeep[f]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) w.vmark[tri[(size_t)f * 3 + k]] = 1;  // in range: k_cc_keep checked it
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cc_emit(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                        int V, int T, MeshWs w, float* __restrict__ v_out,
                                                        int* __restrict__ t_out) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const int nv = w.misc[2], nt = w.misc[3];  // bound of every write: the totals the scan produced
    if (i < V && w.vmark[i]) {
        const int o = tt_compact2_lo(w.c, i);
        if (o < nv) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v_out[(size_t)o * 3 + c] = v_pos[(size_t)i * 3 + c];
        }
    }
    if (i < T && w.fkeep[i]) {
        const int o = tt_compact2_hi(w.c, i);
        if (o < nt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) t_out[(size_t)o * 3 + k] = tt_compact2_lo(w.c, tri[(size_t)i * 3 + k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// losses
// ---------------------------------------------------------------------------------------------------------------
// fixed-order block sum (the result is valid in thread 0): a shuffle tree per wave, then the 4 wave sums in order
__device__ __forceinline__ float block_sum(float v) {
    __shared__ float wave_sum[MESH_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = tt_wave_sum(v);
    if (lane == 0) wave_sum[wave] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < MESH_BLOCK / 64; ++q) t += wave_sum[q];
    }
    return t;
}

// one block: out = (sum of the partials in a fixed order) / n_items  (0 / 0 = NaN for no items, like torch's mean)
__global__ __launch_bounds__(MESH_FINAL_BLOCK) void k_loss_final(const float* __restrict__ part, int nblk, int n_items,
                                                                 float* __restrict__ out) {
    float s = 0.f;
    for (int b = threadIdx.x; b < nblk; b += MESH_FINAL_BLOCK) s += part[b];
    const float t = block_sum(s);
    if (threadIdx.x == 0) out[0] = t / (float)n_items;
}

// r_i = sum over the non-self neighbours j of (v_i - v_j), ascending j
__device__ __forceinline__ void lap_residual(const float* __restrict__ v, const int* __restrict__ ptr,
                                             const int* __restrict__ col, int V, int i, float r[3]) {
    const float vi[3] = {v[(size_t)i * 3], v[(size_t)i * 3 + 1], v[(size_t)i * 3 + 2]};
    r[0] = r[1] = r[2] = 0.f;
    const int b = ptr[i], e = ptr[i + 1];
    for (int q = b; q < e; ++q) {
        const int j = col[q];
        if (j == i || (unsigned)j >= (unsigned)V) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] += vi[c] - v[(size_t)j * 3 + c];
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_lap_fwd(const float* __restrict__ v, const int* __restrict__ ptr,
                                                        const int* __restrict__ col, int V, float* __restrict__ part) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    float nrm = 0.f;
    if (i < V) {
        float r[3];
        lap_residual(v, ptr, col, V, i, r);
        nrm = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    }
    const float t = block_sum(nrm);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// w_i = d loss / d r_i = (g / V) r_i / |r_i|, 0 where r_i = 0 (torch's subgradient of the norm)
__global__ __launch_bounds__(MESH_BLOCK) void k_lap_bwd_w(const float* __restrict__ v, const int* __restrict__ ptr,
                                                          const int* __restrict__ col, int V,
                                                          const float* __restrict__ g_loss, float* __restrict__ w) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= V) return;
    float r[3];
    lap_residual(v, ptr, col, V, i, r);
    const float nrm = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const float s = g_loss[0] / (float)V;
    const float f = nrm > 0.f ? s / nrm : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) w[(size_t)i * 3 + c] = r[c] * f;
}

// g_k = sum over the non-self neighbours j of (w_k - w_j) = (L^T w)_k
__global__ __launch_bounds__(MESH_BLOCK) void k_lap_bwd_g(const float* __restrict__ w, const int* __restrict__ ptr,
                                                          const int* __restrict__ col, int V, float* __restrict__ g) {
    const int k = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (k >= V) return;
    float acc[3];
    lap_residual(w, ptr, col, V, k, acc);
#pragma unroll
    for (int c = 0; c < 3; ++c) g[(size_t)k * 3 + c] = acc[c];
}

// torch.cosine_similarity(x, y, dim=-1, eps) semantics: each norm clamped to eps from below
__device__ __forceinline__ float nc_norm(const float x[3], float& true_norm, float eps) {
    true_norm = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    return fmaxf(true_norm, eps);
}

__device__ __forceinline__ void load3(const float* __restrict__ p, int i, float x[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = p[(size_t)i * 3 + c];
}

__global__ __launch_bounds__(MESH_BLOCK) void k_nc_fwd(const float* __restrict__ n, const int* __restrict__ edges,
                                                       int V, int E, float eps, float* __restrict__ part) {
    const int e = blockIdx.x * MESH_BLOCK + threadIdx.x;
    float term = 0.f;
    if (e < E) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if ((unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V) {
            float x[3], y[3], tx, ty;
            load3(n, a, x);
            load3(n, b, y);
            const float nx = nc_norm(x, tx, eps), ny = nc_norm(y, ty, eps);
            float c = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) c += (x[q] / nx) * (y[q] / ny);
            term = 1.f - c;
        }
    }
    const float t = block_sum(term);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// per vertex k, over its incident edges (CSR entries (k, j); a self edge appears twice):
//   d cos(x, y) / d x = y/(ny nx) - (cos / nx) x / |x|    (x = n_k, y = n_j; the x/|x| term is 0 for x = 0)
__global__ __launch_bounds__(MESH_BLOCK) void k_nc_bwd(const float* __restrict__ n, const int* __restrict__ ptr,
                                                       const int* __restrict__ col, int V, int E, float eps,
                                                       const float* __restrict__ g_loss, float* __restrict__ g) {
    const int k = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (k >= V) return;
    float x[3], tx;
    load3(n, k, x);
    const float nx = nc_norm(x, tx, eps);
    const float xu[3] = {tx > 0.f ? x[0] / tx : 0.f, tx > 0.f ? x[1] / tx : 0.f, tx > 0.f ? x[2] / tx : 0.f};
    float acc[3] = {0.f, 0.f, 0.f};
    const int b = ptr[k], e = ptr[k + 1];
    for (int q = b; q < e; ++q) {
        const int j = col[q];
        if ((unsigned)j >= (unsigned)V) continue;
        float y[3], ty;
        load3(n, j, y);
        const float ny = nc_norm(y, ty, eps);
        float yh[3], c = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            yh[d] = y[d] / ny;
            c += (x[d] / nx) * yh[d];
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) acc[d] += yh[d] / nx - (c / nx) * xu[d];
    }
    const float s = E > 0 ? -g_loss[0] / (float)E : 0.f;  // no edges: no term, zero gradient
#pragma unroll
    for (int d = 0; d < 3; ++d) g[(size_t)k * 3 + d] = acc[d] * s;
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t tt_mesh_workspace_bytes(int32_t V, int32_t T) {
    if (V < 0 || T < 0 || V > TT_MESH_MAX_ITEMS || T > TT_MESH_MAX_ITEMS) return TT_ERR_BAD_ARG;
    return mesh_layout(nullptr, V, T).bytes;
}

extern "C" int tt_mesh_components(const int32_t* face_pairs, int32_t P, int32_t T, void* workspace, int32_t* labels,
                                  void* stream) {
    if (P < 0 || T < 0 || T > TT_MESH_MAX_ITEMS || !workspace) return TT_ERR_BAD_ARG;
    if ((P > 0 && !face_pairs) || (T > 0 && !labels)) return TT_ERR_BAD_ARG;
    if (T == 0) return 0;
    TtCarver c{(char*)workspace};
    const MeshWs w = mesh_components_ws(c, T);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_uf_init, dim3(tt_grid(T)), dim3(MESH_BLOCK), 0, s, (int)T, w);
    if (P > 0)
        hipLaunchKernelGGL(k_uf_hook, dim3(tt_grid(P)), dim3(MESH_BLOCK), 0, s, (const int*)face_pairs, (int)P,
                           (int)T, w);
    hipLaunchKernelGGL(k_uf_flatten, dim3(tt_grid(T)), dim3(MESH_BLOCK), 0, s, (int)T, w, (int*)labels);
    hipLaunchKernelGGL(k_uf_max, dim3(tt_grid(T)), dim3(MESH_BLOCK), 0, s, (const int*)labels, (int)T, w);
    return tt_check_launch();
}

extern "C" int tt_mesh_compact_count(const int32_t* t_pos_idx, const int32_t* labels, int32_t V, int32_t T,
                                     int32_t frac_mode, double frac, int64_t threshold, void* workspace,
                                     int32_t* out_totals, void* stream) {
    if (V < 0 || T < 1 || V > TT_MESH_MAX_ITEMS || T > TT_MESH_MAX_ITEMS) return TT_ERR_BAD_ARG;
    if (!t_pos_idx || !labels || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    if (frac_mode != 0 && frac_mode != 1) return TT_ERR_BAD_ARG;
    if (frac_mode == 1 && !(frac >= -1e300 && frac <= 1e300)) return TT_ERR_BAD_ARG;  // NaN / inf
    const MeshWs w = mesh_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cc_keep, dim3((unsigned)w.c.nblk), dim3(MESH_BLOCK), 0, s, (const int*)t_pos_idx,
                       (const int*)labels, (int)V, (int)T, (int)frac_mode, frac, (long long)threshold, w);
    hipLaunchKernelGGL(k_cc_mark, dim3(tt_grid(T)), dim3(MESH_BLOCK), 0, s, (const int*)t_pos_idx, (int)T, w);
    tt_compact2_scan_flags(w.vmark, V, w.fkeep, T, w.c, (int*)out_totals, s);
    return tt_check_launch();
}

extern "C" int tt_mesh_compact_emit(const float* v_pos, const int32_t* t_pos_idx, int32_t V, int32_t T,
                                    void* workspace, float* v_out, int32_t* t_out, void* stream) {
    if (V < 0 || T < 1 || V > TT_MESH_MAX_ITEMS || T > TT_MESH_MAX_ITEMS) return TT_ERR_BAD_ARG;
    if (!t_pos_idx || !workspace || !t_out || (V > 0 && (!v_pos || !v_out))) return TT_ERR_BAD_ARG;
    const MeshWs w = mesh_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cc_emit, dim3((unsigned)w.c.nblk), dim3(MESH_BLOCK), 0, s, v_pos, (const int*)t_pos_idx,
                       (int)V, (int)T, w, v_out, (int*)t_out);
    return tt_check_launch();
}

// nbr_col is read only inside the rows nbr_ptr delimits: NULL is legal for a mesh without edges (all rows empty)
static bool mesh_csr_ok(const int32_t* ptr, int32_t V) {
    return V >= 0 && V <= TT_MESH_MAX_ITEMS && (V == 0 || ptr);
}

extern "C" int tt_mesh_laplacian_fwd(const float* v_pos, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V,
                                     int32_t T, void* workspace, float* loss, void* stream) {
    if (!mesh_csr_ok(nbr_ptr, V) || T < 0 || T > TT_MESH_MAX_ITEMS || !workspace || !loss)
        return TT_ERR_BAD_ARG;
    if (V > 0 && !v_pos) return TT_ERR_BAD_ARG;
    const MeshWs w = mesh_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = tt_grid(V);
    if (nb > 0)
        hipLaunchKernelGGL(k_lap_fwd, dim3(nb), dim3(MESH_BLOCK), 0, s, v_pos, (const int*)nbr_ptr,
                           (const int*)nbr_col, (int)V, w.part);
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(MESH_FINAL_BLOCK), 0, s, (const float*)w.part, (int)nb, (int)V,
                       loss);
    return tt_check_launch();
}

extern "C" int tt_mesh_laplacian_bwd(const float* v_pos, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V,
                                     int32_t T, const float* grad_loss, void* workspace, float* grad_v, void* stream) {
    if (!mesh_csr_ok(nbr_ptr, V) || T < 0 || T > TT_MESH_MAX_ITEMS || !workspace || !grad_loss)
        return TT_ERR_BAD_ARG;
    if (V > 0 && (!v_pos || !grad_v)) return TT_ERR_BAD_ARG;
    if (V == 0) return 0;
    const MeshWs w = mesh_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lap_bwd_w, dim3(tt_grid(V)), dim3(MESH_BLOCK), 0, s, v_pos, (const int*)nbr_ptr,
                       (const int*)nbr_col, (int)V, grad_loss, w.w);
    hipLaunchKernelGGL(k_lap_bwd_g, dim3(tt_grid(V)), dim3(MESH_BLOCK), 0, s, (const float*)w.w,
                       (const int*)nbr_ptr, (const int*)nbr_col, (int)V, grad_v);
    return tt_check_launch();
}

extern "C" int tt_mesh_nc_fwd(const float* v_nrm, const int32_t* edges, int32_t V, int32_t T, int32_t E,
                              void* workspace, float* loss, void* stream) {
    if (V < 0 || T < 0 || E < 0 || V > TT_MESH_MAX_ITEMS || T > TT_MESH_MAX_ITEMS || (int64_t)E > 3 * (int64_t)T)
        return TT_ERR_BAD_ARG;
    if (!workspace || !loss || (E > 0 && (!edges || !v_nrm))) return TT_ERR_BAD_ARG;
    const MeshWs w = mesh_layout(workspace, V, T).w;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = tt_grid(E);
    if (nb > 0)
        hipLaunchKernelGGL(k_nc_fwd, dim3(nb), dim3(MESH_BLOCK), 0, s, v_nrm, (const int*)edges, (int)V, (int)E,
                           TT_MESH_COS_EPS, w.part);
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(MESH_FINAL_BLOCK), 0, s, (const float*)w.part, (int)nb, (int)E,
                       loss);
    return tt_check_launch();
}

extern "C" int tt_mesh_nc_bwd(const float* v_nrm, const int32_t* nbr_ptr, const int32_t* nbr_col, int32_t V,
                              int32_t E, const float* grad_loss, float* grad_nrm, void* stream) {
    if (!mesh_csr_ok(nbr_ptr, V) || E < 0 || !grad_loss) return TT_ERR_BAD_ARG;
    if (V > 0 && (!v_nrm || !grad_nrm)) return TT_ERR_BAD_ARG;
    if (V == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nc_bwd, dim3(tt_grid(V)), dim3(MESH_BLOCK), 0, s, v_nrm, (const int*)nbr_ptr,
                       (const int*)nbr_col, (int)V, (int)E, TT_MESH_COS_EPS, grad_loss, grad_nrm);
    return tt_check_launch();
}
