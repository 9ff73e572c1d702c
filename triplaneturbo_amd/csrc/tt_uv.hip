// tt_uv.hip -- UV atlas (axis-projection charts) and texture fill for the textured mesh export: the GPU stand-ins for
// xatlas (threestudio/models/mesh.py:207-249) and cv2.inpaint (multiprompt_mesh_exporter.py:96-107).  The contract
// (labels, smoothing, charts, projection, packing, emit order, overlap guard, fill) is written in include/tt_abi.h,
// "UV atlas and texture fill"; the packing itself (O(charts) numbers) is tt_uv_pack in tt_host.cpp.
//
// Labels (tt_uv_labels):
//   k_lab_init     per face: the six axis scores of the double cross product, argmax label, admissible-label bits
//   k_adj_fill     per face pair: the (at most 3) edge neighbours of every face, slot order by integer atomics
//   k_lab_round    one Jacobi round of constrained majority voting (ping-pong buffers; the vote is order-independent)
// Charts (tt_uv_charts):
//   k_pair_filter  same-label pairs of non-singleton faces; the others become (-1, -1), which tt_mesh_components skips
//   tt_mesh_components (tt_mesh.hip) -> comp = smallest face of the chart
//   k_root_flag + int scan (tt_exclusive_scan of tt_scan.h) -> dense chart ids in order of the smallest face;
//   k_chart_assign
//   k_box_reduce   chart bounding box of the projected vertices, ordered-int atomicMin / atomicMax
//   k_box_out      decoded to floats
// Emit (tt_uv_emit_count, tt_uv_emit):
//   vertex -> corner CSR (k_vc_count, int scan, k_vc_fill; the row order does not matter below)
//   k_rep          the representative corner of each (vertex, chart) pair = its smallest corner id; int scan of the
//                  representatives -> UV vertex ids in order of the representative corner
//   k_uv_emit      v_tex of each representative, t_tex_idx of every corner
// Overlap guard (tt_uv_overlap): k_ov_count counts, per texel, the UV triangles whose interior holds its centre (the
// rasterizer's tri_setup / tri_cover on clip (2u - 1, 2v - 1, 0, 1)); k_ov_flag flags the faces on a texel counted
// twice; k_ov_texels counts the covered texels.
// Fill (tt_tex_fill): jump flooding of nearest covered texel ids (key = squared distance << 32 | id, min), then a
// copy.  Every result is integer-atomic or a fixed-order gather: bit-identical from launch to launch.
#include "tt_host.h"
#include "tt_raster_cover.h"  // tri_setup / tri_cover / pix_ndc (and fp contract off for this file)
#include "tt_scan.h"

#define UV_BLOCK TT_ITEM_BLOCK

// ---------------------------------------------------------------------------------------------------------------
// workspace
struct UvWs {
    unsigned char* adm;
    int *lab2, *deg, *nbr, *pairs;
    void* mesh;
    int *comp, *flag, *rootid, *box, *vdeg, *vptr, *vfill, *vcorner, *rep, *isrep, *uvid, *bsum, *tot;
    float4* clip;
    int* cnt;
};

// the workspace sections (tt_uv_workspace_bytes); base may be null for the size alone
static UvWs uv_ws(void* base, long long V, long long T, long long N, long long* bytes = nullptr) {
    TtCarver c{(char*)base};
    UvWs w;
    const long long n = 3 * T > V + 1 ? 3 * T : V + 1;  // longest scanned array
    // tt_mesh_components needs tt_mesh_components_bytes(T); the section keeps the larger size it has always had, a
    // whole tt_mesh_workspace_bytes(0, T), so that tt_uv_workspace_bytes does not change
    const long long mesh_used = tt_mesh_components_bytes(T), mesh_kept = tt_mesh_workspace_bytes(0, (int32_t)T);
    w.adm = c.take<unsigned char>(T);      // [T] admissible-label bits (0: zero-area face)
    w.lab2 = c.take<int>(T);               // [T] Jacobi ping-pong buffer
    w.deg = c.take<int>(T);                // [T] edge neighbours found per face
    w.nbr = c.take<int>(3 * T);            // [3T] the neighbours (slots >= deg unused)
    w.pairs = c.take<int>(3 * T);          // [3T] filtered face pairs (2P <= 3T ints)
    w.mesh = c.take<char>(mesh_kept > mesh_used ? mesh_kept : mesh_used);  // tt_mesh_components' workspace
    w.comp = c.take<int>(T);               // [T] smallest face of the chart
    w.flag = c.take<int>(T);               // [T] chart roots
    w.rootid = c.take<int>(T);             // [T] exclusive scan of the roots: dense chart id at the root
    w.box = c.take<int>(4 * T);            // [4T] ordered-int chart boxes: umin, vmin, umax, vmax
    w.vdeg = c.take<int>(V + 1);           // [V+1] corners per vertex
    w.vptr = c.take<int>(V + 1);           // [V+1] CSR offsets
    w.vfill = c.take<int>(V);              // [V] fill cursors
    w.vcorner = c.take<int>(3 * T);        // [3T] corner ids by vertex
    w.rep = c.take<int>(3 * T);            // [3T] representative corner of each corner's (vertex, chart) pair
    w.isrep = c.take<int>(3 * T);          // [3T] 1 for representatives
    w.uvid = c.take<int>(3 * T);           // [3T] exclusive scan of isrep
    w.bsum = c.take<int>(tt_xscan_blocks(n) + 1);  // scratch of the scans
    w.tot = c.take<int>(64);               // 0 charts, 1 UV vertices, 2 flagged faces, 3 covered texels, 8.. scan totals
    w.clip = c.take<float4>(3 * T);        // [3T] clip positions of the UV vertices (Vt <= 3T)
    w.cnt = c.take<int>(N * N);            // [N*N] UV triangles per texel centre
    if (bytes) *bytes = c.bytes();
    return w;
}


__global__ void k_copy_total(const int* __restrict__ src, int* __restrict__ dst, int* __restrict__ out) {
    if (threadIdx.x == 0) {
        dst[0] = src[0];
        out[0] = src[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// labels
// the three vertex ids of face f clamped into [0, V) (a read in bounds); 0 if one was outside
__device__ __forceinline__ int uv_face_vertices(const int* __restrict__ tri, int f, int V, int* idx) {
    unsigned bad = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = tri[(size_t)f * 3 + k];
        bad += (unsigned)i >= (unsigned)V ? 1u : 0u;
        idx[k] = (int)min((unsigned)i, (unsigned)(V - 1));
    }
    return bad == 0u ? 1 : 0;
}

// the face normal n = (p1 - p0) x (p2 - p0) in double (fixed operation order) and |n|^2
__device__ __forceinline__ double face_normal(const float* __restrict__ v, const int* idx, double n[3]) {
    const double p0x = v[(size_t)idx[0] * 3], p0y = v[(size_t)idx[0] * 3 + 1], p0z = v[(size_t)idx[0] * 3 + 2];
    const double e1x = (double)v[(size_t)idx[1] * 3] - p0x, e1y = (double)v[(size_t)idx[1] * 3 + 1] - p0y,
                 e1z = (double)v[(size_t)idx[1] * 3 + 2] - p0z;
    const double e2x = (double)v[(size_t)idx[2] * 3] - p0x, e2y = (double)v[(size_t)idx[2] * 3 + 1] - p0y,
                 e2z = (double)v[(size_t)idx[2] * 3 + 2] - p0z;
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
    return (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
}

__global__ __launch_bounds__(UV_BLOCK) void k_lab_init(const float* __restrict__ v, const int* __restrict__ tri, int V,
                                                       int T, double tau2, int* __restrict__ labels, UvWs w) {
    const int f = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (f >= T) return;
    int idx[3];
    const int ok = uv_face_vertices(tri, f, V, idx);
    double n[3];
    const double nn = face_normal(v, idx, n);
    int best = 0;
    double bs = n[0];
    unsigned adm = 0;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
        const double a = (l & 1) ? -n[l >> 1] : n[l >> 1];
        best = a > bs ? l : best;  // strict: the first maximum (smallest label) wins a tie
        bs = fmax(a, bs);
        adm |= (copysign(a * a, a) >= tau2 * nn ? 1u : 0u) << l;  // a >= tau |n|
    }
    // zero-area (or invalid) faces have no admissible label and start at +x
    const double live = ok ? nn : 0.0;
    w.adm[f] = (unsigned char)(live > 0.0 ? adm : 0u);
    labels[f] = live > 0.0 ? best : 0;
    w.deg[f] = 0;
}

__global__ __launch_bounds__(UV_BLOCK) void k_adj_fill(const int* __restrict__ pairs, int P, int T, UvWs w) {
    const int e = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (e >= P) return;
    const int a = pairs[2 * e], b = pairs[2 * e + 1];
    if ((unsigned)a >= (unsigned)T || (unsigned)b >= (unsigned)T || a == b) return;
    const int sa = atomicAdd(w.deg + a, 1);
    if (sa < 3) w.nbr[(size_t)a * 3 + sa] = b;
    const int sb = atomicAdd(w.deg + b, 1);
    if (sb < 3) w.nbr[(size_t)b * 3 + sb] = a;
}

__global__ __launch_bounds__(UV_BLOCK) void k_lab_round(const int* __restrict__ lin, int T, UvWs w,
                                                        int* __restrict__ lout) {
    const int f = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (f >= T) return;
    const int cur = lin[f];
    const int d = min(w.deg[f], 3);
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    int nmin = 6;
#pragma unroll
    for (int l = 0; l < 6; ++l) cnt[l] += cur == l ? 1 : 0;
    for (int q = 0; q < d; ++q) {
        const int ln = lin[w.nbr[(size_t)f * 3 + q]];
        nmin = min(nmin, ln);
#pragma unroll
        for (int l = 0; l < 6; ++l) cnt[l] += ln == l ? 1 : 0;
    }
    const unsigned adm = w.adm[f];
    int best = cur, bc = 0;
#pragma unroll
    for (int l = 0; l < 6; ++l) bc += cur == l ? cnt[l] : 0;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
        // admissible and strictly more votes: ONE compare of (admissible ? votes : -1) against the best so far
        const int c = ((adm >> l) & 1u) ? cnt[l] : -1;
        best = c > bc ? l : best;
        bc = max(c, bc);
    }
    // a zero-area face takes its smallest neighbour label (+x without neighbours)
    const int zero_rule = nmin < 6 ? nmin : 0;
    lout[f] = adm == 0u ? zero_rule : best;
}

// ---------------------------------------------------------------------------------------------------------------
// charts
__global__ __launch_bounds__(UV_BLOCK) void k_pair_filter(const int* __restrict__ pairs, int P, int T,
                                                          const int* __restrict__ labels,
                                                          const unsigned char* __restrict__ singleton, UvWs w) {
    const int e = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (e >= P) return;
    const int a = pairs[2 * e], b = pairs[2 * e + 1];
    const int ca = (int)min((unsigned)a, (unsigned)(T - 1)), cb = (int)min((unsigned)b, (unsigned)(T - 1));
    // kept iff both in range, same label and neither a singleton: a sum of non-negative terms compared with 0 once
    const unsigned bad = ((unsigned)a >= (unsigned)T ? 1u : 0u) + ((unsigned)b >= (unsigned)T ? 1u : 0u) +
                         (unsigned)(labels[ca] ^ labels[cb]) +
                         (singleton ? (unsigned)singleton[ca] + (unsigned)singleton[cb] : 0u);
    w.pairs[2 * e] = bad == 0u ? a : -1;
    w.pairs[2 * e + 1] = bad == 0u ? b : -1;
}

__global__ __launch_bounds__(UV_BLOCK) void k_root_flag(int T, UvWs w) {
    const int f = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (f < T) w.flag[f] = w.comp[f] == f ? 1 : 0;
}

// order-preserving int image of a float (signed compare = float compare, -0 < +0)
__device__ __forceinline__ int ord_of(float x) {
    const int b = __float_as_int(x);
    return b >= 0 ? b : (b ^ 0x7fffffff);
}
__device__ __forceinline__ float float_of(int o) { return __int_as_float(o >= 0 ? o : (o ^ 0x7fffffff)); }

__global__ __launch_bounds__(UV_BLOCK) void k_chart_assign(int T, UvWs w, int* __restrict__ chart) {
    const int f = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (f >= T) return;
    chart[f] = w.rootid[w.comp[f]];
    w.box[(size_t)f * 4 + 0] = 0x7fffffff;
    w.box[(size_t)f * 4 + 1] = 0x7fffffff;
    w.box[(size_t)f * 4 + 2] = (int)0x80000000;
    w.box[(size_t)f * 4 + 3] = (int)0x80000000;
}

// in-plane coordinates of label l (u x v = +axis): +x (y,z) -x (z,y) +y (z,x) -y (x,z) +z (x,y) -z (y,x)
__device__ __forceinline__ void uv_axes(int l, int& cu, int& cv) {
    const int a = l >> 1, p = (a + 1) % 3, q = (a + 2) % 3;
    cu = (l & 1) ? q : p;
    cv = (l & 1) ? p : q;
}

__global__ __launch_bounds__(UV_BLOCK) void k_box_reduce(const float* __restrict__ v, const int* __restrict__ tri,
                                                         int V, int T, const int* __restrict__ labels,
                                                         const int* __restrict__ chart, UvWs w) {
    const int f = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (f >= T) return;
    int idx[3];
    uv_face_vertices(tri, f, V, idx);
    int cu, cv;
    uv_axes(labels[f], cu, cv);
    int* b = w.box + (size_t)chart[f] * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ou = ord_of(v[(size_t)idx[k] * 3 + cu]), ov = ord_of(v[(size_t)idx[k] * 3 + cv]);
        atomicMin(b + 0, ou);
        atomicMin(b + 1, ov);
        atomicMax(b + 2, ou);
        atomicMax(b + 3, ov);
    }
}

__global__ __launch_bounds__(UV_BLOCK) void k_box_out(int T, UvWs w, float* __restrict__ chart_box) {
    const int c = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (c >= min(T, w.tot[0])) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) chart_box[(size_t)c * 4 + k] = float_of(w.box[(size_t)c * 4 + k]);
}

// ---------------------------------------------------------------------------------------------------------------
// emit
__global__ __launch_bounds__(UV_BLOCK) void k_vc_count(const int* __restrict__ tri, int V, int T, UvWs w) {
    const int q = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (q >= 3 * T) return;
    const int vi = tri[q];
    if ((unsigned)vi < (unsigned)V) atomicAdd(w.vdeg + vi, 1);
}

__global__ __launch_bounds__(UV_BLOCK) void k_vc_fill(const int* __restrict__ tri, int V, int T, UvWs w) {
    const int q = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (q >= 3 * T) return;
    const int vi = tri[q];
    if ((unsigned)vi >= (unsigned)V) return;
    const int slot = atomicAdd(w.vfill + vi, 1);
    w.vcorner[w.vptr[vi] + slot] = q;
}

__global__ __launch_bounds__(UV_BLOCK) void k_rep(const int* __restrict__ tri, const int* __restrict__ chart, int V,
                                                  int T, UvWs w) {
    const int q = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (q >= 3 * T) return;
    const int vi = tri[q];
    int rep = q;
    if ((unsigned)vi < (unsigned)V) {  // (else the corner stays its own pair)
        const int c = chart[q / 3];
        const int b = w.vptr[vi], e = w.vptr[vi + 1];
        for (int k = b; k < e; ++k) {
            const int o = w.vcorner[k];
            rep = chart[o / 3] == c ? min(rep, o) : rep;
        }
    }
    w.rep[q] = rep;
    w.isrep[q] = rep == q ? 1 : 0;
}

__global__ __launch_bounds__(UV_BLOCK) void k_uv_emit(const float* __restrict__ v, const int* __restrict__ tri, int V,
                                                      int T, const int* __restrict__ labels,
                                                      const int* __restrict__ chart,
                                                      const float* __restrict__ chart_box,
                                                      const int* __restrict__ offsets, int C, float scale, int N,
                                                      int pad, UvWs w, float* __restrict__ v_tex,
                                                      int* __restrict__ t_tex_idx) {
    const int q = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (q >= 3 * T) return;
    const int id = w.uvid[w.rep[q]];
    t_tex_idx[q] = id;
    if (w.isrep[q] == 0) return;
    if (id >= w.tot[1]) return;  // every write bounded by the count the caller allocated
    const int f = q / 3;
    const int c = (int)min((unsigned)chart[f], (unsigned)(C - 1));
    const int vi = (int)min((unsigned)tri[q], (unsigned)(V - 1));
    int cu, cv;
    uv_axes(labels[f], cu, cv);
    const float pu = v[(size_t)vi * 3 + cu], pv = v[(size_t)vi * 3 + cv];
    const float U = ((float)(offsets[2 * c] + pad) + 0.5f) + (pu - chart_box[(size_t)c * 4 + 0]) * scale;
    const float W = ((float)(offsets[2 * c + 1] + pad) + 0.5f) + (pv - chart_box[(size_t)c * 4 + 1]) * scale;
    v_tex[(size_t)id * 2] = U / (float)N;
    v_tex[(size_t)id * 2 + 1] = W / (float)N;
}

// ---------------------------------------------------------------------------------------------------------------
// overlap guard
__global__ __launch_bounds__(UV_BLOCK) void k_ov_clip(const float* __restrict__ v_tex, int Vt, UvWs w) {
    const int i = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (i < Vt)
        w.clip[i] = make_float4(v_tex[(size_t)i * 2] * 2.f - 1.f, v_tex[(size_t)i * 2 + 1] * 2.f - 1.f, 0.f, 1.f);
}

// the texel box of a set-up triangle (k_rast_setup's box with one texel of margin), clamped to the texture
__device__ __forceinline__ int4 ov_box(const TriSetup& s, int N) {
    float x0 = 3.4e38f, x1 = -3.4e38f, y0 = 3.4e38f, y1 = -3.4e38f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float px = ((s.X[k] + 1.f) * (float)N - 1.f) * 0.5f, py = ((s.Y[k] + 1.f) * (float)N - 1.f) * 0.5f;
        x0 = fminf(x0, px);
        x1 = fmaxf(x1, px);
        y0 = fminf(y0, py);
        y1 = fmaxf(y1, py);
    }
    x0 = fminf(fmaxf(floorf(x0) - 1.f, 0.f), (float)N);
    x1 = fminf(fmaxf(ceilf(x1) + 1.f, -1.f), (float)(N - 1));
    y0 = fminf(fmaxf(floorf(y0) - 1.f, 0.f), (float)N);
    y1 = fminf(fmaxf(ceilf(y1) + 1.f, -1.f), (float)(N - 1));
    return make_int4((int)x0, (int)y0, (int)x1, (int)y1);
}

__global__ __launch_bounds__(UV_BLOCK) void k_ov_count(const int* __restrict__ t_tex, int Vt, int T, int N, UvWs w) {
    const int f = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (f >= T) return;
    TriSetup s;
    if (!tri_setup((const float*)w.clip, t_tex, 0, f, Vt, s)) return;
    const int4 bb = ov_box(s, N);
    for (int py = bb.y; py <= bb.w; ++py) {
        for (int px = bb.x; px <= bb.z; ++px) {
            float u, v, zw, S;
            if (tri_cover(s, pix_ndc(px, N), pix_ndc_lo(px, N), pix_ndc(py, N), pix_ndc_lo(py, N), u, v, zw, S))
                atomicAdd(w.cnt + (size_t)py * N + px, 1);
        }
    }
}

__global__ __launch_bounds__(UV_BLOCK) void k_ov_flag(const int* __restrict__ t_tex, int Vt, int T, int N, UvWs w,
                                                      unsigned char* __restrict__ flags) {
    const int f = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (f >= T) return;
    TriSetup s;
    int over = 0;
    if (tri_setup((const float*)w.clip, t_tex, 0, f, Vt, s)) {
        const int4 bb = ov_box(s, N);
        for (int py = bb.y; py <= bb.w; ++py) {
            for (int px = bb.x; px <= bb.z; ++px) {
                float u, v, zw, S;
                if (tri_cover(s, pix_ndc(px, N), pix_ndc_lo(px, N), pix_ndc(py, N), pix_ndc_lo(py, N), u, v, zw, S))
                    over |= w.cnt[(size_t)py * N + px] > 1 ? 1 : 0;
            }
        }
    }
    flags[f] = (unsigned char)over;
    if (over) atomicAdd(w.tot + 2, 1);
}

__global__ __launch_bounds__(UV_BLOCK) void k_ov_texels(int n, UvWs w) {
    const int i = blockIdx.x * UV_BLOCK + threadIdx.x;
    const int c = i < n ? w.cnt[min(i, n - 1)] : 0;
    const int k = tt_wave_sum(c > 0 ? 1 : 0);  // a shuffle sum per wave, one integer atomic per wave
    if ((threadIdx.x & 63) == 0 && k > 0) atomicAdd(w.tot + 3, k);
}

__global__ void k_ov_totals(UvWs w, int* __restrict__ out_totals) {
    if (threadIdx.x == 0) {
        out_totals[0] = w.tot[2];
        out_totals[1] = w.tot[3];
    }
}

__global__ void k_ov_zero_tot(UvWs w) {
    if (threadIdx.x == 0) {
        w.tot[2] = 0;
        w.tot[3] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// texture fill: jump flooding of (squared distance << 32 | source texel) keys, the minimum wins
// (no select: an empty source (-1) ORs in all ones, the largest key, whose low half reads back as -1 again)
__device__ __forceinline__ unsigned long long jfa_key(int x, int y, int src, int W) {
    const int cs = max(src, 0);
    const long long dx = x - cs % W, dy = y - cs / W;
    const unsigned long long k = ((unsigned long long)(dx * dx + dy * dy) << 32) | (unsigned)cs;
    return k | (unsigned long long)(long long)(src >> 31);
}

__global__ __launch_bounds__(UV_BLOCK) void k_jfa_init(const unsigned char* __restrict__ mask, int n,
                                                       int* __restrict__ seed) {
    const int i = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (i < n) seed[i] = mask[i] ? i : -1;
}

__global__ __launch_bounds__(UV_BLOCK) void k_jfa_step(const int* __restrict__ sin, int H, int W, int step,
                                                       int* __restrict__ sout) {
    const int i = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (i >= H * W) return;
    const int x = i % W, y = i / W;
    unsigned long long best = jfa_key(x, y, sin[i], W);
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            // clamped to the image: a clamped neighbour is a real texel, merely looked at twice
            const int qx = min(max(x + dx * step, 0), W - 1), qy = min(max(y + dy * step, 0), H - 1);
            best = min(best, jfa_key(x, y, sin[qy * W + qx], W));
        }
    }
    sout[i] = (int)(unsigned)(best & 0xffffffffu);  // -1 when no source was seen
}

__global__ __launch_bounds__(UV_BLOCK) void k_fill_out(const float* __restrict__ img, const int* __restrict__ seed,
                                                       int n, int C, float* __restrict__ out) {
    const long long j = (long long)blockIdx.x * UV_BLOCK + threadIdx.x;
    if (j >= (long long)n * C) return;
    const int i = (int)(j / C), c = (int)(j % C);
    const int src = seed[i];
    // a covered texel is its own source (distance 0): copied bit for bit
    const float val = img[(size_t)max(src, 0) * C + c];
    out[j] = src >= 0 ? val : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
static bool uv_sizes_ok(int32_t V, int32_t T, int32_t N) {
    return V >= 0 && T >= 0 && V <= TT_MESH_MAX_ITEMS && T <= TT_UV_MAX_FACES && N >= 1 && N <= TT_UV_MAX_TEX;
}

static bool uv_pairs_ok(const int32_t* face_pairs, int32_t P, int32_t T) {
    return P >= 0 && 2 * (int64_t)P <= 3 * (int64_t)T && (P == 0 || face_pairs);
}

extern "C" int64_t tt_uv_workspace_bytes(int32_t V, int32_t T, int32_t N) {
    if (!uv_sizes_ok(V, T, N)) return TT_ERR_BAD_ARG;
    long long bytes;
    uv_ws(nullptr, V, T, N, &bytes);
    return bytes;
}

extern "C" int tt_uv_labels(const float* v_pos, const int32_t* t_pos_idx, const int32_t* face_pairs, int32_t V,
                            int32_t T, int32_t P, int32_t rounds, float tau, int32_t N, void* workspace,
                            int32_t* labels, void* stream) {
    if (!uv_sizes_ok(V, T, N) || !uv_pairs_ok(face_pairs, P, T) || !workspace) return TT_ERR_BAD_ARG;
    if (rounds < 0 || rounds > TT_UV_MAX_SMOOTH_ROUNDS || !(tau > 0.f && tau <= TT_UV_MAX_TAU)) return TT_ERR_BAD_ARG;
    if (T > 0 && (V < 1 || !v_pos || !t_pos_idx || !labels)) return TT_ERR_BAD_ARG;
    if (T == 0) return 0;
    const UvWs w = uv_ws(workspace, V, T, N);
    hipStream_t s = (hipStream_t)stream;
    const double tau2 = (double)tau * (double)tau;
    hipLaunchKernelGGL(k_lab_init, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, v_pos, (const int*)t_pos_idx, (int)V,
                       (int)T, tau2, (int*)labels, w);
    if (P > 0)
        hipLaunchKernelGGL(k_adj_fill, dim3(tt_grid(P)), dim3(UV_BLOCK), 0, s, (const int*)face_pairs, (int)P, (int)T,
                           w);
    for (int r = 0; r < rounds; ++r) {  // Jacobi: labels -> lab2 -> labels -> ...
        const int* in = (r & 1) ? (const int*)w.lab2 : (const int*)labels;
        int* out = (r & 1) ? (int*)labels : w.lab2;
        hipLaunchKernelGGL(k_lab_round, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, in, (int)T, w, out);
    }
    if (rounds & 1) hipMemcpyAsync(labels, w.lab2, 4 * (size_t)T, hipMemcpyDeviceToDevice, s);
    return tt_check_launch();
}

extern "C" int tt_uv_charts(const float* v_pos, const int32_t* t_pos_idx, const int32_t* face_pairs,
                            const int32_t* labels, const uint8_t* singleton, int32_t V, int32_t T, int32_t P,
                            int32_t N, void* workspace, int32_t* chart, float* chart_box, int32_t* out_totals,
                            void* stream) {
    if (!uv_sizes_ok(V, T, N) || !uv_pairs_ok(face_pairs, P, T) || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    if (T > 0 && (V < 1 || !v_pos || !t_pos_idx || !labels || !chart || !chart_box)) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (T == 0) {
        hipMemsetAsync(out_totals, 0, 4, s);
        return tt_check_launch();
    }
    const UvWs w = uv_ws(workspace, V, T, N);
    if (P > 0)
        hipLaunchKernelGGL(k_pair_filter, dim3(tt_grid(P)), dim3(UV_BLOCK), 0, s, (const int*)face_pairs, (int)P,
                           (int)T, (const int*)labels, (const unsigned char*)singleton, w);
    const int st = tt_mesh_components(w.pairs, P, T, w.mesh, w.comp, stream);
    if (st != 0) return st;
    hipLaunchKernelGGL(k_root_flag, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, (int)T, w);
    tt_exclusive_scan<int>(w.flag, T, w.rootid, w.bsum, w.tot + 8, s);
    hipLaunchKernelGGL(k_copy_total, dim3(1), dim3(64), 0, s, (const int*)(w.tot + 8), w.tot, (int*)out_totals);
    hipLaunchKernelGGL(k_chart_assign, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, (int)T, w, (int*)chart);
    hipLaunchKernelGGL(k_box_reduce, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, v_pos, (const int*)t_pos_idx, (int)V,
                       (int)T, (const int*)labels, (const int*)chart, w);
    hipLaunchKernelGGL(k_box_out, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, (int)T, w, chart_box);
    return tt_check_launch();
}

extern "C" int tt_uv_emit_count(const int32_t* t_pos_idx, const int32_t* chart, int32_t V, int32_t T, int32_t N,
                                void* workspace, int32_t* out_totals, void* stream) {
    if (!uv_sizes_ok(V, T, N) || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    if (T > 0 && (V < 1 || !t_pos_idx || !chart)) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (T == 0) {
        hipMemsetAsync(out_totals, 0, 4, s);
        return tt_check_launch();
    }
    const UvWs w = uv_ws(workspace, V, T, N);
    hipMemsetAsync(w.vdeg, 0, 4 * ((size_t)V + 1), s);
    hipMemsetAsync(w.vfill, 0, 4 * (size_t)V, s);
    hipLaunchKernelGGL(k_vc_count, dim3(tt_grid(3ll * T)), dim3(UV_BLOCK), 0, s, (const int*)t_pos_idx, (int)V,
                       (int)T, w);
    tt_exclusive_scan<int>(w.vdeg, V + 1, w.vptr, w.bsum, w.tot + 9, s);
    hipLaunchKernelGGL(k_vc_fill, dim3(tt_grid(3ll * T)), dim3(UV_BLOCK), 0, s, (const int*)t_pos_idx, (int)V,
                       (int)T, w);
    hipLaunchKernelGGL(k_rep, dim3(tt_grid(3ll * T)), dim3(UV_BLOCK), 0, s, (const int*)t_pos_idx,
                       (const int*)chart, (int)V, (int)T, w);
    tt_exclusive_scan<int>(w.isrep, 3 * T, w.uvid, w.bsum, w.tot + 10, s);
    hipLaunchKernelGGL(k_copy_total, dim3(1), dim3(64), 0, s, (const int*)(w.tot + 10), w.tot + 1, (int*)out_totals);
    return tt_check_launch();
}

extern "C" int tt_uv_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* labels, const int32_t* chart,
                          const float* chart_box, const int32_t* offsets, int32_t C, float scale, int32_t V,
                          int32_t T, int32_t N, int32_t padding, void* workspace, float* v_tex, int32_t* t_tex_idx,
                          void* stream) {
    if (!uv_sizes_ok(V, T, N) || !workspace || C < 0 || C > T || padding < 0 || padding > TT_UV_MAX_PADDING)
        return TT_ERR_BAD_ARG;
    if (!(scale >= 0.f && scale <= 3.0e38f)) return TT_ERR_BAD_ARG;
    if (T == 0) return 0;
    if (C < 1 || V < 1 || !v_pos || !t_pos_idx || !labels || !chart || !chart_box || !offsets || !v_tex || !t_tex_idx)
        return TT_ERR_BAD_ARG;
    const UvWs w = uv_ws(workspace, V, T, N);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_uv_emit, dim3(tt_grid(3ll * T)), dim3(UV_BLOCK), 0, s, v_pos, (const int*)t_pos_idx, (int)V,
                       (int)T, (const int*)labels, (const int*)chart, chart_box, (const int*)offsets, (int)C, scale,
                       (int)N, (int)padding, w, v_tex, (int*)t_tex_idx);
    return tt_check_launch();
}

// t_tex_idx alone, from the workspace tt_uv_emit_count left: what the conformal flattening (tt_uv_lscm.hip) starts from
__global__ __launch_bounds__(UV_BLOCK) void k_uv_index(int T, UvWs w, int* __restrict__ t_tex_idx) {
    const int q = blockIdx.x * UV_BLOCK + threadIdx.x;
    if (q < 3 * T) t_tex_idx[q] = w.uvid[w.rep[q]];
}

extern "C" int tt_uv_lscm_index(int32_t V, int32_t T, int32_t N, void* workspace, int32_t* t_tex_idx, void* stream) {
    if (!uv_sizes_ok(V, T, N) || !workspace || (T > 0 && !t_tex_idx)) return TT_ERR_BAD_ARG;
    if (T == 0) return 0;
    const UvWs w = uv_ws(workspace, V, T, N);
    hipLaunchKernelGGL(k_uv_index, dim3(tt_grid(3ll * T)), dim3(UV_BLOCK), 0, (hipStream_t)stream, (int)T, w,
                       (int*)t_tex_idx);
    return tt_check_launch();
}

extern "C" int tt_uv_overlap(const float* v_tex, const int32_t* t_tex_idx, int32_t Vt, int32_t V, int32_t T,
                             int32_t N, void* workspace, uint8_t* flags, int32_t* out_totals, void* stream) {
    if (!uv_sizes_ok(V, T, N) || Vt < 0 || (int64_t)Vt > 3 * (int64_t)T || !workspace || !out_totals)
        return TT_ERR_BAD_ARG;
    if (T > 0 && (!t_tex_idx || !flags)) return TT_ERR_BAD_ARG;
    if (Vt > 0 && !v_tex) return TT_ERR_BAD_ARG;
    const UvWs w = uv_ws(workspace, V, T, N);
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)N * N;
    hipMemsetAsync(w.cnt, 0, 4 * (size_t)n, s);
    hipLaunchKernelGGL(k_ov_zero_tot, dim3(1), dim3(64), 0, s, w);
    if (T > 0) {
        if (Vt > 0) hipLaunchKernelGGL(k_ov_clip, dim3(tt_grid(Vt)), dim3(UV_BLOCK), 0, s, v_tex, (int)Vt, w);
        hipLaunchKernelGGL(k_ov_count, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, (const int*)t_tex_idx, (int)Vt,
                           (int)T, (int)N, w);
        hipLaunchKernelGGL(k_ov_flag, dim3(tt_grid(T)), dim3(UV_BLOCK), 0, s, (const int*)t_tex_idx, (int)Vt,
                           (int)T, (int)N, w, (unsigned char*)flags);
    }
    hipLaunchKernelGGL(k_ov_texels, dim3(tt_grid(n)), dim3(UV_BLOCK), 0, s, (int)n, w);
    hipLaunchKernelGGL(k_ov_totals, dim3(1), dim3(64), 0, s, w, (int*)out_totals);
    return tt_check_launch();
}

// the two ping-pong seed buffers of the jump flooding, [H*W] each; base may be null for the size alone
struct TexFillWs {
    int *a, *b;
    long long bytes;
};
static TexFillWs tex_fill_ws(void* base, int H, int W) {
    TtCarver c{(char*)base};
    TexFillWs w;
    w.a = c.take<int>((long long)H * W);
    w.b = c.take<int>((long long)H * W);
    w.bytes = c.bytes();
    return w;
}

extern "C" int64_t tt_tex_fill_workspace_bytes(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || H > TT_UV_MAX_TEX || W > TT_UV_MAX_TEX) return TT_ERR_BAD_ARG;
    return tex_fill_ws(nullptr, H, W).bytes;
}

extern "C" int tt_tex_fill(const float* img, const uint8_t* mask, int32_t H, int32_t W, int32_t C, void* workspace,
                           float* out, void* stream) {
    if (H < 1 || W < 1 || H > TT_UV_MAX_TEX || W > TT_UV_MAX_TEX || C < 1 || C > TT_UV_MAX_CHANNELS)
        return TT_ERR_BAD_ARG;
    if (!img || !mask || !workspace || !out) return TT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W;
    const TexFillWs w = tex_fill_ws(workspace, H, W);
    int *a = w.a, *b = w.b;
    hipLaunchKernelGGL(k_jfa_init, dim3(tt_grid(n)), dim3(UV_BLOCK), 0, s, (const unsigned char*)mask, n, a);
    // steps: the largest power of two below max(H, W) down to 1, then the JFA+2 refinement steps 2 and 1
    int step = 1;
    while (2 * step < (H > W ? H : W)) step *= 2;
    int steps[40], ns = 0;
    for (int k = step; k >= 1; k /= 2) steps[ns++] = k;
    steps[ns++] = 2;
    steps[ns++] = 1;
    for (int k = 0; k < ns; ++k) {
        hipLaunchKernelGGL(k_jfa_step, dim3(tt_grid(n)), dim3(UV_BLOCK), 0, s, (const int*)a, (int)H, (int)W,
                           steps[k], b);
        int* t = a;
        a = b;
        b = t;
    }
    hipLaunchKernelGGL(k_fill_out, dim3(tt_grid((long long)n * C)), dim3(UV_BLOCK), 0, s, img, (const int*)a, n,
                       (int)C, out);
    return tt_check_launch();
}
