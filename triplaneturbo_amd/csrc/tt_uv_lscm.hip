// tt_uv_lscm.hip -- least-squares conformal (LSCM) flattening of the UV atlas' charts: the opt-in second flattening of
// ops.uv_atlas(method="lscm").  The contract (energy, pins, solve, normalise, orient, accept, emit) is written in
// include/tt_abi.h, "conformal UV charts"; labels, charts, packing, the overlap guard and the fill stay tt_uv.hip's.
//
// Everything works on the UV vertices in CHART ORDER (sorted by chart, then by UV-vertex id: the host's stable sort), so a
// chart is one contiguous range of every solver vector, cut into tiles of TT_UV_LSCM_TILE vertices; the int32 `tables`
// argument carries that order (ls_tab below).  One wave owns one tile, one wave owns one chart:
//   per-chart sums   stage 1: a wave sums its tile (4 vertices per lane in ascending order, then the fixed shuffle tree of
//                    tt_wave_sum) into part[tile]; stage 2: the chart's wave sums its tiles (lane-strided ascending, the same
//                    tree).  A chart of 3 vertices costs one wave, a chart of 10^4 costs 40 tiles and one more wave.  No float
//                    atomics anywhere: bit-identical from launch to launch.
//   operator         A = M^T M of the energy, matrix-free: k_ls_face_apply writes, per face, the three corner terms of
//                    M^T (M x) (its local frame is computed once, k_ls_face); the vertex gather sums a vertex's corner terms
//                    in ascending corner order over the corner CSR.
//   pins / boxes     integer atomics on ordered images (float -> int, non-negative double -> its bit pattern)
// Setup (tt_uv_lscm_setup): chart boxes in 3-D, the two pins, face frames, the Jacobi diagonal, b = -A x_pin, r = b,
// p = D^-1 r.  Iterate (tt_uv_lscm_iterate): n lock-step CG iterations, six launches each, every chart with its own alpha,
// beta and residual; a converged chart is skipped by every kernel.  Finish (tt_uv_lscm_finish): areas -> scale, covariance
// -> rotation, the per-face acceptance test, the final fp32 coordinates and their boxes.  tt_uv_lscm_emit: the texel UVs.
#include "tt_host.h"
#include "tt_scan.h"

#pragma clang fp contract(off)  // the fallback projection repeats tt_uv_emit's fp32 formula bit for bit; doubles as written

#define LS_BLOCK TT_ITEM_BLOCK
#define LS_WAVES (LS_BLOCK / 64)
#define LS_PER_LANE (TT_UV_LSCM_TILE / 64)
#define LS_CONVERGED 1  // bits of LsWs::done
#define LS_NO_PINS 2
#define LS_BAD_AREA 4   // bits of LsWs::fail
#define LS_BAD_FACE 8

// ---------------------------------------------------------------------------------------------------------------
// the host's tables (one int32 array; the layout is part of the contract) and the workspace
struct LsTab {
    const int *fc, *ccol, *vmesh, *vchart, *vperm, *cptr, *vptr, *tptr, *tchart, *tbegin;
};

static LsTab ls_tab(const int32_t* t, long long T, long long Vt, long long C, long long NT) {
    LsTab a;
    a.fc = t;                     // [3T] UV vertex (chart order) of corner 3f + k
    a.ccol = a.fc + 3 * T;        // [3T] corner ids by UV vertex, every row ascending
    a.vmesh = a.ccol + 3 * T;     // [Vt] mesh vertex of a UV vertex
    a.vchart = a.vmesh + Vt;      // [Vt] its chart (ascending)
    a.vperm = a.vchart + Vt;      // [Vt] its UV-vertex id (tt_uv_emit's numbering)
    a.cptr = a.vperm + Vt;        // [Vt+1] rows of ccol
    a.vptr = a.cptr + (Vt + 1);   // [C+1] vertex range of a chart
    a.tptr = a.vptr + (C + 1);    // [C+1] tile range of a chart
    a.tchart = a.tptr + (C + 1);  // [NT] chart of a tile
    a.tbegin = a.tchart + NT;     // [NT] first vertex of a tile (it ends TT_UV_LSCM_TILE later or with its chart)
    return a;
}

struct LsWs {
    double4* face;  // [T] x1, x2, y2 of the local frame (p0 = 0, p1 = (x1, 0), p2 = (x2, y2)) and 1 / (4 A_f); zeros: no term
    double2* cor;   // [3T] the corner terms of the last operator application
    double2 *x, *r, *p, *q;  // [Vt] (u, v) per UV vertex
    double* invd;   // [Vt] 1 / diagonal; 0 at a pin and at a vertex that only zero-area faces use (such an entry is fixed)
    double* part;   // [4 NT] tile sums
    double *alpha, *beta, *rz, *bb, *rr;  // [C]
    double* ctr;    // [3C] centre the pin search measures from
    double* stat;   // [8C] 0 UV area, 1 3-D area, 2 scale k, 3 mean u, 4 mean v, 5 theta, 6 cos, 7 sin
    unsigned long long* dmax;  // [C] bit pattern of the largest squared distance
    int *pin, *bbox, *obox, *done, *fail, *iters;  // [2C] [6C] [4C] [C] [C] [C]
    int* active;    // [64] 0: charts still iterating
};

static LsWs ls_ws(void* base, long long T, long long Vt, long long C, long long NT, long long* bytes = nullptr) {
    TtCarver c{(char*)base};
    LsWs w;
    w.face = c.take<double4>(T);
    w.cor = c.take<double2>(3 * T);
    w.x = c.take<double2>(Vt);
    w.r = c.take<double2>(Vt);
    w.p = c.take<double2>(Vt);
    w.q = c.take<double2>(Vt);
    w.invd = c.take<double>(Vt);
    w.part = c.take<double>(4 * NT);
    w.alpha = c.take<double>(C);
    w.beta = c.take<double>(C);
    w.rz = c.take<double>(C);
    w.bb = c.take<double>(C);
    w.rr = c.take<double>(C);
    w.ctr = c.take<double>(3 * C);
    w.stat = c.take<double>(8 * C);
    w.dmax = c.take<unsigned long long>(C);
    w.pin = c.take<int>(2 * C);
    w.bbox = c.take<int>(6 * C);
    w.obox = c.take<int>(4 * C);
    w.done = c.take<int>(C);
    w.fail = c.take<int>(C);
    w.iters = c.take<int>(C);
    w.active = c.take<int>(64);
    if (bytes) *bytes = c.bytes();
    return w;
}

struct LsDim {
    int V, T, Vt, C, NT;
};

// ---------------------------------------------------------------------------------------------------------------
// small helpers
__device__ __forceinline__ int ls_cl(int i, int n) { return min(max(i, 0), n - 1); }  // a read in bounds, whatever came in

__device__ __forceinline__ int ls_ord(float x) {  // order-preserving int image of a float (tt_uv.hip's ord_of)
    const int b = __float_as_int(x);
    return b >= 0 ? b : (b ^ 0x7fffffff);
}
__device__ __forceinline__ float ls_unord(int o) { return __int_as_float(o >= 0 ? o : (o ^ 0x7fffffff)); }

// the tile of this wave: chart c, vertices [b, e); false past the last tile (the whole wave leaves)
__device__ __forceinline__ bool ls_tile(const LsTab& t, const LsDim& d, int& tile, int& c, int& b, int& e) {
    tile = blockIdx.x * LS_WAVES + (threadIdx.x >> 6);
    if (tile >= d.NT) return false;
    c = ls_cl(t.tchart[tile], d.C);
    b = min(max(t.tbegin[tile], 0), d.Vt);
    e = min(min(b + TT_UV_LSCM_TILE, max(t.vptr[c + 1], 0)), d.Vt);
    return true;
}

// the chart of this wave and its tiles [t0, t1)
__device__ __forceinline__ bool ls_chart(const LsTab& t, const LsDim& d, int& c, int& t0, int& t1) {
    c = blockIdx.x * LS_WAVES + (threadIdx.x >> 6);
    if (c >= d.C) return false;
    t0 = min(max(t.tptr[c], 0), d.NT);
    t1 = min(max(t.tptr[c + 1], t0), d.NT);
    return true;
}

// sum of slot k of the chart's tile sums: lane-strided ascending, then the shuffle tree (valid in lane 0)
__device__ __forceinline__ double ls_chart_sum(const double* __restrict__ part, int t0, int t1, int k) {
    double a = 0.0;
    for (int t = t0 + (int)(threadIdx.x & 63); t < t1; t += 64) a += part[(size_t)t * 4 + k];
    return tt_wave_sum(a);
}

// sum of a vertex's corner terms in ascending corner order
__device__ __forceinline__ double2 ls_gather(const LsTab& t, const LsDim& d, const double2* __restrict__ cor, int i) {
    const int b = min(max(t.cptr[i], 0), 3 * d.T), e = min(max(t.cptr[i + 1], b), 3 * d.T);
    double gu = 0.0, gv = 0.0;
    for (int k = b; k < e; ++k) {
        const double2 g = cor[ls_cl(t.ccol[k], 3 * d.T)];
        gu += g.x;
        gv += g.y;
    }
    return make_double2(gu, gv);
}

__device__ __forceinline__ void ls_pos(const float* __restrict__ v, const LsTab& t, const LsDim& d, int i, double p[3]) {
    const int m = ls_cl(t.vmesh[i], d.V);
    p[0] = v[(size_t)m * 3];
    p[1] = v[(size_t)m * 3 + 1];
    p[2] = v[(size_t)m * 3 + 2];
}

// W_k = (y_{k+1} - y_{k+2}, x_{k+2} - x_{k+1}) of the local triangle: grad u = (1 / 2A) sum_k u_k W_k
__device__ __forceinline__ void ls_w(const double4& F, double wx[3], double wy[3]) {
    wx[0] = -F.z;
    wy[0] = F.y - F.x;
    wx[1] = F.z;
    wy[1] = -F.y;
    wx[2] = 0.0;
    wy[2] = F.x;
}

__device__ __forceinline__ double ls_uv_area(const double2 a, const double2 b, const double2 c) {
    return 0.5 * ((b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x));
}

// ---------------------------------------------------------------------------------------------------------------
// setup
__global__ __launch_bounds__(LS_BLOCK) void k_ls_chart_init(LsDim d, LsWs w) {
    const int c = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (c == 0) w.active[0] = 0;
    if (c >= d.C) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w.bbox[(size_t)c * 6 + k] = 0x7fffffff;
        w.bbox[(size_t)c * 6 + 3 + k] = (int)0x80000000;
    }
    w.obox[(size_t)c * 4 + 0] = 0x7fffffff;
    w.obox[(size_t)c * 4 + 1] = 0x7fffffff;
    w.obox[(size_t)c * 4 + 2] = (int)0x80000000;
    w.obox[(size_t)c * 4 + 3] = (int)0x80000000;
    w.dmax[c] = 0ull;
    w.pin[2 * c] = 0x7fffffff;
    w.pin[2 * c + 1] = 0x7fffffff;
    w.done[c] = 0;
    w.fail[c] = 0;
    w.iters[c] = 0;
    w.alpha[c] = 0.0;
    w.beta[c] = 0.0;
    w.rz[c] = 0.0;
    w.bb[c] = 0.0;
    w.rr[c] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w.stat[(size_t)c * 8 + k] = 0.0;
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_bbox(const float* __restrict__ v, LsTab t, LsDim d, LsWs w) {
    const int i = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (i >= d.Vt) return;
    const int c = ls_cl(t.vchart[i], d.C), m = ls_cl(t.vmesh[i], d.V);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = ls_ord(v[(size_t)m * 3 + k]);
        atomicMin(w.bbox + (size_t)c * 6 + k, o);
        atomicMax(w.bbox + (size_t)c * 6 + 3 + k, o);
    }
}

// the centre of the pin search: mode 0 the middle of the chart's 3-D box, mode 1 the position of pin 0 (checked first)
__global__ __launch_bounds__(LS_BLOCK) void k_ls_center(const float* __restrict__ v, LsTab t, LsDim d, int mode, LsWs w) {
    const int c = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (c >= d.C) return;
    if (mode == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            w.ctr[(size_t)c * 3 + k] =
                0.5 * ((double)ls_unord(w.bbox[(size_t)c * 6 + k]) + (double)ls_unord(w.bbox[(size_t)c * 6 + 3 + k]));
    } else {
        const int first = ls_cl(t.vptr[c], d.Vt);
        if ((unsigned)w.pin[2 * c] >= (unsigned)d.Vt) {  // (a NaN position: no distance equals the maximum)
            w.pin[2 * c] = first;
            w.done[c] |= LS_NO_PINS;
        }
        double p[3];
        ls_pos(v, t, d, w.pin[2 * c], p);
#pragma unroll
        for (int k = 0; k < 3; ++k) w.ctr[(size_t)c * 3 + k] = p[k];
        w.dmax[c] = 0ull;
    }
}

__device__ __forceinline__ unsigned long long ls_dist2(const float* __restrict__ v, const LsTab& t, const LsDim& d,
                                                       const LsWs& w, int i, int c) {
    double p[3];
    ls_pos(v, t, d, i, p);
    const double dx = p[0] - w.ctr[(size_t)c * 3], dy = p[1] - w.ctr[(size_t)c * 3 + 1],
                 dz = p[2] - w.ctr[(size_t)c * 3 + 2];
    return (unsigned long long)__double_as_longlong((dx * dx + dy * dy) + dz * dz);  // >= 0: bit order = value order
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_far_max(const float* __restrict__ v, LsTab t, LsDim d, LsWs w) {
    const int i = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (i >= d.Vt) return;
    const int c = ls_cl(t.vchart[i], d.C);
    atomicMax(w.dmax + c, ls_dist2(v, t, d, w, i, c));
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_far_arg(const float* __restrict__ v, LsTab t, LsDim d, int slot,
                                                         LsWs w) {
    const int i = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (i >= d.Vt) return;
    const int c = ls_cl(t.vchart[i], d.C);
    if (ls_dist2(v, t, d, w, i, c) == w.dmax[c]) atomicMin(w.pin + 2 * c + slot, i);  // a tie: the smallest id
}

// pin 1 checked, x = the pins' values: pin 0 at (0, 0), pin 1 at (|p1 - p0|, 0); everything else starts at 0
__global__ __launch_bounds__(LS_BLOCK) void k_ls_pins(LsTab t, LsDim d, LsWs w) {
    const int c = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (c >= d.C) return;
    const double d2 = __longlong_as_double((long long)w.dmax[c]);
    if ((unsigned)w.pin[2 * c + 1] >= (unsigned)d.Vt) {
        w.pin[2 * c + 1] = w.pin[2 * c];
        w.done[c] |= LS_NO_PINS;
    }
    if (!(d2 > 0.0) || w.pin[2 * c + 1] == w.pin[2 * c]) w.done[c] |= LS_NO_PINS;  // every vertex in one point
    if (w.done[c] == 0) w.x[w.pin[2 * c + 1]] = make_double2(sqrt(d2), 0.0);
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_face(const float* __restrict__ v, LsTab t, LsDim d, LsWs w) {
    const int f = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (f >= d.T) return;
    double p0[3], p1[3], p2[3];
    ls_pos(v, t, d, ls_cl(t.fc[(size_t)f * 3], d.Vt), p0);
    ls_pos(v, t, d, ls_cl(t.fc[(size_t)f * 3 + 1], d.Vt), p1);
    ls_pos(v, t, d, ls_cl(t.fc[(size_t)f * 3 + 2], d.Vt), p2);
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double nn = (nx * nx + ny * ny) + nz * nz;  // (tt_uv_labels' zero-area rule: |n|^2 = 0)
    double4 F = make_double4(0.0, 0.0, 0.0, 0.0);
    if (nn > 0.0) {
        const double l1 = sqrt((e1x * e1x + e1y * e1y) + e1z * e1z), n = sqrt(nn);
        F.x = l1;
        F.y = ((e2x * e1x + e2y * e1y) + e2z * e1z) / l1;
        F.z = n / l1;
        F.w = 1.0 / (2.0 * n);  // 1 / (4 A_f), A_f = |n| / 2
    }
    w.face[f] = F;
}

// invd: the Jacobi preconditioner and the mask of the fixed entries in one
__global__ __launch_bounds__(LS_BLOCK) void k_ls_diag(LsTab t, LsDim d, LsWs w) {
    const int i = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (i >= d.Vt) return;
    const int c = ls_cl(t.vchart[i], d.C);
    const int b = min(max(t.cptr[i], 0), 3 * d.T), e = min(max(t.cptr[i + 1], b), 3 * d.T);
    double D = 0.0;
    for (int k = b; k < e; ++k) {
        const int q = ls_cl(t.ccol[k], 3 * d.T);
        const double4 F = w.face[q / 3];
        double wx[3], wy[3];
        ls_w(F, wx, wy);
        const int j = q % 3;
        D += F.w * (wx[j] * wx[j] + wy[j] * wy[j]);
    }
    const bool pinned = i == w.pin[2 * c] || i == w.pin[2 * c + 1];
    w.invd[i] = (D > 0.0 && !pinned) ? 1.0 / D : 0.0;
}

// the corner terms of A src = M^T (M src); faces of a chart that is done are skipped (nobody reads their terms)
__global__ __launch_bounds__(LS_BLOCK) void k_ls_face_apply(LsTab t, LsDim d, const double2* __restrict__ src,
                                                            LsWs w) {
    const int f = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (f >= d.T) return;
    int a[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = ls_cl(t.fc[(size_t)f * 3 + k], d.Vt);
    if (w.done[ls_cl(t.vchart[a[0]], d.C)] != 0) return;
    const double4 F = w.face[f];
    double wx[3], wy[3];
    ls_w(F, wx, wy);
    const double2 s0 = src[a[0]], s1 = src[a[1]], s2 = src[a[2]];
    // M src: the two components of (sum_k v_k W_k) - J (sum_k u_k W_k), J = rotation by +90 degrees
    const double rx = ((s0.y * wx[0] + s0.x * wy[0]) + (s1.y * wx[1] + s1.x * wy[1])) + (s2.y * wx[2] + s2.x * wy[2]);
    const double ry = ((s0.y * wy[0] - s0.x * wx[0]) + (s1.y * wy[1] - s1.x * wx[1])) + (s2.y * wy[2] - s2.x * wx[2]);
    const double gx = F.w * rx, gy = F.w * ry;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        w.cor[(size_t)f * 3 + k] = make_double2(wy[k] * gx - wx[k] * gy, wx[k] * gx + wy[k] * gy);
}

// b = -A x_pin on the free entries; r = b, p = D^-1 r; tile sums 0: b.b, 1: r.z
__global__ __launch_bounds__(LS_BLOCK) void k_ls_rhs(LsTab t, LsDim d, LsWs w) {
    int tile, c, b, e;
    if (!ls_tile(t, d, tile, c, b, e)) return;
    const bool live = w.done[c] == 0;  // (a chart without pins has no corner terms: b = 0)
    double sbb = 0.0, srz = 0.0;
    for (int j = 0; j < LS_PER_LANE; ++j) {
        const int i = b + (int)(threadIdx.x & 63) + 64 * j;
        if (i < e) {
            const double id = live ? w.invd[i] : 0.0;
            const double2 g = live ? ls_gather(t, d, w.cor, i) : make_double2(0.0, 0.0);
            const double2 r = id > 0.0 ? make_double2(-g.x, -g.y) : make_double2(0.0, 0.0);
            w.r[i] = r;
            w.p[i] = make_double2(r.x * id, r.y * id);
            w.q[i] = make_double2(0.0, 0.0);
            sbb += r.x * r.x + r.y * r.y;
            srz += r.x * (r.x * id) + r.y * (r.y * id);
        }
    }
    sbb = tt_wave_sum(sbb);
    srz = tt_wave_sum(srz);
    if ((threadIdx.x & 63) == 0) {
        w.part[(size_t)tile * 4] = sbb;
        w.part[(size_t)tile * 4 + 1] = srz;
    }
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_rhs_chart(LsTab t, LsDim d, LsWs w) {
    int c, t0, t1;
    if (!ls_chart(t, d, c, t0, t1)) return;
    const double sbb = ls_chart_sum(w.part, t0, t1, 0), srz = ls_chart_sum(w.part, t0, t1, 1);
    if ((threadIdx.x & 63) == 0) {
        w.bb[c] = sbb;
        w.rr[c] = sbb;
        w.rz[c] = srz;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// one CG iteration: k_ls_face_apply(p), then
__global__ __launch_bounds__(LS_BLOCK) void k_ls_q(LsTab t, LsDim d, LsWs w) {  // q = A p, tile sum 0: p.q
    int tile, c, b, e;
    if (!ls_tile(t, d, tile, c, b, e)) return;
    if (w.done[c] != 0) return;
    double spq = 0.0;
    for (int j = 0; j < LS_PER_LANE; ++j) {
        const int i = b + (int)(threadIdx.x & 63) + 64 * j;
        if (i < e) {
            const double2 g = ls_gather(t, d, w.cor, i);
            const double2 q = w.invd[i] > 0.0 ? g : make_double2(0.0, 0.0);
            const double2 p = w.p[i];
            w.q[i] = q;
            spq += p.x * q.x + p.y * q.y;
        }
    }
    spq = tt_wave_sum(spq);
    if ((threadIdx.x & 63) == 0) w.part[(size_t)tile * 4] = spq;
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_alpha(LsTab t, LsDim d, LsWs w) {
    int c, t0, t1;
    if (!ls_chart(t, d, c, t0, t1)) return;
    if (w.done[c] != 0) return;
    const double pq = ls_chart_sum(w.part, t0, t1, 0);
    if ((threadIdx.x & 63) == 0) w.alpha[c] = pq > 0.0 ? w.rz[c] / pq : 0.0;
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_update(LsTab t, LsDim d, LsWs w) {  // x, r; tile sums 1: r.z, 2: r.r
    int tile, c, b, e;
    if (!ls_tile(t, d, tile, c, b, e)) return;
    if (w.done[c] != 0) return;
    const double al = w.alpha[c];
    double srz = 0.0, srr = 0.0;
    for (int j = 0; j < LS_PER_LANE; ++j) {
        const int i = b + (int)(threadIdx.x & 63) + 64 * j;
        if (i < e) {
            const double2 p = w.p[i], q = w.q[i];
            double2 x = w.x[i], r = w.r[i];
            const double id = w.invd[i];
            x.x += al * p.x;
            x.y += al * p.y;
            r.x -= al * q.x;
            r.y -= al * q.y;
            w.x[i] = x;
            w.r[i] = r;
            srz += r.x * (r.x * id) + r.y * (r.y * id);
            srr += r.x * r.x + r.y * r.y;
        }
    }
    srz = tt_wave_sum(srz);
    srr = tt_wave_sum(srr);
    if ((threadIdx.x & 63) == 0) {
        w.part[(size_t)tile * 4 + 1] = srz;
        w.part[(size_t)tile * 4 + 2] = srr;
    }
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_beta(LsTab t, LsDim d, double tol2, LsWs w) {
    int c, t0, t1;
    if (!ls_chart(t, d, c, t0, t1)) return;
    if (w.done[c] != 0) return;
    const double srz = ls_chart_sum(w.part, t0, t1, 1), srr = ls_chart_sum(w.part, t0, t1, 2);
    if ((threadIdx.x & 63) != 0) return;
    const double rz = w.rz[c];
    w.iters[c] += 1;
    w.rr[c] = srr;
    w.beta[c] = rz > 0.0 ? srz / rz : 0.0;
    w.rz[c] = srz;
    if (srr <= tol2 * w.bb[c])  // |r| <= tol |b| (false for a NaN: such a chart never converges)
        w.done[c] = LS_CONVERGED;
    else
        atomicAdd(w.active, 1);
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_p(LsTab t, LsDim d, LsWs w) {  // p = z + beta p
    const int i = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (i >= d.Vt) return;
    const int c = ls_cl(t.vchart[i], d.C);
    if (w.done[c] != 0) return;
    const double be = w.beta[c], id = w.invd[i];
    const double2 r = w.r[i], p = w.p[i];
    w.p[i] = make_double2(r.x * id + be * p.x, r.y * id + be * p.y);
}

__global__ void k_ls_zero_active(LsWs w) {
    if (threadIdx.x == 0) w.active[0] = 0;
}

// charts that neither converged nor failed their pins
__global__ __launch_bounds__(LS_BLOCK) void k_ls_count_open(LsDim d, LsWs w) {
    const int c = blockIdx.x * LS_BLOCK + threadIdx.x;
    const int open = (c < d.C && w.done[min(c, d.C - 1)] == 0) ? 1 : 0;
    const int k = tt_wave_sum(open);
    if ((threadIdx.x & 63) == 0 && k > 0) atomicAdd(w.active, k);
}

__global__ void k_ls_active_out(LsWs w, int* __restrict__ out_totals) {
    if (threadIdx.x == 0) out_totals[0] = w.active[0];
}

// ---------------------------------------------------------------------------------------------------------------
// finish.  A face belongs to the UV vertex of its corner 0, so the per-face sums ride on the vertex tiles.
__global__ __launch_bounds__(LS_BLOCK) void k_ls_area(LsTab t, LsDim d, LsWs w) {  // tile sums: UV area, area, sum u, sum v
    int tile, c, b, e;
    if (!ls_tile(t, d, tile, c, b, e)) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < LS_PER_LANE; ++j) {
        const int i = b + (int)(threadIdx.x & 63) + 64 * j;
        if (i < e) {
            const int kb = min(max(t.cptr[i], 0), 3 * d.T), ke = min(max(t.cptr[i + 1], kb), 3 * d.T);
            for (int k = kb; k < ke; ++k) {
                const int q = ls_cl(t.ccol[k], 3 * d.T);
                const double4 F = w.face[q / 3];
                if (q % 3 != 0 || !(F.w > 0.0)) continue;
                const int f = q / 3;
                s[0] += ls_uv_area(w.x[i], w.x[ls_cl(t.fc[(size_t)f * 3 + 1], d.Vt)],
                                   w.x[ls_cl(t.fc[(size_t)f * 3 + 2], d.Vt)]);
                s[1] += 0.5 * (F.x * F.z);
            }
            const double2 x = w.x[i];
            s[2] += x.x;
            s[3] += x.y;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s[k] = tt_wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) w.part[(size_t)tile * 4 + k] = s[k];
    }
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_scale(LsTab t, LsDim d, LsWs w) {
    int c, t0, t1;
    if (!ls_chart(t, d, c, t0, t1)) return;
    double s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = ls_chart_sum(w.part, t0, t1, k);
    if ((threadIdx.x & 63) != 0) return;
    const int n = max(t.vptr[c + 1] - t.vptr[c], 1);
    const double k2 = s[1] / s[0];
    const bool ok = s[0] > 0.0 && s[1] > 0.0 && k2 > 0.0 && k2 < 1.0e300;  // (false for a NaN, an infinity)
    if (!ok) w.fail[c] |= LS_BAD_AREA;
    double* st = w.stat + (size_t)c * 8;
    st[0] = s[0];
    st[1] = s[1];
    st[2] = ok ? sqrt(k2) : 1.0;
    st[3] = s[2] / (double)n;
    st[4] = s[3] / (double)n;
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_cov(LsTab t, LsDim d, LsWs w) {  // tile sums: du du, du dv, dv dv
    int tile, c, b, e;
    if (!ls_tile(t, d, tile, c, b, e)) return;
    const double mu = w.stat[(size_t)c * 8 + 3], mv = w.stat[(size_t)c * 8 + 4];
    double s[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < LS_PER_LANE; ++j) {
        const int i = b + (int)(threadIdx.x & 63) + 64 * j;
        if (i < e) {
            const double2 x = w.x[i];
            const double du = x.x - mu, dv = x.y - mv;
            s[0] += du * du;
            s[1] += du * dv;
            s[2] += dv * dv;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = tt_wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) w.part[(size_t)tile * 4 + k] = s[k];
    }
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_rot(LsTab t, LsDim d, LsWs w) {
    int c, t0, t1;
    if (!ls_chart(t, d, c, t0, t1)) return;
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = ls_chart_sum(w.part, t0, t1, k);
    if ((threadIdx.x & 63) != 0) return;
    // the principal axis sits at theta = atan2(2 s_uv, s_uu - s_vv) / 2 (atan2(0, 0) = 0: a tie turns nothing)
    double th = 0.5 * atan2(2.0 * s[1], s[0] - s[2]);
    if (!(th >= -4.0 && th <= 4.0)) th = 0.0;
    double* st = w.stat + (size_t)c * 8;
    st[5] = th;
    st[6] = cos(th);
    st[7] = sin(th);
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_check(LsTab t, LsDim d, double tau, LsWs w) {
    const int f = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (f >= d.T) return;
    int a[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = ls_cl(t.fc[(size_t)f * 3 + k], d.Vt);
    const int c = ls_cl(t.vchart[a[0]], d.C);
    const double4 F = w.face[f];
    if (w.done[c] != LS_CONVERGED || !(F.w > 0.0)) return;
    const double k = w.stat[(size_t)c * 8 + 2];
    const double auv = ls_uv_area(w.x[a[0]], w.x[a[1]], w.x[a[2]]);
    const double ratio = ((k * k) * auv) / (0.5 * (F.x * F.z));
    if (!(auv > 0.0) || !(ratio >= tau && ratio <= 1.0 / tau)) atomicOr(w.fail + c, LS_BAD_FACE);
}

// the raw solution, and the final fp32 coordinates R k (u, v) of the accepted charts with their boxes
__global__ __launch_bounds__(LS_BLOCK) void k_ls_final(LsTab t, LsDim d, LsWs w, double* __restrict__ uv64,
                                                       float* __restrict__ uvf) {
    const int i = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (i >= d.Vt) return;
    const int c = ls_cl(t.vchart[i], d.C), id = ls_cl(t.vperm[i], d.Vt);
    const double2 x = w.x[i];
    uv64[(size_t)id * 2] = x.x;
    uv64[(size_t)id * 2 + 1] = x.y;
    float fu = 0.f, fv = 0.f;
    if (w.done[c] == LS_CONVERGED && w.fail[c] == 0) {
        const double* st = w.stat + (size_t)c * 8;
        fu = (float)(st[2] * (st[6] * x.x + st[7] * x.y));  // rotation by -theta: the principal axis onto u
        fv = (float)(st[2] * (st[6] * x.y - st[7] * x.x));
        atomicMin(w.obox + (size_t)c * 4 + 0, ls_ord(fu));
        atomicMin(w.obox + (size_t)c * 4 + 1, ls_ord(fv));
        atomicMax(w.obox + (size_t)c * 4 + 2, ls_ord(fu));
        atomicMax(w.obox + (size_t)c * 4 + 3, ls_ord(fv));
    }
    uvf[(size_t)id * 2] = fu;
    uvf[(size_t)id * 2 + 1] = fv;
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_out(LsTab t, LsDim d, LsWs w, const float* __restrict__ box_in,
                                                     float* __restrict__ box_out, unsigned char* __restrict__ fallback,
                                                     int* __restrict__ pins, int* __restrict__ iterations,
                                                     double* __restrict__ residual, double* __restrict__ rotation,
                                                     double* __restrict__ scale) {
    const int c = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (c >= d.C) return;
    const bool ok = w.done[c] == LS_CONVERGED && w.fail[c] == 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        box_out[(size_t)c * 4 + k] = ok ? ls_unord(w.obox[(size_t)c * 4 + k]) : (box_in ? box_in[(size_t)c * 4 + k] : 0.f);
    fallback[c] = ok ? 0 : 1;
    pins[2 * c] = ls_cl(t.vperm[ls_cl(w.pin[2 * c], d.Vt)], d.Vt);
    pins[2 * c + 1] = ls_cl(t.vperm[ls_cl(w.pin[2 * c + 1], d.Vt)], d.Vt);
    iterations[c] = w.iters[c];
    residual[c] = w.bb[c] > 0.0 ? sqrt(w.rr[c] / w.bb[c]) : 0.0;
    rotation[c] = ok ? -w.stat[(size_t)c * 8 + 5] : 0.0;
    scale[c] = ok ? w.stat[(size_t)c * 8 + 2] : 1.0;
}

// in-plane coordinates of label l, as tt_uv.hip's uv_axes
__device__ __forceinline__ void ls_axes(int l, int& cu, int& cv) {
    const int a = l >> 1, p = (a + 1) % 3, q = (a + 2) % 3;
    cu = (l & 1) ? q : p;
    cv = (l & 1) ? p : q;
}

// every corner writes its UV vertex (the corners of one (chart, vertex) pair write the same bits)
__global__ __launch_bounds__(LS_BLOCK) void k_ls_emit(const float* __restrict__ v, const int* __restrict__ tri,
                                                      const int* __restrict__ labels, const int* __restrict__ chart,
                                                      const int* __restrict__ t_tex, const float* __restrict__ uvf,
                                                      const unsigned char* __restrict__ fallback,
                                                      const float* __restrict__ chart_box,
                                                      const int* __restrict__ offsets, int C, float scale, int V, int T,
                                                      int Vt, int N, int pad, float* __restrict__ v_tex) {
    const int q = blockIdx.x * LS_BLOCK + threadIdx.x;
    if (q >= 3 * T) return;
    const int id = t_tex[q];
    if ((unsigned)id >= (unsigned)Vt) return;
    const int f = q / 3;
    const int c = (int)min((unsigned)chart[f], (unsigned)(C - 1));
    float pu, pv;
    if (fallback[c]) {  // tt_uv_emit's projection of the chart's label
        const int vi = (int)min((unsigned)tri[q], (unsigned)(V - 1));
        int cu, cv;
        ls_axes(min(max(labels[f], 0), 5), cu, cv);
        pu = v[(size_t)vi * 3 + cu];
        pv = v[(size_t)vi * 3 + cv];
    } else {
        pu = uvf[(size_t)id * 2];
        pv = uvf[(size_t)id * 2 + 1];
    }
    const float U = ((float)(offsets[2 * c] + pad) + 0.5f) + (pu - chart_box[(size_t)c * 4 + 0]) * scale;
    const float W = ((float)(offsets[2 * c + 1] + pad) + 0.5f) + (pv - chart_box[(size_t)c * 4 + 1]) * scale;
    v_tex[(size_t)id * 2] = U / (float)N;
    v_tex[(size_t)id * 2 + 1] = W / (float)N;
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
static bool ls_sizes_ok(int32_t V, int32_t T, int32_t Vt, int32_t C, int32_t NT) {
    // every chart has a vertex and a tile; a tile has a vertex
    return V >= 1 && V <= TT_MESH_MAX_ITEMS && T >= 1 && T <= TT_UV_MAX_FACES && Vt >= 1 && (int64_t)Vt <= 3 * (int64_t)T &&
           C >= 1 && C <= T && C <= Vt && NT >= C && NT <= Vt;
}

static unsigned ls_wave_grid(long long n) { return (unsigned)((n + LS_WAVES - 1) / LS_WAVES); }

extern "C" int64_t tt_uv_lscm_workspace_bytes(int32_t T, int32_t Vt, int32_t C, int32_t NT) {
    if (!ls_sizes_ok(1, T, Vt, C, NT)) return TT_ERR_BAD_ARG;
    long long bytes;
    ls_ws(nullptr, T, Vt, C, NT, &bytes);
    return bytes;
}

extern "C" int64_t tt_uv_lscm_table_ints(int32_t T, int32_t Vt, int32_t C, int32_t NT) {
    if (!ls_sizes_ok(1, T, Vt, C, NT)) return TT_ERR_BAD_ARG;
    return 6 * (int64_t)T + 3 * (int64_t)Vt + ((int64_t)Vt + 1) + 2 * ((int64_t)C + 1) + 2 * (int64_t)NT;  // ls_tab's end
}

extern "C" int tt_uv_lscm_setup(const float* v_pos, const int32_t* tables, int32_t V, int32_t T, int32_t Vt, int32_t C,
                                int32_t NT, void* workspace, void* stream) {
    if (!ls_sizes_ok(V, T, Vt, C, NT) || !v_pos || !tables || !workspace) return TT_ERR_BAD_ARG;
    const LsTab t = ls_tab(tables, T, Vt, C, NT);
    const LsWs w = ls_ws(workspace, T, Vt, C, NT);
    const LsDim d{V, T, Vt, C, NT};
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(LS_BLOCK);
    hipMemsetAsync(w.x, 0, sizeof(double2) * (size_t)Vt, s);  // (all-zero bits are 0.0)
    hipLaunchKernelGGL(k_ls_chart_init, dim3(tt_grid(C)), blk, 0, s, d, w);
    hipLaunchKernelGGL(k_ls_bbox, dim3(tt_grid(Vt)), blk, 0, s, v_pos, t, d, w);
    for (int mode = 0; mode < 2; ++mode) {
        hipLaunchKernelGGL(k_ls_center, dim3(tt_grid(C)), blk, 0, s, v_pos, t, d, mode, w);
        hipLaunchKernelGGL(k_ls_far_max, dim3(tt_grid(Vt)), blk, 0, s, v_pos, t, d, w);
        hipLaunchKernelGGL(k_ls_far_arg, dim3(tt_grid(Vt)), blk, 0, s, v_pos, t, d, mode, w);
    }
    hipLaunchKernelGGL(k_ls_pins, dim3(tt_grid(C)), blk, 0, s, t, d, w);
    hipLaunchKernelGGL(k_ls_face, dim3(tt_grid(T)), blk, 0, s, v_pos, t, d, w);
    hipLaunchKernelGGL(k_ls_diag, dim3(tt_grid(Vt)), blk, 0, s, t, d, w);
    hipLaunchKernelGGL(k_ls_face_apply, dim3(tt_grid(T)), blk, 0, s, t, d, (const double2*)w.x, w);
    hipLaunchKernelGGL(k_ls_rhs, dim3(ls_wave_grid(NT)), blk, 0, s, t, d, w);
    hipLaunchKernelGGL(k_ls_rhs_chart, dim3(ls_wave_grid(C)), blk, 0, s, t, d, w);
    return tt_check_launch();
}

extern "C" int tt_uv_lscm_iterate(const int32_t* tables, int32_t T, int32_t Vt, int32_t C, int32_t NT, int32_t n_iters,
                                  double tol, void* workspace, int32_t* out_totals, void* stream) {
    if (!ls_sizes_ok(1, T, Vt, C, NT) || !tables || !workspace || !out_totals) return TT_ERR_BAD_ARG;
    if (n_iters < 0 || n_iters > TT_UV_LSCM_MAX_BATCH || !(tol >= 0.0 && tol < 1.0)) return TT_ERR_BAD_ARG;
    const LsTab t = ls_tab(tables, T, Vt, C, NT);
    const LsWs w = ls_ws(workspace, T, Vt, C, NT);
    const LsDim d{1, T, Vt, C, NT};
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(LS_BLOCK);
    const double tol2 = tol * tol;
    for (int it = 0; it < n_iters; ++it) {
        hipLaunchKernelGGL(k_ls_face_apply, dim3(tt_grid(T)), blk, 0, s, t, d, (const double2*)w.p, w);
        hipLaunchKernelGGL(k_ls_q, dim3(ls_wave_grid(NT)), blk, 0, s, t, d, w);
        hipLaunchKernelGGL(k_ls_alpha, dim3(ls_wave_grid(C)), blk, 0, s, t, d, w);
        hipLaunchKernelGGL(k_ls_update, dim3(ls_wave_grid(NT)), blk, 0, s, t, d, w);
        hipLaunchKernelGGL(k_ls_beta, dim3(ls_wave_grid(C)), blk, 0, s, t, d, tol2, w);
        hipLaunchKernelGGL(k_ls_p, dim3(tt_grid(Vt)), blk, 0, s, t, d, w);
    }
    // the charts still iterating, counted afresh (so n_iters = 0 reports them too)
    hipLaunchKernelGGL(k_ls_zero_active, dim3(1), dim3(64), 0, s, w);
    hipLaunchKernelGGL(k_ls_count_open, dim3(tt_grid(C)), blk, 0, s, d, w);
    hipLaunchKernelGGL(k_ls_active_out, dim3(1), dim3(64), 0, s, w, (int*)out_totals);
    return tt_check_launch();
}

extern "C" int tt_uv_lscm_finish(const int32_t* tables, const float* chart_box, int32_t T, int32_t Vt, int32_t C,
                                 int32_t NT, float tau, void* workspace, double* uv, float* uv_final, float* box_out,
                                 uint8_t* fallback, int32_t* pins, int32_t* iterations, double* residual,
                                 double* rotation, double* scale, void* stream) {
    if (!ls_sizes_ok(1, T, Vt, C, NT) || !tables || !workspace) return TT_ERR_BAD_ARG;
    if (!(tau > 0.f && tau <= TT_UV_MAX_TAU)) return TT_ERR_BAD_ARG;
    if (!uv || !uv_final || !box_out || !fallback || !pins || !iterations || !residual || !rotation || !scale)
        return TT_ERR_BAD_ARG;
    const LsTab t = ls_tab(tables, T, Vt, C, NT);
    const LsWs w = ls_ws(workspace, T, Vt, C, NT);
    const LsDim d{1, T, Vt, C, NT};
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(LS_BLOCK);
    hipLaunchKernelGGL(k_ls_area, dim3(ls_wave_grid(NT)), blk, 0, s, t, d, w);
    hipLaunchKernelGGL(k_ls_scale, dim3(ls_wave_grid(C)), blk, 0, s, t, d, w);
    hipLaunchKernelGGL(k_ls_cov, dim3(ls_wave_grid(NT)), blk, 0, s, t, d, w);
    hipLaunchKernelGGL(k_ls_rot, dim3(ls_wave_grid(C)), blk, 0, s, t, d, w);
    hipLaunchKernelGGL(k_ls_check, dim3(tt_grid(T)), blk, 0, s, t, d, (double)tau, w);
    hipLaunchKernelGGL(k_ls_final, dim3(tt_grid(Vt)), blk, 0, s, t, d, w, uv, uv_final);
    hipLaunchKernelGGL(k_ls_out, dim3(tt_grid(C)), blk, 0, s, t, d, w, chart_box, box_out, (unsigned char*)fallback,
                       (int*)pins, (int*)iterations, residual, rotation, scale);
    return tt_check_launch();
}

extern "C" int tt_uv_lscm_emit(const float* v_pos, const int32_t* t_pos_idx, const int32_t* labels,
                               const int32_t* chart, const int32_t* t_tex_idx, const float* uv_final,
                               const uint8_t* fallback, const float* chart_box, const int32_t* offsets, int32_t C,
                               float scale, int32_t V, int32_t T, int32_t Vt, int32_t N, int32_t padding, float* v_tex,
                               void* stream) {
    if (V < 1 || V > TT_MESH_MAX_ITEMS || T < 1 || T > TT_UV_MAX_FACES || N < 1 || N > TT_UV_MAX_TEX) return TT_ERR_BAD_ARG;
    if (C < 1 || C > T || Vt < 1 || (int64_t)Vt > 3 * (int64_t)T || padding < 0 || padding > TT_UV_MAX_PADDING)
        return TT_ERR_BAD_ARG;
    if (!(scale >= 0.f && scale <= 3.0e38f)) return TT_ERR_BAD_ARG;
    if (!v_pos || !t_pos_idx || !labels || !chart || !t_tex_idx || !uv_final || !fallback || !chart_box || !offsets ||
        !v_tex)
        return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_ls_emit, dim3(tt_grid(3ll * T)), dim3(LS_BLOCK), 0, (hipStream_t)stream, v_pos,
                       (const int*)t_pos_idx, (const int*)labels, (const int*)chart, (const int*)t_tex_idx, uv_final,
                       (const unsigned char*)fallback, chart_box, (const int*)offsets, (int)C, scale, (int)V, (int)T,
                       (int)Vt, (int)N, (int)padding, v_tex);
    return tt_check_launch();
}
