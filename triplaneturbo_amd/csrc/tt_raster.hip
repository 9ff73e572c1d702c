// tt_raster.hip -- differentiable triangle rasterization, attribute interpolation and silhouette antialiasing: the
// drop-in for the three nvdiffrast primitives (CUDA-only) that the reference's mesh renderer calls through
// NVDiffRasterizerContext (threestudio/utils/rasterize.py; generative_space_mesh_rasterize_renderer.py:137-295).
// Instance mode: one topology tri (T,3) shared by B views of clip-space positions pos (B,V,4).  Range mode: one
// vertex buffer pos (V,4) and per image a range (first, count) of tri; the kernels are the same, the work list of the
// forward is mapped to (image, triangle) by rast_slot and pos is read with a batch stride of 0.  The contract (pixel
// centres, coverage, tie rule, depth test, antialias pairs) is written in include/tt_abi.h.
//
// Rasterize, five launches (range mode: four more for the images' slot prefix), no host round trip:
//   k_rast_setup      per (image, triangle) slot: clip culling and a clamped screen bounding box; its pixel count
//   tt_exclusive_scan (tt_scan.h, three launches)    exclusive int64 scan of the counts -> candidate offsets
//   k_rast_cover      grid-stride over the candidates (triangle, pixel), total read on the device: coverage by the
//                     homogeneous edge functions, then a 64-bit atomicMin of (ordered z/w bits << 32 | tri) into the
//                     pixel's key.  Min is order-independent, so the result is bit-reproducible.
//   k_rast_resolve    per pixel: the winner's (u, v, z/w) recomputed by the same function as the coverage test
// Interpolate and antialias are per-pixel gathers; their vertex gradients (grad_pos, grad_attr) use fp32 atomics.
#include "tt_host.h"
#include "tt_scan.h"

#pragma clang fp contract(off)  // edge functions exactly as written: shared edges must see exactly negated values

#define RS_BLOCK 256

#include "tt_raster_cover.h"  // TriSetup, tri_setup, tri_cover, pix_ndc: shared with tt_uv.hip

// ---------------------------------------------------------------------------------------------------------------
// rasterize forward

struct RastLayout {
    int4* bbox;
    long long *offs, *bsum;
    unsigned long long* keys;
    long long *prefix, *psum;  // range mode only
    long long n, bytes;        // (image, triangle) slots, size of the workspace
};

// the workspace sections (tt_rast_workspace_bytes, tt_rast_range_workspace_bytes) for n slots (instance mode: B T,
// range mode: the sum of the counts); base may be null for the size alone
static RastLayout rast_layout(void* base, int B, long long n, int H, int W, bool range) {
    TtCarver c{(char*)base};
    RastLayout l;
    l.n = n;
    l.bbox = c.take<int4>(l.n);                                 // [n] clamped screen box of the slot
    l.offs = c.take<long long>(l.n + 1);                        // [n + 1] pixel counts, scanned in place; [n] = total
    l.bsum = c.take<long long>(tt_xscan_blocks(l.n) + 1);       // scratch of the scan
    l.keys = c.take<unsigned long long>((long long)B * H * W);  // per pixel: ordered z/w bits << 32 | tri, min wins
    l.prefix = l.psum = nullptr;
    if (range) {
        l.prefix = c.take<long long>((long long)B + 1);         // [B + 1] the images' counts, scanned in place
        l.psum = c.take<long long>(tt_xscan_blocks(B) + 1);     // scratch of that scan
    }
    l.bytes = c.bytes();
    return l;
}

// The forward's work list: slot i -> image b, triangle t (an index into the whole tri) and the batch index pb of its
// positions.  Instance mode (prefix null): the B T (view, triangle) pairs, b = i / T, t = i % T, pb = b.  Range mode:
// image b owns the slots prefix[b] <= i < prefix[b + 1], t = first_b + (i - prefix[b]), pb = 0.
struct RastSlots {
    const long long* prefix;  // (B + 1) exclusive scan of the ranges' counts
    const int* ranges;        // (B, 2) = (first, count)
    int B, T;
};

// false: no such slot (only if the device ranges differ from the ones the host sized the work list by)
__device__ __forceinline__ bool rast_slot(const RastSlots& m, long long i, int& b, int& t, int& pb) {
    if (!m.prefix) {
        b = (int)(i / m.T);
        t = (int)(i % m.T);
        pb = b;
        return true;
    }
    // the image with prefix[b] <= i < prefix[b + 1] (the last of equal prefixes: a non-empty range)
    int lo = 0, hi = m.B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (m.prefix[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const long long local = i - m.prefix[lo];
    b = lo;
    pb = 0;
    t = m.ranges[2 * lo] + (int)local;
    return local < (long long)m.ranges[2 * lo + 1] && (unsigned)t < (unsigned)m.T;
}

// range mode: the images' counts as the input of the prefix scan
__global__ __launch_bounds__(RS_BLOCK) void k_rast_range_counts(const int* __restrict__ ranges, int B,
                                                                long long* __restrict__ cnt) {
    const int b = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (b < B) cnt[b] = ranges[2 * b + 1] > 0 ? ranges[2 * b + 1] : 0;
}

__global__ __launch_bounds__(RS_BLOCK) void k_rast_setup(const float* __restrict__ pos, const int* __restrict__ tri,
                                                         RastSlots m, long long n, int V, int H, int W,
                                                         int4* __restrict__ bbox, long long* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= n) return;
    int b, t, pb;
    TriSetup s;
    long long area = 0;
    int4 bb = make_int4(0, 0, -1, -1);
    if (rast_slot(m, i, b, t, pb) && tri_setup(pos, tri, pb, t, V, s)) {
        // culled if all vertices lie beyond one clip plane, or all w <= 0
        bool cull = (s.w[0] <= 0.f && s.w[1] <= 0.f && s.w[2] <= 0.f);
        cull |= (s.x[0] > s.w[0] && s.x[1] > s.w[1] && s.x[2] > s.w[2]);
        cull |= (s.x[0] < -s.w[0] && s.x[1] < -s.w[1] && s.x[2] < -s.w[2]);
        cull |= (s.y[0] > s.w[0] && s.y[1] > s.w[1] && s.y[2] > s.w[2]);
        cull |= (s.y[0] < -s.w[0] && s.y[1] < -s.w[1] && s.y[2] < -s.w[2]);
        cull |= (s.z[0] > s.w[0] && s.z[1] > s.w[1] && s.z[2] > s.w[2]);
        cull |= (s.z[0] < -s.w[0] && s.z[1] < -s.w[1] && s.z[2] < -s.w[2]);
        if (!cull) {
            if (s.w[0] > 0.f && s.w[1] > 0.f && s.w[2] > 0.f) {
                float x0 = 3.4e38f, x1 = -3.4e38f, y0 = 3.4e38f, y1 = -3.4e38f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    // pixel coordinate whose centre samples NDC X: ((X + 1) W - 1) / 2
                    const float px = ((s.x[k] / s.w[k] + 1.f) * (float)W - 1.f) * 0.5f;
                    const float py = ((s.y[k] / s.w[k] + 1.f) * (float)H - 1.f) * 0.5f;
                    x0 = fminf(x0, px);
                    x1 = fmaxf(x1, px);
                    y0 = fminf(y0, py);
                    y1 = fmaxf(y1, py);
                }
                // one pixel of margin against rounding (the coverage test is exact; the box only bounds it), clamped
                // in float before the conversion
                x0 = fminf(fmaxf(floorf(x0) - 1.f, 0.f), (float)W);
                x1 = fminf(fmaxf(ceilf(x1) + 1.f, -1.f), (float)(W - 1));
                y0 = fminf(fmaxf(floorf(y0) - 1.f, 0.f), (float)H);
                y1 = fminf(fmaxf(ceilf(y1) + 1.f, -1.f), (float)(H - 1));
                bb = make_int4((int)x0, (int)y0, (int)x1, (int)y1);
            } else {  // straddles w = 0 (rare): the whole screen
                bb = make_int4(0, 0, W - 1, H - 1);
            }
            if (bb.z >= bb.x && bb.w >= bb.y) area = (long long)(bb.z - bb.x + 1) * (bb.w - bb.y + 1);
        }
    }
    bbox[i] = bb;
    cnt[i] = area;
}

__device__ __forceinline__ unsigned ordered_bits(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(RS_BLOCK) void k_rast_cover(const float* __restrict__ pos, const int* __restrict__ tri,
                                                         RastSlots m, int V, int H, int W,
                                                         const int4* __restrict__ bbox,
                                                         const long long* __restrict__ offs, long long n,
                                                         unsigned long long* __restrict__ keys) {
    const long long total = offs[n];  // read on the device: no host round trip, capturable
    const long long stride = (long long)gridDim.x * RS_BLOCK;
    for (long long c = (long long)blockIdx.x * RS_BLOCK + threadIdx.x; c < total; c += stride) {
        // the (image, triangle) slot i with offs[i] <= c < offs[i + 1] (the last of equal offsets: a non-empty box)
        long long lo = 0, hi = n - 1;
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= c) lo = mid;
            else hi = mid - 1;
        }
        const int4 bb = bbox[lo];
        const long long local = c - offs[lo];
        const int bw = bb.z - bb.x + 1;
        const int px = bb.x + (int)(local % bw), py = bb.y + (int)(local / bw);
        if (px > bb.z || py > bb.w) continue;  // cannot happen for a consistent scan; keeps every store in bounds
        int b, t, pb;
        TriSetup s;
        if (!rast_slot(m, lo, b, t, pb) || !tri_setup(pos, tri, pb, t, V, s)) continue;
        float u, v, zw, S;
        if (!tri_cover(s, pix_ndc(px, W), pix_ndc_lo(px, W), pix_ndc(py, H), pix_ndc_lo(py, H), u, v, zw, S)) continue;
        // zw + 0: -0 becomes +0, so that the key ranks the two zeros as the equal depths they are (ordered_bits alone
        // puts -0 in front)
        const unsigned long long key = ((unsigned long long)ordered_bits(zw + 0.f) << 32) | (unsigned)t;
        atomicMin(keys + ((long long)b * H + py) * W + px, key);
    }
}

__global__ __launch_bounds__(RS_BLOCK) void k_rast_resolve(const float* __restrict__ pos, int pos_batch,
                                                           const int* __restrict__ tri, int B, int V, int T, int H, int W,
                                                           const unsigned long long* __restrict__ keys,
                                                           float* __restrict__ rast) {
    const long long p = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= (long long)B * H * W) return;
    const int b = (int)(p / ((long long)H * W));
    const int rem = (int)(p % ((long long)H * W));
    const int py = rem / W, px = rem % W;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned long long key = keys[p];
    if (key != ~0ull) {
        const int t = (int)(unsigned)(key & 0xffffffffu);
        TriSetup s;
        float u, v, zw, S;
        if (t < T && tri_setup(pos, tri, pos_batch == 1 ? 0 : b, t, V, s) &&
            tri_cover(s, pix_ndc(px, W), pix_ndc_lo(px, W), pix_ndc(py, H), pix_ndc_lo(py, H), u, v, zw, S))
            out = make_float4(u, v, zw + 0.f, (float)(t + 1));  // the depth of the key: never -0
    }
    reinterpret_cast<float4*>(rast)[p] = out;
}

// ---------------------------------------------------------------------------------------------------------------
// rasterize backward: d(u, v) / d(x, y, w) of the three vertices (z receives nothing)

__device__ __forceinline__ int pix_tri(float id, int T) {
    // id channel: tri + 1 (0 = empty); anything that is not a valid id is empty.  (Clamped in float, then ONE
    // compare and select: a select on two combined compares is the lane-mask shape tools/mask_hazard_lint.py flags.)
    const int t = (int)fminf(fmaxf(id, 0.f), 33554432.f) - 1;
    return t >= T ? -1 : t;
}

__global__ __launch_bounds__(RS_BLOCK) void k_rast_bwd(const float* __restrict__ pos, int pos_batch,
                                                       const int* __restrict__ tri, const float* __restrict__ rast,
                                                       const float* __restrict__ grad_rast, int B, int V, int T, int H,
                                                       int W, float* __restrict__ grad_pos) {
    const long long p = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= (long long)B * H * W) return;
    const float4 r = reinterpret_cast<const float4*>(rast)[p];
    const int t = pix_tri(r.w, T);
    if (t < 0) return;
    const float4 g = reinterpret_cast<const float4*>(grad_rast)[p];
    if (g.x == 0.f && g.y == 0.f) return;
    const int b = (int)(p / ((long long)H * W));
    const int pb = pos_batch == 1 ? 0 : b;  // range mode: one vertex buffer, the images' gradients sum in it
    const int rem = (int)(p % ((long long)H * W));
    const int py = rem / W, px = rem % W;
    TriSetup s;
    float u, v, zw, sum;
    if (!tri_setup(pos, tri, pb, t, V, s)) return;
    if (!tri_cover(s, pix_ndc(px, W), pix_ndc_lo(px, W), pix_ndc(py, H), pix_ndc_lo(py, H), u, v, zw, sum)) return;
    const float base = g.x * u + g.y * v;
    float ge[3];  // d loss / d e_k, e_k = (v_i x v_j) . p in cyclic order (u = sign(D) e_0 / sum, v likewise)
    ge[0] = s.sd * (g.x - base) / sum;
    ge[1] = s.sd * (g.y - base) / sum;
    ge[2] = s.sd * (-base) / sum;
    const float P[3] = {pix_ndc(px, W), pix_ndc(py, H), 1.f};
    float acc[3][3] = {};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        float c[3];
        // d e_k / d v_i = v_j x p ; d e_k / d v_j = p x v_i
        cross3(s.x[j], s.y[j], s.w[j], P[0], P[1], P[2], c);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[i][q] += ge[k] * c[q];
        cross3(P[0], P[1], P[2], s.x[i], s.y[i], s.w[i], c);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[j][q] += ge[k] * c[q];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float* gp = grad_pos + ((long long)pb * V + s.idx[k]) * 4;
        atomicAdd(gp + 0, acc[k][0]);
        atomicAdd(gp + 1, acc[k][1]);
        atomicAdd(gp + 3, acc[k][2]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// interpolate

__global__ __launch_bounds__(RS_BLOCK) void k_interp_fwd(const float* __restrict__ attr, int attr_batch,
                                                         const float* __restrict__ rast, const int* __restrict__ tri,
                                                         int B, int V, int T, int H, int W, int C,
                                                         float* __restrict__ out) {
    const long long p = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= (long long)B * H * W) return;
    const float4 r = reinterpret_cast<const float4*>(rast)[p];
    const int t = pix_tri(r.w, T);
    int idx[3];
    float* o = out + p * C;
    if (t < 0 || !tri_indices(tri, t, V, idx)) {
        for (int c = 0; c < C; ++c) o[c] = 0.f;
        return;
    }
    const int b = (int)(p / ((long long)H * W));
    const long long ab = attr_batch == 1 ? 0 : b;
    const float w2 = 1.f - r.x - r.y;
    const float* a0 = attr + (ab * V + idx[0]) * C;
    const float* a1 = attr + (ab * V + idx[1]) * C;
    const float* a2 = attr + (ab * V + idx[2]) * C;
    for (int c = 0; c < C; ++c) o[c] = (r.x * a0[c] + r.y * a1[c]) + w2 * a2[c];
}

__global__ __launch_bounds__(RS_BLOCK) void k_interp_bwd(const float* __restrict__ attr, int attr_batch,
                                                         const float* __restrict__ rast, const int* __restrict__ tri,
                                                         const float* __restrict__ grad_out, int B, int V, int T,
                                                         int H, int W, int C, float* __restrict__ grad_attr,
                                                         float* __restrict__ grad_rast) {
    const long long p = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= (long long)B * H * W) return;
    const float4 r = reinterpret_cast<const float4*>(rast)[p];
    const int t = pix_tri(r.w, T);
    int idx[3];
    float gu = 0.f, gv = 0.f;
    if (t >= 0 && tri_indices(tri, t, V, idx)) {
        const int b = (int)(p / ((long long)H * W));
        const long long ab = attr_batch == 1 ? 0 : b;
        const float w2 = 1.f - r.x - r.y;
        const float* a0 = attr + (ab * V + idx[0]) * C;
        const float* a1 = attr + (ab * V + idx[1]) * C;
        const float* a2 = attr + (ab * V + idx[2]) * C;
        float* g0 = grad_attr ? grad_attr + (ab * V + idx[0]) * C : nullptr;
        float* g1 = grad_attr ? grad_attr + (ab * V + idx[1]) * C : nullptr;
        float* g2 = grad_attr ? grad_attr + (ab * V + idx[2]) * C : nullptr;
        const float* go = grad_out + p * C;
        for (int c = 0; c < C; ++c) {
            const float g = go[c];
            gu += g * (a0[c] - a2[c]);
            gv += g * (a1[c] - a2[c]);
            if (g0 && g != 0.f) {
                atomicAdd(g0 + c, r.x * g);
                atomicAdd(g1 + c, r.y * g);
                atomicAdd(g2 + c, w2 * g);
            }
        }
    }
    if (grad_rast) reinterpret_cast<float4*>(grad_rast)[p] = make_float4(gu, gv, 0.f, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------
// antialias (Laine et al. 2020, section 4.3; contract in tt_abi.h)

struct AaCtx {
    const float* rast;
    const float* pos;
    const int* tri;
    const int* edge_ofs;  // (3T, 2): first sorted slot, count of the edge group of triangle edge 3t + k
    const int* edge_tri;  // (3T): triangle of each sorted slot
    int B, V, T, H, W;
    int pos_batch;  // B (instance mode) or 1 (range mode: pos (V,4) shared by the images)
};

__device__ __forceinline__ int aa_pos_batch(const AaCtx& cx, int b) { return cx.pos_batch == 1 ? 0 : b; }

struct AaPair {
    int a_first;  // 1: the occluder's pixel a is the pair's first (left / top) pixel
    float s;      // crossing distance from a's centre, in pixels, [0, 1)
    int k;        // edge of the occluder: vertices k, (k + 1) % 3
    int t;        // occluder
};

__device__ __forceinline__ float vtx_pix(float c, float w, int N) { return ((c / w + 1.f) * (float)N) * 0.5f - 0.5f; }

__device__ bool aa_silhouette(const AaCtx& cx, int pb, int t, int k, float ot) {
    const int slot = 3 * t + k;
    const int first = cx.edge_ofs[2 * slot], cnt = cx.edge_ofs[2 * slot + 1];
    if (first < 0 || cnt < 1 || (long long)first + cnt > 3ll * cx.T) return false;  // malformed topology: no edge
    bool other = false;
    for (int j = first; j < first + cnt; ++j) {
        const int u = cx.edge_tri[j];
        if (u == t || (unsigned)u >= (unsigned)cx.T) continue;
        other = true;
        if (tri_orient(cx.pos, cx.tri, pb, u, cx.V) * ot < 0.f) return true;
    }
    return !other;
}

// the pair (first, second) of view b, first = the left (horiz) or upper pixel; false: the pair changes nothing
__device__ bool aa_pair(const AaCtx& cx, int b, int fx, int fy, bool horiz, AaPair& pr) {
    const int sx = fx + (horiz ? 1 : 0), sy = fy + (horiz ? 0 : 1);
    const int pb = aa_pos_batch(cx, b);
    const long long pf = ((long long)b * cx.H + fy) * cx.W + fx, ps = ((long long)b * cx.H + sy) * cx.W + sx;
    const float4 rf = reinterpret_cast<const float4*>(cx.rast)[pf];
    const float4 rs = reinterpret_cast<const float4*>(cx.rast)[ps];
    const int tf = pix_tri(rf.w, cx.T), ts = pix_tri(rs.w, cx.T);
    if (tf == ts) return false;
    // occluder: the smaller depth key (z/w, then id), an empty pixel's key is the largest (one 64-bit compare)
    const unsigned long long kf = tf < 0 ? ~0ull : ((unsigned long long)ordered_bits(rf.z) << 32) | (unsigned)tf;
    const unsigned long long ks = ts < 0 ? ~0ull : ((unsigned long long)ordered_bits(rs.z) << 32) | (unsigned)ts;
    const bool a_first = kf < ks;
    const int t = a_first ? tf : ts;
    int idx[3];
    if (!tri_indices(cx.tri, t, cx.V, idx)) return false;
    float4 v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = vtx(cx.pos, pb, cx.V, idx[q]);
    const float ot = tri_orient(cx.pos, cx.tri, pb, t, cx.V);
    // a's centre along the pair axis, the direction to b, and the perpendicular (scanline) coordinate
    const float al = horiz ? (float)(a_first ? fx : sx) : (float)(a_first ? fy : sy);
    const float dir = a_first ? 1.f : -1.f;
    const float q0 = horiz ? (float)fy : (float)fx;
    float best = 1.f;
    int bk = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 e0 = v[k], e1 = v[(k + 1) % 3];
        if (!(e0.w > 0.f) || !(e1.w > 0.f)) continue;
        const float l0 = horiz ? vtx_pix(e0.x, e0.w, cx.W) : vtx_pix(e0.y, e0.w, cx.H);
        const float l1 = horiz ? vtx_pix(e1.x, e1.w, cx.W) : vtx_pix(e1.y, e1.w, cx.H);
        const float p0 = horiz ? vtx_pix(e0.y, e0.w, cx.H) : vtx_pix(e0.x, e0.w, cx.W);
        const float p1 = horiz ? vtx_pix(e1.y, e1.w, cx.H) : vtx_pix(e1.x, e1.w, cx.W);
        if ((p0 > q0) == (p1 > q0)) continue;  // half-open in the perpendicular axis
        const float r = (q0 - p0) / (p1 - p0);
        const float lc = l0 + r * (l1 - l0);
        const float s = (lc - al) * dir;
        if (!(s >= 0.f && s < best)) continue;
        if (!aa_silhouette(cx, pb, t, k, ot)) continue;
        best = s;
        bk = k;
    }
    if (bk < 0) return false;
    pr.a_first = a_first ? 1 : 0;
    pr.s = best;
    pr.k = bk;
    pr.t = t;
    return true;
}

// the pairs of pixel (x, y) in a fixed order: left, right, up, down.  Returns the pair's first pixel and axis.
__device__ __forceinline__ bool aa_pair_of(int n, int x, int y, int W, int H, int& fx, int& fy, bool& horiz,
                                           bool& self_first) {
    switch (n) {
        case 0: fx = x - 1; fy = y; horiz = true; self_first = false; return x > 0;
        case 1: fx = x; fy = y; horiz = true; self_first = true; return x + 1 < W;
        case 2: fx = x; fy = y - 1; horiz = false; self_first = false; return y > 0;
        default: fx = x; fy = y; horiz = false; self_first = true; return y + 1 < H;
    }
}

__global__ __launch_bounds__(RS_BLOCK) void k_aa_fwd(AaCtx cx, const float* __restrict__ color, int C,
                                                     float* __restrict__ out) {
    const long long p = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= (long long)cx.B * cx.H * cx.W) return;
    const int b = (int)(p / ((long long)cx.H * cx.W));
    const int rem = (int)(p % ((long long)cx.H * cx.W));
    const int y = rem / cx.W, x = rem % cx.W;
    const float* cs = color + p * C;
    float* o = out + p * C;
    for (int c = 0; c < C; ++c) o[c] = cs[c];
    for (int n = 0; n < 4; ++n) {
        int fx, fy;
        bool horiz, self_first;
        if (!aa_pair_of(n, x, y, cx.W, cx.H, fx, fy, horiz, self_first)) continue;
        AaPair pr;
        if (!aa_pair(cx, b, fx, fy, horiz, pr)) continue;
        const bool m_first = pr.a_first ? (pr.s < 0.5f) : !(pr.s < 0.5f);  // the pixel the pair changes
        if (m_first != self_first) continue;
        const float alpha = pr.s < 0.5f ? 0.5f - pr.s : pr.s - 0.5f;
        const long long po = self_first ? p + (horiz ? 1 : cx.W) : p - (horiz ? 1 : cx.W);
        const float* co = color + po * C;
        for (int c = 0; c < C; ++c) o[c] += alpha * (co[c] - cs[c]);
    }
}

__global__ __launch_bounds__(RS_BLOCK) void k_aa_bwd(AaCtx cx, const float* __restrict__ color, int C,
                                                     const float* __restrict__ grad_out,
                                                     float* __restrict__ grad_color, float* __restrict__ grad_pos) {
    const long long p = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= (long long)cx.B * cx.H * cx.W) return;
    const int b = (int)(p / ((long long)cx.H * cx.W));
    const int rem = (int)(p % ((long long)cx.H * cx.W));
    const int y = rem / cx.W, x = rem % cx.W;
    const int pb = aa_pos_batch(cx, b);
    const float* gs = grad_out + p * C;
    float* gc = grad_color + p * C;
    for (int c = 0; c < C; ++c) gc[c] = gs[c];
    for (int n = 0; n < 4; ++n) {
        int fx, fy;
        bool horiz, self_first;
        if (!aa_pair_of(n, x, y, cx.W, cx.H, fx, fy, horiz, self_first)) continue;
        AaPair pr;
        if (!aa_pair(cx, b, fx, fy, horiz, pr)) continue;
        const bool m_first = pr.a_first ? (pr.s < 0.5f) : !(pr.s < 0.5f);
        const float alpha = pr.s < 0.5f ? 0.5f - pr.s : pr.s - 0.5f;
        const long long po = self_first ? p + (horiz ? 1 : cx.W) : p - (horiz ? 1 : cx.W);
        if (m_first != self_first) {  // the other pixel m is changed by alpha (c_self - c_m)
            const float* gm = grad_out + po * C;
            for (int c = 0; c < C; ++c) gc[c] += alpha * gm[c];
            continue;
        }
        // this pixel is m: out[m] += alpha (c_o - c_m)
        for (int c = 0; c < C; ++c) gc[c] -= alpha * gs[c];
        if (!grad_pos) continue;
        // d out[m] / d s = c_a - c_b
        const bool self_is_a = pr.a_first ? self_first : !self_first;
        const float* ca = color + (self_is_a ? p : po) * C;
        const float* cb = color + (self_is_a ? po : p) * C;
        float gsum = 0.f;
        for (int c = 0; c < C; ++c) gsum += gs[c] * (ca[c] - cb[c]);
        if (gsum == 0.f) continue;
        // s = (l0 + r (l1 - l0) - al) dir, r = (q0 - p0) / (p1 - p0); l / p pixel coordinates of the edge ends
        int idx[3];
        tri_indices(cx.tri, pr.t, cx.V, idx);  // valid: aa_pair checked it
        const int i0 = idx[pr.k], i1 = idx[(pr.k + 1) % 3];
        const float4 e0 = vtx(cx.pos, pb, cx.V, i0), e1 = vtx(cx.pos, pb, cx.V, i1);
        const int Nl = horiz ? cx.W : cx.H, Np = horiz ? cx.H : cx.W;
        const float cl0 = horiz ? e0.x : e0.y, cl1 = horiz ? e1.x : e1.y;
        const float cp0 = horiz ? e0.y : e0.x, cp1 = horiz ? e1.y : e1.x;
        const float l0 = vtx_pix(cl0, e0.w, Nl), l1 = vtx_pix(cl1, e1.w, Nl);
        const float p0 = vtx_pix(cp0, e0.w, Np), p1 = vtx_pix(cp1, e1.w, Np);
        const float q0 = horiz ? (float)fy : (float)fx;
        const float dp = p1 - p0, r = (q0 - p0) / dp, dl = l1 - l0;
        const float dir = pr.a_first ? 1.f : -1.f;
        const float g = gsum * dir;
        const float g_l0 = g * (1.f - r), g_l1 = g * r;
        const float g_p0 = g * dl * (r - 1.f) / dp, g_p1 = -g * dl * r / dp;
        // pixel coordinate c -> ((c / w + 1) N) / 2 - 1/2:  d/dc = N / (2 w),  d/dw = -c N / (2 w^2)
        const float hl = 0.5f * (float)Nl, hp = 0.5f * (float)Np;
        const float gcl0 = g_l0 * hl / e0.w, gcl1 = g_l1 * hl / e1.w;
        const float gcp0 = g_p0 * hp / e0.w, gcp1 = g_p1 * hp / e1.w;
        const float gw0 = -(gcl0 * cl0 + gcp0 * cp0) / e0.w, gw1 = -(gcl1 * cl1 + gcp1 * cp1) / e1.w;
        float* gp0 = grad_pos + ((long long)pb * cx.V + i0) * 4;
        float* gp1 = grad_pos + ((long long)pb * cx.V + i1) * 4;
        atomicAdd(gp0 + (horiz ? 0 : 1), gcl0);
        atomicAdd(gp0 + (horiz ? 1 : 0), gcp0);
        atomicAdd(gp0 + 3, gw0);
        atomicAdd(gp1 + (horiz ? 0 : 1), gcl1);
        atomicAdd(gp1 + (horiz ? 1 : 0), gcp1);
        atomicAdd(gp1 + 3, gw1);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI

static bool rs_dims_ok(int B, int V, int T, int H, int W) {
    return B >= 1 && V >= 0 && T >= 0 && T < TT_RAST_MAX_TRIS && H >= 1 && W >= 1 &&
           (long long)B * H * W < (1ll << 40);
}

static unsigned rs_blocks(long long n) { return (unsigned)((n + RS_BLOCK - 1) / RS_BLOCK); }

extern "C" int64_t tt_rast_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t W) {
    if (!rs_dims_ok(B, 0, T, H, W)) return TT_ERR_BAD_ARG;
    return rast_layout(nullptr, B, (long long)B * T, H, W, false).bytes;
}

// the launches of both modes behind the layout; range mode (l.prefix) first scans the images' counts
static int rast_fwd_launch(const float* pos, const int* tri, const int* ranges, const RastLayout& l, int B, int V, int T,
                           int H, int W, float* rast, hipStream_t st) {
    const long long npix = (long long)B * H * W;
    if (l.n == 0 || V == 0) {
        if (hipMemsetAsync(rast, 0, (size_t)npix * 16, st) != hipSuccess) return TT_ERR_LAUNCH;
        return tt_check_launch();
    }
    if (hipMemsetAsync(l.keys, 0xff, (size_t)npix * 8, st) != hipSuccess) return TT_ERR_LAUNCH;
    if (l.prefix) {
        hipLaunchKernelGGL(k_rast_range_counts, dim3(rs_blocks(B)), dim3(RS_BLOCK), 0, st, ranges, B, l.prefix);
        tt_exclusive_scan<long long>(l.prefix, B, l.prefix, l.psum, l.prefix + B, st);
    }
    const RastSlots m{l.prefix, ranges, B, T};
    hipLaunchKernelGGL(k_rast_setup, dim3(rs_blocks(l.n)), dim3(RS_BLOCK), 0, st, pos, tri, m, l.n, V, H, W, l.bbox,
                       l.offs);
    // the counts were written into offs[]: scanned in place, the total behind them
    tt_exclusive_scan<long long>(l.offs, l.n, l.offs, l.bsum, l.offs + l.n, st);
    int cus = tt_num_cus();
    if (cus <= 0) cus = 256;
    hipLaunchKernelGGL(k_rast_cover, dim3((unsigned)cus * 8), dim3(RS_BLOCK), 0, st, pos, tri, m, V, H, W, l.bbox,
                       l.offs, l.n, l.keys);
    hipLaunchKernelGGL(k_rast_resolve, dim3(rs_blocks(npix)), dim3(RS_BLOCK), 0, st, pos, l.prefix ? 1 : B, tri, B, V,
                       T, H, W, l.keys, rast);
    return tt_check_launch();
}

extern "C" int tt_rast_fwd(const float* pos, const int32_t* tri, int32_t B, int32_t V, int32_t T, int32_t H,
                           int32_t W, void* workspace, float* rast, void* stream) {
    if (!rs_dims_ok(B, V, T, H, W) || !workspace || !rast || (V > 0 && !pos) || (T > 0 && !tri))
        return TT_ERR_BAD_ARG;
    return rast_fwd_launch(pos, (const int*)tri, nullptr, rast_layout(workspace, B, (long long)B * T, H, W, false), B,
                           V, T, H, W, rast, (hipStream_t)stream);
}

// the slots of B ranges (first, count) over T triangles, read on the host; -1: a range leaves [0, T]
static long long range_slots(const int32_t* ranges_host, int B, int T) {
    long long n = 0;
    for (int b = 0; b < B; ++b) {
        const long long first = ranges_host[2 * b], count = ranges_host[2 * b + 1];
        if (first < 0 || count < 0 || first + count > T) return -1;
        n += count;
    }
    return n;
}

extern "C" int64_t tt_rast_range_workspace_bytes(int32_t B, int64_t n_slots, int32_t H, int32_t W) {
    if (!rs_dims_ok(B, 0, 0, H, W) || n_slots < 0 || n_slots >= (1ll << 40)) return TT_ERR_BAD_ARG;
    return rast_layout(nullptr, B, n_slots, H, W, true).bytes;
}

extern "C" int tt_rast_range_fwd(const float* pos, const int32_t* tri, const int32_t* ranges_dev,
                                 const int32_t* ranges_host, int32_t B, int32_t V, int32_t T, int32_t H, int32_t W,
                                 void* workspace, float* rast, void* stream) {
    if (!rs_dims_ok(B, V, T, H, W) || !workspace || !rast || !ranges_dev || !ranges_host || (V > 0 && !pos) ||
        (T > 0 && !tri))
        return TT_ERR_BAD_ARG;
    const long long n = range_slots(ranges_host, B, T);
    if (n < 0 || n >= (1ll << 40)) return TT_ERR_BAD_ARG;
    return rast_fwd_launch(pos, (const int*)tri, (const int*)ranges_dev, rast_layout(workspace, B, n, H, W, true), B,
                           V, T, H, W, rast, (hipStream_t)stream);
}

static int rast_bwd_launch(const float* pos, int pos_batch, const int32_t* tri, const float* rast,
                           const float* grad_rast, int B, int V, int T, int H, int W, float* grad_pos, void* stream) {
    if (!rs_dims_ok(B, V, T, H, W) || !rast || !grad_rast || (V > 0 && (!pos || !grad_pos)) || (T > 0 && !tri))
        return TT_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) return TT_OK;
    if (hipMemsetAsync(grad_pos, 0, (size_t)pos_batch * V * 16, st) != hipSuccess) return TT_ERR_LAUNCH;
    if (T == 0) return tt_check_launch();
    hipLaunchKernelGGL(k_rast_bwd, dim3(rs_blocks((long long)B * H * W)), dim3(RS_BLOCK), 0, st, pos, pos_batch,
                       (const int*)tri, rast, grad_rast, B, V, T, H, W, grad_pos);
    return tt_check_launch();
}

extern "C" int tt_rast_bwd(const float* pos, const int32_t* tri, const float* rast, const float* grad_rast, int32_t B,
                           int32_t V, int32_t T, int32_t H, int32_t W, float* grad_pos, void* stream) {
    return rast_bwd_launch(pos, B, tri, rast, grad_rast, B, V, T, H, W, grad_pos, stream);
}

extern "C" int tt_rast_range_bwd(const float* pos, const int32_t* tri, const float* rast, const float* grad_rast,
                                 int32_t B, int32_t V, int32_t T, int32_t H, int32_t W, float* grad_pos,
                                 void* stream) {
    return rast_bwd_launch(pos, 1, tri, rast, grad_rast, B, V, T, H, W, grad_pos, stream);
}

extern "C" int tt_interp_fwd(const float* attr, int32_t attr_batch, const float* rast, const int32_t* tri, int32_t B,
                             int32_t V, int32_t T, int32_t H, int32_t W, int32_t C, float* out, void* stream) {
    if (!rs_dims_ok(B, V, T, H, W) || C < 1 || !rast || !out || (V > 0 && !attr) || (T > 0 && !tri) ||
        (attr_batch != 1 && attr_batch != B))
        return TT_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_interp_fwd, dim3(rs_blocks((long long)B * H * W)), dim3(RS_BLOCK), 0, (hipStream_t)stream,
                       attr, attr_batch, rast, (const int*)tri, B, V, T, H, W, C, out);
    return tt_check_launch();
}

extern "C" int tt_interp_bwd(const float* attr, int32_t attr_batch, const float* rast, const int32_t* tri,
                             const float* grad_out, int32_t B, int32_t V, int32_t T, int32_t H, int32_t W, int32_t C,
                             float* grad_attr, float* grad_rast, void* stream) {
    if (!rs_dims_ok(B, V, T, H, W) || C < 1 || !rast || !grad_out || (V > 0 && !attr) || (T > 0 && !tri) ||
        (attr_batch != 1 && attr_batch != B) || (!grad_attr && !grad_rast))
        return TT_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (grad_attr && V > 0 &&
        hipMemsetAsync(grad_attr, 0, (size_t)attr_batch * V * C * 4, st) != hipSuccess)
        return TT_ERR_LAUNCH;
    hipLaunchKernelGGL(k_interp_bwd, dim3(rs_blocks((long long)B * H * W)), dim3(RS_BLOCK), 0, st, attr, attr_batch,
                       rast, (const int*)tri, grad_out, B, V, T, H, W, C, V > 0 ? grad_attr : nullptr, grad_rast);
    return tt_check_launch();
}

static bool aa_args_ok(const float* color, const float* rast, const float* pos, const int32_t* tri,
                       const int32_t* edge_ofs, const int32_t* edge_tri, int B, int V, int T, int H, int W, int C) {
    return rs_dims_ok(B, V, T, H, W) && C >= 1 && color && rast && (V > 0 || T == 0) && (V == 0 || pos) &&
           (T == 0 || (tri && edge_ofs && edge_tri));
}

static int aa_fwd_launch(const float* color, const float* rast, const float* pos, int pos_batch, const int32_t* tri,
                         const int32_t* edge_ofs, const int32_t* edge_tri, int B, int V, int T, int H, int W, int C,
                         float* out, void* stream) {
    if (!aa_args_ok(color, rast, pos, tri, edge_ofs, edge_tri, B, V, T, H, W, C) || !out) return TT_ERR_BAD_ARG;
    const AaCtx cx{rast, pos, (const int*)tri, (const int*)edge_ofs, (const int*)edge_tri, B, V, T, H, W, pos_batch};
    hipLaunchKernelGGL(k_aa_fwd, dim3(rs_blocks((long long)B * H * W)), dim3(RS_BLOCK), 0, (hipStream_t)stream, cx,
                       color, C, out);
    return tt_check_launch();
}

static int aa_bwd_launch(const float* color, const float* rast, const float* pos, int pos_batch, const int32_t* tri,
                         const int32_t* edge_ofs, const int32_t* edge_tri, const float* grad_out, int B, int V, int T,
                         int H, int W, int C, float* grad_color, float* grad_pos, void* stream) {
    if (!aa_args_ok(color, rast, pos, tri, edge_ofs, edge_tri, B, V, T, H, W, C) || !grad_out || !grad_color)
        return TT_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (grad_pos && V > 0 && hipMemsetAsync(grad_pos, 0, (size_t)pos_batch * V * 16, st) != hipSuccess)
        return TT_ERR_LAUNCH;
    const AaCtx cx{rast, pos, (const int*)tri, (const int*)edge_ofs, (const int*)edge_tri, B, V, T, H, W, pos_batch};
    hipLaunchKernelGGL(k_aa_bwd, dim3(rs_blocks((long long)B * H * W)), dim3(RS_BLOCK), 0, st, cx, color, C, grad_out,
                       grad_color, V > 0 ? grad_pos : nullptr);
    return tt_check_launch();
}

extern "C" int tt_aa_fwd(const float* color, const float* rast, const float* pos, const int32_t* tri,
                         const int32_t* edge_ofs, const int32_t* edge_tri, int32_t B, int32_t V, int32_t T, int32_t H,
                         int32_t W, int32_t C, float* out, void* stream) {
    return aa_fwd_launch(color, rast, pos, B, tri, edge_ofs, edge_tri, B, V, T, H, W, C, out, stream);
}

extern "C" int tt_aa_range_fwd(const float* color, const float* rast, const float* pos, const int32_t* tri,
                               const int32_t* edge_ofs, const int32_t* edge_tri, int32_t B, int32_t V, int32_t T,
                               int32_t H, int32_t W, int32_t C, float* out, void* stream) {
    return aa_fwd_launch(color, rast, pos, 1, tri, edge_ofs, edge_tri, B, V, T, H, W, C, out, stream);
}

extern "C" int tt_aa_bwd(const float* color, const float* rast, const float* pos, const int32_t* tri,
                         const int32_t* edge_ofs, const int32_t* edge_tri, const float* grad_out, int32_t B,
                         int32_t V, int32_t T, int32_t H, int32_t W, int32_t C, float* grad_color, float* grad_pos,
                         void* stream) {
    return aa_bwd_launch(color, rast, pos, B, tri, edge_ofs, edge_tri, grad_out, B, V, T, H, W, C, grad_color,
                         grad_pos, stream);
}

extern "C" int tt_aa_range_bwd(const float* color, const float* rast, const float* pos, const int32_t* tri,
                               const int32_t* edge_ofs, const int32_t* edge_tri, const float* grad_out, int32_t B,
                               int32_t V, int32_t T, int32_t H, int32_t W, int32_t C, float* grad_color,
                               float* grad_pos, void* stream) {
    return aa_bwd_launch(color, rast, pos, 1, tri, edge_ofs, edge_tri, grad_out, B, V, T, H, W, C, grad_color,
                         grad_pos, stream);
}
