// tt_host.h -- host-side helpers shared by the translation units of libtt_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/tt_abi.h"

int tt_check_launch();
int tt_num_cus();
int tt_validate_cfg(const tt_render_cfg* cfg);
bool tt_planes_too_large(long long n_prompts, int plane_h, int plane_w);  // packed planes >= 4 GB: unsupported

// Precision mode of the matrix products (tt_mfma16.h, "precision switch").  A launch takes its mode from its flag bits
// (tt_abi.h): no precision bit = PREC_S3 (the default), *_SPLIT2 = PREC_S2 (fast), *_EXACT_F32 = PREC_F32.  More than one
// precision bit is rejected by tt_validate_cfg / tt_qflags_ok.
enum { PREC_S2 = 0, PREC_F32 = 1, PREC_S3 = 2 };
static inline int tt_prec_of_r(int flags) {
    return (flags & TT_R_EXACT_F32) ? PREC_F32 : ((flags & TT_R_SPLIT2) ? PREC_S2 : PREC_S3);
}
static inline int tt_prec_of_q(int flags) {
    return (flags & TT_Q_EXACT_F32) ? PREC_F32 : ((flags & TT_Q_SPLIT2) ? PREC_S2 : PREC_S3);
}
static inline bool tt_qflags_ok(int flags) {
    const int pbits = flags & (TT_Q_EXACT_F32 | TT_Q_SPLIT2 | TT_Q_SPLIT3);
    return (pbits & (pbits - 1)) == 0;
}

// The one place a runtime precision mode becomes a template argument: calls f(std::integral_constant<int, PREC_*>{}).
// Every kernel launch that is templated on the mode goes through here, so each instantiates its three modes and no other.
template <class F>
static inline void tt_dispatch_prec(int prec, F&& f) {
    if (prec == PREC_F32)
        f(std::integral_constant<int, PREC_F32>{});
    else if (prec == PREC_S3)
        f(std::integral_constant<int, PREC_S3>{});
    else
        f(std::integral_constant<int, PREC_S2>{});
}
// ... and, for the kernels that also compile the normal / texture outputs in or out, the two switches as
// std::bool_constant: f(prec, need_n, need_t).
template <class F>
static inline void tt_dispatch(int prec, bool need_n, bool need_t, F&& f) {
    if (need_n && need_t)
        tt_dispatch_prec(prec, [&](auto P) { f(P, std::true_type{}, std::true_type{}); });
    else if (need_n)
        tt_dispatch_prec(prec, [&](auto P) { f(P, std::true_type{}, std::false_type{}); });
    else if (need_t)
        tt_dispatch_prec(prec, [&](auto P) { f(P, std::false_type{}, std::true_type{}); });
    else
        tt_dispatch_prec(prec, [&](auto P) { f(P, std::false_type{}, std::false_type{}); });
}

// Grid of a persistent, queue-driven kernel: one workgroup of `waves_per_block` waves per CU, no more than the items
// need (a wave takes an item at a time), rounded up to a multiple of 8 (the XCDs deal workgroups round-robin).
static inline long long tt_persistent_blocks(long long n_items, int cus, int waves_per_block) {
    long long blocks = cus;
    const long long need = (n_items + waves_per_block - 1) / waves_per_block;
    if (blocks > need) blocks = need;
    return (blocks + 7) / 8 * 8;
}

// Arguments every per-point entry point takes.  The counts, the batch split and the flag word come first everywhere
// (points_cfg, tt_backward_common.h, goes on to tt_validate_cfg with them); tt_query_points, tt_query_field and
// tt_points_bwd_x need only the radius and square planes besides.
static inline bool tt_points_counts_ok(int32_t n_batch, int64_t n_points, int32_t n_prompts, int32_t views_per_prompt,
                                       int32_t q_flags) {
    return n_batch > 0 && n_points > 0 && n_prompts > 0 && views_per_prompt > 0 &&
           (int64_t)n_prompts * views_per_prompt == n_batch && tt_qflags_ok(q_flags);
}
static inline int tt_validate_points(int32_t n_batch, int64_t n_points, int32_t n_prompts, int32_t views_per_prompt,
                                     int32_t plane_h, int32_t plane_w, float radius, int32_t q_flags) {
    if (!tt_points_counts_ok(n_batch, n_points, n_prompts, views_per_prompt, q_flags) || !(radius > 0.f))
        return TT_ERR_BAD_ARG;
    if (plane_h != plane_w || plane_h <= 0) return TT_ERR_UNSUPPORTED;
    return TT_OK;
}

// The mesh-stage kernels take one item per thread in blocks of TT_ITEM_BLOCK threads: the grid for n items
#define TT_ITEM_BLOCK 256
static inline unsigned tt_grid(long long n) { return (unsigned)((n + TT_ITEM_BLOCK - 1) / TT_ITEM_BLOCK); }

// Carves the sections of one workspace allocation: every section starts 256-byte aligned, in the order of the take()
// calls.  With a null base take() returns null and only bytes() means something (the tt_*_workspace_bytes queries run
// the same function as the launches, so a section cannot be sized in one place and placed in another).
struct TtCarver {
    char* base;
    long long off = 0;
    template <typename T>
    T* take(long long count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += ((long long)sizeof(T) * count + 255) & ~255ll;
        return p;
    }
    long long bytes() const { return off; }
};

// the leading part of the tt_mesh_workspace_bytes layout that tt_mesh_components touches, for T faces (tt_mesh.hip);
// tt_uv.hip nests such a workspace inside its own
long long tt_mesh_components_bytes(long long T);

struct TileGeom;
// fills the tile geometry / chunking for a render config; returns the number of work items.
// default_order: order of an XCD's item queue, 0 = chunk-major, 1 = block-major (measured slightly faster in all
// three kernels once the queue is dynamic: concurrent waves of an XCD then walk ONE pixel block's depth chunks and
// its neighbours rather than one depth slab of the whole image share).
long long tt_make_geom(const tt_render_cfg* cfg, long long wave_slots, TileGeom* g, int default_order,
                       int steps_per_item = 6, int min_items_per_slot = 8);

// Work-queue counters for one kernel launch: 8 int32 heads (one per XCD) in a library-owned device scratch, zeroed on
// `stream` by a one-wave kernel enqueued here (so the caller must launch the kernel on the same stream, next).  A
// ring of slots per (device, stream) for eager launches, a round-robin pool for launches recorded under stream capture
// (see tt_host.cpp).  Returns nullptr on a HIP error.  (The only state the library keeps: a 328 KB allocation per
// device, never freed; its first use must not happen inside a stream capture.)
int* tt_queue_counters(hipStream_t stream);
// layout of a slot (ints): [0..8] queue heads; [TT_SLOT_BOUNDS + k] = bit pattern of a non-negative float, raised with
// atomicMax by the reduction kernels launched in front of a backward kernel (tt_backward.hip: magnitude bounds of the
// operands of the split-fp16 weight-gradient outer products); everything is zeroed together with the queue heads.
#define TT_SLOT_INTS 32
#define TT_SLOT_BOUNDS 16
#define TT_BOUND_PLANES 0   /* max |texel| of the three planes the kernel reads */
#define TT_BOUND_UP0 1      /* geometry: max |d/d sdf|;            texture: max |g_rgb| */
#define TT_BOUND_UP1 2      /* geometry: max |d/d sdf_grad| comp.; texture: max |g_features| */
#define TT_SLOT_EIKONAL 24  /* tt_eikonal_fwd: 4 ints (8-byte aligned): fixed-point sum, overflow float, arrival counter */

// the ray march in front of / behind the decode kernels (tt_march.hip)
int tt_launch_march_fwd(const float* rays_d, const float* t_starts, const float* t_ends, const tt_render_cfg* cfg,
                        const float* sdf, const float* sdf_grad, const float* features, float* opacity, float* depth,
                        float* rgb_fg, float* z_variance, float* normal_acc, float* weights, float* trans,
                        hipStream_t stream);
int tt_launch_march_bwd(const float* rays_d, const float* t_starts, const float* t_ends, const tt_render_cfg* cfg,
                        const float* sdf, const float* sdf_grad, const float* features, const float* trans,
                        const float* opacity, const float* depth, const float* g_opacity, const float* g_depth,
                        const float* g_rgb_fg, const float* g_z_variance, const float* g_normal_acc,
                        const float* g_weights, const float* g_sdf, const float* g_sdf_grad, float* g_inv_std_rays,
                        float* ws, hipStream_t stream);
