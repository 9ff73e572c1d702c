// tt_launch.h -- host side of the decode family (tt_forward.hip, tt_backward.hip, tt_backward_tex.hip, tt_points.hip):
// what every entry point does between validating its arguments and launching its kernel.  The precision dispatch, the
// grid of the queue-driven kernels and the per-point validator are plain host C++ in tt_host.h.
#pragma once
#include <stdlib.h>

#include "tt_device.h"
#include "tt_host.h"

struct MlpGradPtrs {
    float* w1;
    float* w2;
    float* w3;
    float* v1;
    float* v2;
    float* v3;
};

static inline MlpPtrs to_ptrs(const tt_mlp_weights* w) {
    MlpPtrs m;
    m.w1 = w->w1;
    m.w2 = w->w2;
    m.w3 = w->w3;
    m.v1 = w->v1;
    m.v2 = w->v2;
    m.v3 = w->v3;
    return m;
}
static inline MlpGradPtrs to_gptrs(const tt_mlp_grads* g) {
    MlpGradPtrs m;
    m.w1 = g->w1;
    m.w2 = g->w2;
    m.w3 = g->w3;
    m.v1 = g->v1;
    m.v2 = g->v2;
    m.v3 = g->v3;
    return m;
}

static inline int debug_flags() {
#ifdef TT_TUNING
    const char* e = getenv("TT_DEBUG_FLAGS");  // profiling ablations, tuning build only
    return e ? (int)strtol(e, nullptr, 0) : 0;
#else
    return 0;
#endif
}

// The parameter structs of the ray kernels (DecodeRaysParams, RenderEvalParams, BwdGeoParams, BwdTexParams) open with the
// same seven fields; the per-point backward entries launch the same kernels with "rays" of one sample whose origin is the
// point (rays_d, t_starts, t_ends null => x = o exactly).
template <class P>
static inline void tt_fill_rays(P& p, const float* packed, const tt_mlp_weights* w, const float* rays_o,
                                const float* rays_d, const float* t_starts, const float* t_ends,
                                const tt_render_cfg& cfg) {
    p.packed = packed;
    p.w = to_ptrs(w);
    p.rays_o = rays_o;
    p.rays_d = rays_d;
    p.t_starts = t_starts;
    p.t_ends = t_ends;
    p.cfg = cfg;
}

// ... and those of the per-point kernels (QueryParams, QueryFieldParams, PointsBwdXParams) with these nine.
template <class P>
static inline void tt_fill_points(P& p, const float* packed, const tt_mlp_weights* w, const float* points,
                                  int32_t n_batch, int64_t n_points, int32_t views_per_prompt, int32_t plane_h,
                                  int32_t plane_w, float radius) {
    p.packed = packed;
    p.w = to_ptrs(w);
    p.points = points;
    p.n_batch = n_batch;
    p.n_points = n_points;
    p.views_per_prompt = views_per_prompt;
    p.H = plane_h;
    p.W = plane_w;
    p.radius = radius;
}

// Grid of a per-point kernel: its waves stride over the tiles of TT_TILE points, so no more workgroups than the tiles
// fill and at most `max_blocks` (what fits the device at the kernel's occupancy).
static inline dim3 tt_point_blocks(int64_t n_points, int32_t n_batch, int waves_per_block, long long max_blocks) {
    const long long n_tiles = ((n_points + TT_TILE - 1) / TT_TILE) * n_batch;
    const long long blocks = (n_tiles + waves_per_block - 1) / waves_per_block;
    return dim3((unsigned)(blocks < max_blocks ? blocks : max_blocks));
}

// Plans a queue-driven launch: the tile geometry and the item count (tt_make_geom, block-major queues), the limit of
// 2^30 items the 32-bit queue heads can deal (TT_ERR_UNSUPPORTED) and a zeroed queue slot on `stream` (TT_ERR_DEVICE if
// there is none).  The kernel must be the next launch on that stream.
static inline int tt_plan_queue(const tt_render_cfg* cfg, long long wave_slots, hipStream_t stream, TileGeom* geom,
                                long long* n_items, int** queue, int steps_per_item = 6, int min_items_per_slot = 8) {
    *n_items = tt_make_geom(cfg, wave_slots, geom, 1, steps_per_item, min_items_per_slot);
    if (*n_items > (1LL << 30)) return TT_ERR_UNSUPPORTED;
    *queue = tt_queue_counters(stream);
    return *queue ? TT_OK : TT_ERR_DEVICE;
}
