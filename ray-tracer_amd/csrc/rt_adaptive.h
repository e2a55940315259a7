/*
 * rt_adaptive.h — what the adaptive-sampling entry points (rt_adaptive_capi.cpp) share with their kernels (rt_adaptive_kernel.h) and with
 * the host-only sanitizer program (tests/sanitize/adaptive_host_fuzz.cpp): the plan kernel's argument block, the parameter checks and the
 * pass's tile list.  Plain functions of vectors and scalars; no HIP.  include/rt_amd.h has the definitions.
 */
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include <stdint.h>

#include "rt_amd.h"

/* one plan launch: A, B (W*H*3) and count (W*H) in, budget (W*H) and the two per-tile planes out */
typedef struct {
    const float *a, *b;
    const uint32_t *count;
    uint16_t *budget;
    float *tile_error;
    uint32_t *tile_active;
    int32_t width, height, tiles_x, num_tiles;
    float threshold, pixel_threshold, floor;
    uint32_t step_spp, max_spp;
} rt_plan_args;

#ifdef __cplusplus
#include <algorithm>
#include <cmath>
#include <vector>

namespace rt_adaptive {

/* what is wrong with the parameters (nullptr: nothing); the ranges are include/rt_amd.h's */
inline const char *params_error(const rt_adaptive_params &p)
{
    if (p.pilot_spp < 1 || p.pilot_spp > RT_BUDGET_MAX) return "bad adaptive parameters: pilot_spp (1 .. 65535)";
    if (p.step_spp < 1 || p.step_spp > RT_BUDGET_MAX) return "bad adaptive parameters: step_spp (1 .. 65535)";
    if (p.max_spp < p.pilot_spp || p.max_spp > RT_ADAPTIVE_MAX_SPP) return "bad adaptive parameters: max_spp (pilot_spp .. 2^24)";
    if (p.max_passes < 0 || p.max_passes > RT_ADAPTIVE_MAX_PASSES) return "bad adaptive parameters: max_passes (0 .. 64)";
    if (!(p.threshold > 0.0f) || std::isinf(p.threshold)) return "bad adaptive parameters: threshold must be positive and finite";
    if (!(p.pixel_threshold > 0.0f)) return "bad adaptive parameters: pixel_threshold must be positive (+inf: that rule is off)";
    if (!(p.floor > 0.0f) || std::isinf(p.floor)) return "bad adaptive parameters: floor must be positive and finite";
    if (p.reserved[0]) return "bad adaptive parameters: reserved fields must be 0";
    return nullptr;
}

/* The tile list of a pass from the plan's per-tile planes: the tiles with an active pixel, by decreasing error (the longest jobs first: a
 * tile's error is what keeps it sampling), ties by the lower index.  A NaN error cannot be ordered: it counts as the largest (the plan
 * kernel does not produce one - a NaN pixel's e is 0 - but the planes are the caller's in rt_adaptive_plan_device). */
inline void build_tile_list(const float *tile_error, const uint32_t *tile_active, int32_t num_tiles, std::vector<uint32_t> &list)
{
    list.clear();
    for (int32_t t = 0; t < num_tiles; t++)
        if (tile_active[t]) list.push_back((uint32_t)t);
    auto before = [&](uint32_t x, uint32_t y) {
        const float ex = tile_error[x], ey = tile_error[y];
        const bool nx = ex != ex, ny = ey != ey;
        if (nx != ny) return nx;
        if (!nx && ex != ey) return ex > ey;
        return x < y;
    };
    std::sort(list.begin(), list.end(), before);
}

}  // namespace rt_adaptive
#endif

#endif
