/*
 * rt_denoise.h — the argument block of the denoise kernels (rt_denoise_kernel.h).  Written by rt_denoise_capi.cpp, read by the kernels.
 */
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <stdint.h>

#include "rt_amd.h"
#include "rt_device_scene.h"

typedef struct {
    int32_t width, height;
    /* the caller's planes (rt_render's row-major layout): read by the pack pass; albedo also by the last level.  object, albedo may be NULL */
    const float *colour, *normal, *depth;
    const int32_t *object;
    const float *albedo;
    float albedo_floor;
    /* the context's records, one per pixel: guide {N.x, N.y, N.z, Z}, written once; colour {F.r, F.g, F.b, object bits}, level i reads
     * `src` and writes `dst` (the last level writes interleaved RGB to `out` instead) */
    rt_f4 *guide;
    const rt_f4 *src;
    rt_f4 *dst;
    float *out;
    /* one level: the step s, 1 / s, 1 / sc^2 for this level's sc, sigma_depth, how often the normal weight is squared */
    int32_t step;
    float inv_step, kc, sigma_depth;
    int32_t normal_power_log2;
} rt_denoise_args;

#endif
