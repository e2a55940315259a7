/*
 * rt_adaptive_kernel.h — the image-space kernels of the adaptive sampling loop (include/rt_amd.h has the definitions; the operation order
 * below IS the interface: tests/adaptive_ref.py reproduces it bit for bit).  Nothing here traverses a scene.
 *   plan      one wave per 8x8 tile, one lane per pixel (lane = row in tile * 8 + column): the pixel's error estimate from the two
 *             half buffers, the tile's mean by an xor butterfly over the wave (a fixed pairwise tree), the pixel's next budget.
 *   combine   one lane per pixel: frame = (A + B) * 0.5f (a NaN as the canonical quiet NaN), count = 2 * count.
 * The launchers at the end are declared in rt_launch.h.  No LDS, no atomics.
 */
#ifndef RT_ADAPTIVE_KERNEL_H
#define RT_ADAPTIVE_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_adaptive.h"
#include "rt_launch.h"
#include "rt_math.h"

#define RT_PLAN_WAVES 4              /* tiles per workgroup */

__global__ __launch_bounds__(64 * RT_PLAN_WAVES) void rt_adaptive_plan_kernel(const rt_plan_args a)
{
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * RT_PLAN_WAVES + (threadIdx.x >> 6);
    if (tile >= a.num_tiles) return;                                    /* (the whole wave) */
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
    const bool inside = px < a.width && py < a.height;
    const size_t pixel = (size_t)py * (size_t)a.width + (size_t)px;
    float e = 0.0f;                                                     /* a slot outside the image counts as 0 */
    uint32_t count = 0u;
    if (inside) {
        const float ar = a.a[3 * pixel], ag = a.a[3 * pixel + 1], ab = a.a[3 * pixel + 2];
        const float br = a.b[3 * pixel], bg = a.b[3 * pixel + 1], bb = a.b[3 * pixel + 2];
        const float ir = (ar + br) * 0.5f, ig = (ag + bg) * 0.5f, ib = (ab + bb) * 0.5f;
        const float num = (fabsf(ar - br) + fabsf(ag - bg)) + fabsf(ab - bb);
        const float s = (ir + ig) + ib;
        e = num / sqrtf(s > a.floor ? s : a.floor);
        if (e != e) e = 0.0f;
        count = a.count[pixel];
    }
    float v = e;
    for (int k = 1; k < 64; k <<= 1) v = v + __shfl_xor(v, k, 64);      /* every lane ends with the same bits: x + y == y + x */
    const int in_x = a.width - tx * 8 < 8 ? a.width - tx * 8 : 8, in_y = a.height - ty * 8 < 8 ? a.height - ty * 8 : 8;
    const float E = v / (float)(in_x * in_y);
    const bool active = inside && count < a.max_spp && (E > a.threshold || e > a.pixel_threshold);
    const unsigned long long m_active = __ballot(active);
    if (inside) {
        const uint32_t left = a.max_spp - count;
        a.budget[pixel] = (uint16_t)(active ? (a.step_spp < left ? a.step_spp : left) : 0u);
    }
    if (lane == 0) {
        a.tile_error[tile] = E;
        a.tile_active[tile] = (uint32_t)__popcll(m_active);
    }
}

__global__ __launch_bounds__(256) void rt_adaptive_combine_kernel(const float *a, const float *b, const uint32_t *count, float *frame, uint32_t *count_out, long long n_pixels)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pixels) return;
    for (int k = 0; k < 3; k++) frame[3 * p + k] = rt_canon_nan((a[3 * p + k] + b[3 * p + k]) * 0.5f);
    if (count_out) count_out[p] = 2u * count[p];
}

extern "C" hipError_t rt_launch_adaptive_plan(const rt_plan_args *args, hipStream_t stream)
{
    const unsigned blocks = ((unsigned)args->num_tiles + RT_PLAN_WAVES - 1u) / RT_PLAN_WAVES;
    hipLaunchKernelGGL(rt_adaptive_plan_kernel, dim3(blocks), dim3(64 * RT_PLAN_WAVES), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_adaptive_combine(const float *a, const float *b, const uint32_t *count, float *frame, uint32_t *count_out, long long n_pixels, hipStream_t stream)
{
    const unsigned blocks = (unsigned)((n_pixels + 255) / 256);
    hipLaunchKernelGGL(rt_adaptive_combine_kernel, dim3(blocks), dim3(256), 0, stream, a, b, count, frame, count_out, n_pixels);
    return hipGetLastError();
}

#endif
