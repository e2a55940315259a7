/*
 * rt_denoise_kernel.h — the edge-avoiding a-trous wavelet filter of rt_denoise (include/rt_amd.h has the definition; the operation
 * order below IS the interface: tests/denoise_ref.py reproduces it bit for bit).  Part of rt_kernel.hip's translation unit (one code object for the
 * library); the launchers at the end are declared in rt_launch.h.
 *
 * Nothing here traverses a scene: the passes are image-space.  This is a first, untuned shape: correct to the bit, measured, not optimised.
 *   pack    one lane per pixel: reads the caller's planes (12-byte pixels), demodulates, writes two 16-byte records per pixel -
 *           colour {F.r, F.g, F.b, object bits} and guide {N.x, N.y, N.z, Z} - so that a tap is two aligned dwordx4 loads;
 *   level   one lane per pixel, a workgroup per 32 x 8 tile: the 5 x 5 stencil dilated by `step`, 24 taps read straight from the
 *           records with global loads (an LDS tile for the small steps was not built and not measured), the centre from registers.
 *           The tap loops are unrolled, so every spline weight is a literal, and a tap outside the image loads from a clamped
 *           address.  AS COMPILED for gfx950 the taps are NOT independent: each is a region of its own - its two loads, a wait for
 *           them, a scalar loop for the normal power, the weight under an exec mask ("inside and same object"), the accumulation
 *           under a second one ("w != 0"), a wait for all loads before the next tap - so a wave has one pair of loads in flight
 *           and takes about six branches per tap (DESIGN.md §12 has the disassembly's summary and what a select-based rewrite
 *           compiles to).  The last level remodulates and writes interleaved RGB.
 * No LDS, no atomics, no cross-lane operations; registers and scratch are checked by tests/test_denoise_abi.py.
 */
#ifndef RT_DENOISE_KERNEL_H
#define RT_DENOISE_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_denoise.h"
#include "rt_device_scene.h"
#include "rt_launch.h"

#define RT_DN_TILE_X 32
#define RT_DN_TILE_Y 8

/* k(x) = (x < 1) ? (1 - x)^2 : 0, the compactly supported falloff (a NaN compares false: 0) */
__device__ __forceinline__ float rt_dn_falloff(float x)
{
    const float t = 1.0f - x;
    return x < 1.0f ? t * t : 0.0f;
}

__global__ __launch_bounds__(256) void rt_denoise_pack_kernel(const rt_denoise_args a)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.width * a.height) return;
    float r = a.colour[3 * p + 0], g = a.colour[3 * p + 1], b = a.colour[3 * p + 2];
    if (a.albedo) {
        const float ar = a.albedo[3 * p + 0], ag = a.albedo[3 * p + 1], ab = a.albedo[3 * p + 2];
        r = r / (ar > a.albedo_floor ? ar : a.albedo_floor);
        g = g / (ag > a.albedo_floor ? ag : a.albedo_floor);
        b = b / (ab > a.albedo_floor ? ab : a.albedo_floor);
    }
    a.dst[p] = rt_f4{r, g, b, __int_as_float(a.object ? a.object[p] : 0)};
    a.guide[p] = rt_f4{a.normal[3 * p + 0], a.normal[3 * p + 1], a.normal[3 * p + 2], a.depth[p]};
}

template <bool LAST>
__global__ __launch_bounds__(RT_DN_TILE_X * RT_DN_TILE_Y) void rt_denoise_level_kernel(const rt_denoise_args a)
{
    const int x = blockIdx.x * RT_DN_TILE_X + (threadIdx.x & (RT_DN_TILE_X - 1)), y = blockIdx.y * RT_DN_TILE_Y + threadIdx.x / RT_DN_TILE_X;
    if (x >= a.width || y >= a.height) return;
    const int p = y * a.width + x;
    const rt_f4 fp = a.src[p], gp = a.guide[p];
    const float kz = 1.0f / (a.sigma_depth * gp.w);
    const int object = __float_as_int(fp.w);
    /* {1/6, 2/3, 1, 2/3, 1/6} as the nearest binary32 values: the B3 spline 1:4:6:4:1 scaled so that the centre is exactly 1 */
    constexpr float h[5] = {0x1.555556p-3f, 0x1.555556p-1f, 1.0f, 0x1.555556p-1f, 0x1.555556p-3f};
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            if (dx == 0 && dy == 0) {                   /* w = 1: the weight functions are not evaluated */
                acc_r = acc_r + fp.x; acc_g = acc_g + fp.y; acc_b = acc_b + fp.z;
                wsum = wsum + 1.0f;
                continue;
            }
            const int qx = x + dx * a.step, qy = y + dy * a.step;
            const bool inside = qx >= 0 && qx < a.width && qy >= 0 && qy < a.height;
            /* a tap outside the image is skipped: its load is clamped into the image and its weight forced to 0 */
            const int cx = qx < 0 ? 0 : (qx >= a.width ? a.width - 1 : qx), cy = qy < 0 ? 0 : (qy >= a.height ? a.height - 1 : qy);
            const int q = cy * a.width + cx;
            const rt_f4 fq = a.src[q], gq = a.guide[q];
            const float hw = h[dy + 2] * h[dx + 2];                                  /* one rounding; a literal once the loops are unrolled */
            const int ring = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy);
            const float inv_r = ring == 2 ? a.inv_step * 0.5f : a.inv_step;            /* 1 / (max(|dx|, |dy|) * s): a power of two */
            const float dn = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
            float wn = dn > 0.0f ? dn : 0.0f;
            for (int k = 0; k < a.normal_power_log2; k++) wn = wn * wn;
            const float gz = ((gq.w - gp.w) * kz) * inv_r;
            const float wz = rt_dn_falloff(gz * gz);
            const float dr = fq.x - fp.x, dg = fq.y - fp.y, db = fq.z - fp.z;
            const float wc = rt_dn_falloff(((dr * dr + dg * dg) + db * db) * a.kc);
            float w = hw * ((wn * wz) * wc);
            if (!inside || __float_as_int(fq.w) != object) w = 0.0f;
            if (w != 0.0f) {                            /* (a zero weight is skipped, so a non-finite colour behind it does not spread) */
                acc_r = acc_r + w * fq.x; acc_g = acc_g + w * fq.y; acc_b = acc_b + w * fq.z;
                wsum = wsum + w;
            }
        }
    }
    float r = acc_r / wsum, g = acc_g / wsum, b = acc_b / wsum;       /* wsum >= 1 */
    if (!LAST) {
        a.dst[p] = rt_f4{r, g, b, fp.w};
        return;
    }
    if (a.albedo) {
        const float ar = a.albedo[3 * p + 0], ag = a.albedo[3 * p + 1], ab = a.albedo[3 * p + 2];
        r = r * (ar > a.albedo_floor ? ar : a.albedo_floor);
        g = g * (ag > a.albedo_floor ? ag : a.albedo_floor);
        b = b * (ab > a.albedo_floor ? ab : a.albedo_floor);
    }
    a.out[3 * p + 0] = r; a.out[3 * p + 1] = g; a.out[3 * p + 2] = b;
}

extern "C" hipError_t rt_launch_denoise_pack(const rt_denoise_args *args, hipStream_t stream)
{
    const unsigned blocks = ((unsigned)args->width * (unsigned)args->height + 255u) / 256u;
    hipLaunchKernelGGL(rt_denoise_pack_kernel, dim3(blocks), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_denoise_level(const rt_denoise_args *args, int last, hipStream_t stream)
{
    const dim3 grid((args->width + RT_DN_TILE_X - 1) / RT_DN_TILE_X, (args->height + RT_DN_TILE_Y - 1) / RT_DN_TILE_Y);
    if (last) hipLaunchKernelGGL(rt_denoise_level_kernel<true>, grid, dim3(RT_DN_TILE_X * RT_DN_TILE_Y), 0, stream, *args);
    else hipLaunchKernelGGL(rt_denoise_level_kernel<false>, grid, dim3(RT_DN_TILE_X * RT_DN_TILE_Y), 0, stream, *args);
    return hipGetLastError();
}

#endif
