/*
 * rt_frame_kernels.h — the small streaming kernels over frames and their launchers (declared in rt_launch.h): the fold of a multi-frame launch's planes into the frame buffer, whole or for a list of tiles, the tile-list exchange
 * copy, and float -> RGBA8.
 */
#ifndef RT_FRAME_KERNELS_H
#define RT_FRAME_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_launch.h"
#include "rt_math.h"

/* The sequential part of a multi-frame launch (src/raytracer.cu:109-112, once per frame): the image
 * after frame n is (c_n + image * n) / (n + 1), c_n = that frame's per-pixel mean (plane n - frame_num
 * of `partial`).  In place on `frame`; its content is used only when frame_num > 0. */
__global__ void rt_blend_kernel(const float *partial, long long plane_floats, int num_frames, int frame_num, float *frame, long long n_floats)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_floats) return;
    float r = frame_num > 0 ? frame[i] : 0.0f;
    for (int k = 0; k < num_frames; k++) {
        const int n = frame_num + k;
        const float previous_sum = r * (float)n;
        r = (partial[(long long)k * plane_floats + i] + previous_sum) / (float)(n + 1);
    }
    frame[i] = rt_canon_nan(r);
}

extern "C" hipError_t rt_launch_blend(const float *partial, long long plane_floats, int num_frames, int frame_num, float *frame, long long n_floats, hipStream_t stream)
{
    const long long blocks = (n_floats + 255) / 256;
    hipLaunchKernelGGL(rt_blend_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, partial, plane_floats, num_frames, frame_num, frame, n_floats);
    return hipGetLastError();
}

/* float i of a tile list's compact image (tile k = i / 192, 64 pixels of 3 floats, row-major inside the tile) -> its
 * index in the full W x H frame, or -1 for the part of a ragged edge tile that lies outside the image */
__device__ __forceinline__ long long rt_tile_float_index(long long i, const uint32_t *tile_list, int tiles_x, int W, int H)
{
    const long long k = i / 192;
    const int r = (int)(i - k * 192), within = r / 3, c = r - within * 3;
    const int g = (int)tile_list[k];
    const int ty = g / tiles_x, tx = g - ty * tiles_x;
    const int x = tx * 8 + (within & 7), y = ty * 8 + (within >> 3);
    if (x >= W || y >= H) return -1;
    return ((long long)y * W + x) * 3 + c;
}

/* the same fold for a launch that rendered a LIST of tiles into a full-layout frame: only the listed tiles' pixels are
 * touched (planes and frame are both full W x H frames) */
__global__ void rt_blend_tiles_kernel(const float *partial, long long plane_floats, int num_frames, int frame_num, float *frame,
                                      const uint32_t *tile_list, long long n_floats, int tiles_x, int W, int H)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_floats) return;
    const long long j = rt_tile_float_index(i, tile_list, tiles_x, W, H);
    if (j < 0) return;
    float r = frame_num > 0 ? frame[j] : 0.0f;
    for (int k = 0; k < num_frames; k++) {
        const int n = frame_num + k;
        const float previous_sum = r * (float)n;
        r = (partial[(long long)k * plane_floats + j] + previous_sum) / (float)(n + 1);
    }
    frame[j] = rt_canon_nan(r);
}

extern "C" hipError_t rt_launch_blend_tiles(const float *partial, long long plane_floats, int num_frames, int frame_num, float *frame,
                                            const uint32_t *tile_list, int n_tiles, int tiles_x, int W, int H, hipStream_t stream)
{
    const long long n_floats = (long long)n_tiles * 192;
    hipLaunchKernelGGL(rt_blend_tiles_kernel, dim3((unsigned)((n_floats + 255) / 256)), dim3(256), 0, stream, partial, plane_floats, num_frames, frame_num,
                       frame, tile_list, n_floats, tiles_x, W, H);
    return hipGetLastError();
}

/* The exchange step of the tile-list partition: a rank's compact image (its tiles back to back)
 * <-> the full frame.  to_frame: frame[tile pixels] = compact; otherwise compact = frame[tile pixels].  Streaming:
 * 12 B read + 12 B written per pixel; the compact side is contiguous, the frame side comes in 96-byte runs. */
__global__ void rt_tiles_copy_kernel(float *compact, float *frame, const uint32_t *tile_list, long long n_floats, int tiles_x, int W, int H, int to_frame)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_floats) return;
    const long long j = rt_tile_float_index(i, tile_list, tiles_x, W, H);
    if (j < 0) return;
    if (to_frame) frame[j] = compact[i];
    else compact[i] = frame[j];
}

extern "C" hipError_t rt_launch_tiles_copy(float *compact, float *frame, const uint32_t *tile_list, int n_tiles, int tiles_x, int W, int H, int to_frame, hipStream_t stream)
{
    const long long n_floats = (long long)n_tiles * 192;
    if (n_floats == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_tiles_copy_kernel, dim3((unsigned)((n_floats + 255) / 256)), dim3(256), 0, stream, compact, frame, tile_list, n_floats, tiles_x, W, H, to_frame);
    return hipGetLastError();
}

/* float -> RGBA8 of src/main.cu:343-371 */
__global__ void rt_rgba8_kernel(const float *rgb, int n_pixels, uint8_t *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    uint32_t packed = 0xff000000u;
    for (int c = 0; c < 3; c++) {
        int colour = rt_f2i(rgb[3 * i + c] * 255.0f);
        colour = colour > 255 ? 255 : (colour < 0 ? 0 : colour);
        packed |= (uint32_t)colour << (8 * c);
    }
    ((uint32_t *)out)[i] = packed;
}

extern "C" hipError_t rt_launch_rgba8(const float *rgb, int n_pixels, uint8_t *out, hipStream_t stream)
{
    int blocks = (n_pixels + 255) / 256;
    hipLaunchKernelGGL(rt_rgba8_kernel, dim3(blocks), dim3(256), 0, stream, rgb, n_pixels, out);
    return hipGetLastError();
}

#endif
