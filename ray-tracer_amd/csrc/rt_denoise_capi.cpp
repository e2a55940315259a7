/*
 * rt_denoise_capi.cpp — the edge-avoiding a-trous denoiser of the C ABI (include/rt_amd.h): argument checks, the per-level constants
 * (binary32, on the host), the host-buffer form.  The kernels are rt_denoise_kernel.h; the context is rt_capi.cpp's, and the image-size
 * check and the launch bracket (the context's launch ordering and timing) are rt_internal.h's; there is no scene.
 */
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rt_denoise.h"
#include "rt_internal.h"

namespace {

rt_status check_denoise(rt_ctx *ctx, int32_t width, int32_t height, const void *colour, const void *normal, const void *depth, const void *albedo,
                        const rt_denoise_params *pr, const void *out)
{
    if (!ctx) return RT_ERR_INVALID;
    if (!colour || !normal || !depth || !pr || !out) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (rt_status st = check_image_size(ctx, width, height)) return st;
    if (pr->iterations < 1 || pr->iterations > 8) return set_err(ctx, RT_ERR_INVALID, "bad denoise parameters: iterations (1 .. 8)");
    if (!(pr->sigma_colour > 0.0f) || std::isinf(pr->sigma_colour) || !(pr->sigma_depth > 0.0f) || std::isinf(pr->sigma_depth))
        return set_err(ctx, RT_ERR_INVALID, "bad denoise parameters: sigma_colour and sigma_depth must be positive and finite");
    if (pr->normal_power_log2 < 0 || pr->normal_power_log2 > 8) return set_err(ctx, RT_ERR_INVALID, "bad denoise parameters: normal_power_log2 (0 .. 8)");
    if (albedo && (!(pr->albedo_floor > 0.0f) || std::isinf(pr->albedo_floor)))
        return set_err(ctx, RT_ERR_INVALID, "bad denoise parameters: albedo_floor must be positive and finite");
    if (pr->reserved[0] || pr->reserved[1] || pr->reserved[2]) return set_err(ctx, RT_ERR_INVALID, "bad denoise parameters: reserved fields must be 0");
    return RT_OK;
}

}  // namespace

extern "C" void rt_denoise_params_default(rt_denoise_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->iterations = 5;
    p->sigma_colour = 4.0f;
    p->sigma_depth = 0.02f;
    p->normal_power_log2 = 5;
    p->albedo_floor = 0.01f;
}

extern "C" rt_status rt_denoise_device(rt_ctx *ctx, int32_t width, int32_t height, const float *d_colour, const float *d_normal,
                                       const float *d_depth, const int32_t *d_object, const float *d_albedo,
                                       const rt_denoise_params *params, float *d_out, void *hip_stream)
{
    rt_status st = check_denoise(ctx, width, height, d_colour, d_normal, d_depth, d_albedo, params, d_out);
    if (st != RT_OK) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the context's records: guide, then the two colour buffers the levels alternate between, allocated ahead of the launch bracket (on
     * the context's device: the bracket selects it once more).  A launch still running on another stream reads them until ev_stop (a
     * regrown buffer is freed only after the device is idle: hipFree waits) */
    const size_t px = (size_t)width * (size_t)height;
    RT_HIP(ctx, ctx->d_denoise.grow(3 * px), "allocating the denoise records");
    return launch_bracket(ctx, stream, [&]() -> rt_status {
        rt_denoise_args a;
        std::memset(&a, 0, sizeof a);
        a.width = width; a.height = height;
        a.colour = d_colour; a.normal = d_normal; a.depth = d_depth; a.object = d_object; a.albedo = d_albedo;
        a.albedo_floor = params->albedo_floor;
        a.guide = ctx->d_denoise.p;
        rt_f4 *buf[2] = {ctx->d_denoise.p + px, ctx->d_denoise.p + 2 * px};
        a.dst = buf[0];
        a.out = d_out;
        a.sigma_depth = params->sigma_depth;
        a.normal_power_log2 = params->normal_power_log2;
        RT_HIP(ctx, rt_launch_denoise_pack(&a, stream), "launching the denoise pack kernel");
        for (int i = 0; i < params->iterations; i++) {
            /* sc = sigma_colour * 2^-i (exact), kc = 1 / (sc * sc): three binary32 operations, each rounded once */
            const float sc = params->sigma_colour * std::ldexp(1.0f, -i);
            const float sc2 = sc * sc;
            a.kc = 1.0f / sc2;
            a.step = 1 << i;
            a.inv_step = std::ldexp(1.0f, -i);
            a.src = buf[i & 1];
            a.dst = buf[(i + 1) & 1];
            RT_HIP(ctx, rt_launch_denoise_level(&a, i == params->iterations - 1, stream), "launching a denoise level kernel");
        }
        return RT_OK;
    });
}

extern "C" rt_status rt_denoise(rt_ctx *ctx, int32_t width, int32_t height, const float *colour, const float *normal, const float *depth,
                                const int32_t *object, const float *albedo, const rt_denoise_params *params, float *out)
{
    rt_status st = check_denoise(ctx, width, height, colour, normal, depth, albedo, params, out);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the planes one after another in the context's input buffer (floats; the object plane's int32 are as wide), the result in its output buffer */
    const size_t px = (size_t)width * (size_t)height;
    const void *host[5] = {colour, normal, depth, object, albedo};
    const size_t width_of[5] = {3, 3, 1, 1, 3};
    float *dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t total = 0;
    for (int k = 0; k < 5; k++) if (host[k]) total += width_of[k] * px;
    RT_HIP(ctx, ctx->d_query_in.grow(total), "allocating the planes");
    RT_HIP(ctx, ctx->d_query_out.grow((3 * px + 3) / 4), "allocating the result");
    float *at = ctx->d_query_in.p;
    for (int k = 0; k < 5; k++)
        if (host[k]) {
            dev[k] = at;
            at += width_of[k] * px;
            RT_HIP(ctx, hipMemcpy(dev[k], host[k], width_of[k] * px * 4, hipMemcpyHostToDevice), "copying a plane to the device");
        }
    st = rt_denoise_device(ctx, width, height, dev[0], dev[1], dev[2], (const int32_t *)dev[3], dev[4], params, (float *)ctx->d_query_out.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "denoise kernels");
    RT_HIP(ctx, hipMemcpy(out, ctx->d_query_out.p, 3 * px * 4, hipMemcpyDeviceToHost), "copying the result to host");
    return RT_OK;
}
