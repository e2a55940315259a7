/*
 * rt_ao_capi.cpp — the ambient-occlusion plane of the C ABI (include/rt_amd.h): argument checks, the host-buffer form.  The kernel is
 * rt_ao_kernel.h; the context and the scene are rt_capi.cpp's, and the checks, the argument block's shared part and the launch are
 * rt_internal.h's, as for rt_occlusion_capi.cpp.
 */
#include <cmath>
#include <cstdint>

#include "rt_internal.h"
#include "rt_ao.h"

namespace {

rt_status check_ao(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, int32_t samples, float radius, float bias, const void *count, const void *ao)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!cam || (!count && !ao)) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (samples < 1 || samples > RT_AO_MAX_SAMPLES) return set_err(ctx, RT_ERR_INVALID, "bad sample count (1 .. 4096)");
    if (!(radius > 0.0f)) return set_err(ctx, RT_ERR_INVALID, "bad radius (> 0, or +inf)");
    if (!(bias >= 0.0f) || !std::isfinite(bias)) return set_err(ctx, RT_ERR_INVALID, "bad bias (>= 0 and finite)");
    return check_image_size(ctx, cam->width, cam->height);
}

}  // namespace

extern "C" rt_status rt_render_ao_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, int32_t samples, float radius, float bias,
                                         int32_t time_ms, uint16_t *d_count, float *d_ao, void *hip_stream)
{
    rt_status st = check_ao(ctx, scene, cam, samples, radius, bias, d_count, d_ao);
    if (st != RT_OK) return st;
    rt_ao_args a = ray_args_view<rt_ao_args>(ctx, scene, cam);
    a.samples = samples;
    a.radius = radius;
    a.bias = bias;
    a.seed = (uint32_t)time_ms * 6291469u;       /* src/raytracer.cu:127 */
    a.count = d_count;
    a.ao = d_ao;
    return launch_rays(ctx, scene, a, rt_launch_ao, true, "launching ambient-occlusion kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_render_ao(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, int32_t samples, float radius, float bias,
                                  int32_t time_ms, uint16_t *count, float *ao)
{
    rt_status st = check_ao(ctx, scene, cam, samples, radius, bias, count, ao);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the context's plane buffer: W * H floats, then W * H counts */
    const size_t px = (size_t)cam->width * (size_t)cam->height;
    RT_HIP(ctx, ctx->d_query_out.grow((px * 6 + sizeof(rt_f4) - 1) / sizeof(rt_f4)), "allocating the planes");
    float *d_ao = (float *)ctx->d_query_out.p;
    uint16_t *d_count = (uint16_t *)(d_ao + px);
    st = rt_render_ao_device(ctx, scene, cam, samples, radius, bias, time_ms, count ? d_count : nullptr, ao ? d_ao : nullptr, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "ambient-occlusion kernel");
    if (count) RT_HIP(ctx, hipMemcpy(count, d_count, px * 2, hipMemcpyDeviceToHost), "copying the counts to host");
    if (ao) RT_HIP(ctx, hipMemcpy(ao, d_ao, px * 4, hipMemcpyDeviceToHost), "copying the plane to host");
    return RT_OK;
}
