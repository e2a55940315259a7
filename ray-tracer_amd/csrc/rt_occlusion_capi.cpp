/*
 * rt_occlusion_capi.cpp — the occlusion (any-hit) ray queries and the light-visibility plane of the C ABI (include/rt_amd.h): argument
 * checks, the host-buffer forms.  The kernels are rt_occlusion_kernel.h; the context and the scene are rt_capi.cpp's, and the checks, the
 * argument block's shared part and the launch are rt_internal.h's, as for rt_query_capi.cpp.
 */
#include <cstdint>
#include <cstring>

#include "rt_internal.h"
#include "rt_occlusion.h"

namespace {

rt_status check_visibility(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float *light_pos, const void *visibility)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!cam || !light_pos || !visibility) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return check_image_size(ctx, cam->width, cam->height);
}

}  // namespace

extern "C" rt_status rt_occluded_rays_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions,
                                             const float *d_tmax, int64_t n, uint8_t *d_occluded, void *hip_stream)
{
    rt_status st = check_rays(ctx, scene, d_origins, d_directions, n, d_occluded);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    rt_occlusion_args a = ray_args_scene<rt_occlusion_args>(ctx, scene, (uint32_t)n);
    a.origins = d_origins;
    a.directions = d_directions;
    a.tmax = d_tmax;
    a.out = d_occluded;
    return launch_rays(ctx, scene, a, rt_launch_occlusion, false, "launching occlusion kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_occluded_rays(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, const float *tmax,
                                      int64_t n, uint8_t *occluded)
{
    rt_status st = check_rays(ctx, scene, origins, directions, n, occluded);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(2 * floats + (size_t)n), "allocating the rays");
    RT_HIP(ctx, ctx->d_query_out.grow(((size_t)n + sizeof(rt_f4) - 1) / sizeof(rt_f4)), "allocating the answers");
    float *d_o = ctx->d_query_in.p, *d_d = d_o + floats, *d_t = tmax ? d_d + floats : nullptr;
    RT_HIP(ctx, hipMemcpy(d_o, origins, floats * 4, hipMemcpyHostToDevice), "copying ray origins");
    RT_HIP(ctx, hipMemcpy(d_d, directions, floats * 4, hipMemcpyHostToDevice), "copying ray directions");
    if (tmax) RT_HIP(ctx, hipMemcpy(d_t, tmax, (size_t)n * 4, hipMemcpyHostToDevice), "copying ray limits");
    st = rt_occluded_rays_device(ctx, scene, d_o, d_d, d_t, n, (uint8_t *)ctx->d_query_out.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "occlusion kernel");
    RT_HIP(ctx, hipMemcpy(occluded, ctx->d_query_out.p, (size_t)n, hipMemcpyDeviceToHost), "copying the answers to host");
    return RT_OK;
}

extern "C" rt_status rt_render_visibility_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float light_pos[3], float bias,
                                                 uint8_t *d_visibility, void *hip_stream)
{
    rt_status st = check_visibility(ctx, scene, cam, light_pos, d_visibility);
    if (st != RT_OK) return st;
    rt_occlusion_args a = ray_args_view<rt_occlusion_args>(ctx, scene, cam);
    std::memcpy(a.light, light_pos, 12);
    a.bias = bias;
    a.out = d_visibility;
    return launch_rays(ctx, scene, a, rt_launch_occlusion, true, "launching occlusion kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_render_visibility(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float light_pos[3], float bias,
                                          uint8_t *visibility)
{
    rt_status st = check_visibility(ctx, scene, cam, light_pos, visibility);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t px = (size_t)cam->width * (size_t)cam->height;
    RT_HIP(ctx, ctx->d_query_out.grow((px + sizeof(rt_f4) - 1) / sizeof(rt_f4)), "allocating the plane");
    st = rt_render_visibility_device(ctx, scene, cam, light_pos, bias, (uint8_t *)ctx->d_query_out.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "occlusion kernel");
    RT_HIP(ctx, hipMemcpy(visibility, ctx->d_query_out.p, px, hipMemcpyDeviceToHost), "copying the plane to host");
    return RT_OK;
}
