/*
 * rt_query_capi.cpp — the closest-hit ray queries and the first-hit AOV pass of the C ABI (include/rt_amd.h): argument checks, the
 * host-buffer forms.  The kernels are rt_query_kernel.h; the context and the scene are rt_capi.cpp's, and the checks, the argument
 * block's shared part and the launch (in the context's launch order, between its timing events) are rt_internal.h's.  A translation
 * unit of its own so that rt_capi.cpp links without the query launcher.
 */
#include <cstdint>
#include <cstring>

#include "rt_internal.h"
#include "rt_query.h"

namespace {

rt_status check_aov(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float *sky, bool any_plane)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!cam || !sky) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (!any_plane) return set_err(ctx, RT_ERR_INVALID, "no plane requested");
    return check_image_size(ctx, cam->width, cam->height);
}

}  // namespace

extern "C" rt_status rt_trace_rays_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions, int64_t n,
                                          rt_hit *d_hits, void *hip_stream)
{
    rt_status st = check_rays(ctx, scene, d_origins, d_directions, n, d_hits);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    if ((uintptr_t)d_hits & 15u) return set_err(ctx, RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    rt_query_args a = ray_args_scene<rt_query_args>(ctx, scene, (uint32_t)n);
    a.tri_uv = scene->d_tri_uv.p;
    a.tex_data = scene->d_tex.p;
    a.origins = d_origins;
    a.directions = d_directions;
    a.hits = d_hits;
    return launch_rays(ctx, scene, a, rt_launch_query, false, "launching query kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_trace_rays(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, int64_t n, rt_hit *hits)
{
    rt_status st = check_rays(ctx, scene, origins, directions, n, hits);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3;
    static_assert(sizeof(rt_hit) == 3 * sizeof(rt_f4), "rt_hit is three 16-byte units");
    RT_HIP(ctx, ctx->d_query_in.grow(2 * floats), "allocating the rays");
    RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 3), "allocating the hit records");
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, origins, floats * 4, hipMemcpyHostToDevice), "copying ray origins");
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p + floats, directions, floats * 4, hipMemcpyHostToDevice), "copying ray directions");
    st = rt_trace_rays_device(ctx, scene, ctx->d_query_in.p, ctx->d_query_in.p + floats, n, (rt_hit *)ctx->d_query_out.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "query kernel");
    RT_HIP(ctx, hipMemcpy(hits, ctx->d_query_out.p, (size_t)n * sizeof(rt_hit), hipMemcpyDeviceToHost), "copying hit records to host");
    return RT_OK;
}

extern "C" rt_status rt_render_aov_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float sky_colour[3],
                                          float *d_depth, float *d_normal, float *d_albedo, int32_t *d_object, float *d_ray, void *hip_stream)
{
    rt_status st = check_aov(ctx, scene, cam, sky_colour, d_depth || d_normal || d_albedo || d_object || d_ray);
    if (st != RT_OK) return st;
    rt_query_args a = ray_args_view<rt_query_args>(ctx, scene, cam);
    a.tri_uv = scene->d_tri_uv.p;
    a.tex_data = scene->d_tex.p;
    std::memcpy(a.sky, sky_colour, 12);
    a.depth = d_depth; a.normal = d_normal; a.albedo = d_albedo; a.object = d_object; a.ray = d_ray;
    return launch_rays(ctx, scene, a, rt_launch_query, true, "launching query kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_render_aov(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float sky_colour[3],
                                   float *depth, float *normal, float *albedo, int32_t *object, float *ray)
{
    rt_status st = check_aov(ctx, scene, cam, sky_colour, depth || normal || albedo || object || ray);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the requested planes one after another in the context's output buffer (floats; the object plane's int32 are as wide) */
    const size_t px = (size_t)cam->width * (size_t)cam->height;
    void *host[5] = {depth, normal, albedo, object, ray};
    const size_t width[5] = {1, 3, 3, 1, 3};
    float *dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t total = 0;
    for (int k = 0; k < 5; k++) if (host[k]) total += width[k] * px;
    RT_HIP(ctx, ctx->d_query_out.grow((total + 3) / 4), "allocating the planes");
    float *at = (float *)ctx->d_query_out.p;
    for (int k = 0; k < 5; k++) if (host[k]) { dev[k] = at; at += width[k] * px; }
    st = rt_render_aov_device(ctx, scene, cam, sky_colour, dev[0], dev[1], dev[2], (int32_t *)dev[3], dev[4], nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "query kernel");
    for (int k = 0; k < 5; k++)
        if (host[k]) RT_HIP(ctx, hipMemcpy(host[k], dev[k], width[k] * px * 4, hipMemcpyDeviceToHost), "copying a plane to host");
    return RT_OK;
}
