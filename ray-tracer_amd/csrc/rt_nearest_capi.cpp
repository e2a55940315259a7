/*
 * rt_nearest_capi.cpp — the nearest-surface queries of the C ABI (include/rt_amd.h): argument checks, the host-buffer form.  The kernel is
 * rt_nearest_kernel.h, the arithmetic rt_nearest.h; the context and the scene are rt_capi.cpp's, and the checks, the argument block's
 * shared part and the launch (in the context's launch order, between its timing events) are rt_internal.h's.
 */
#include <cstdint>

#include "rt_internal.h"
#include "rt_nearest.h"

namespace {

/* n points on a scene and where the answers go (the limits may be missing) */
rt_status check_nearest(rt_ctx *ctx, const rt_scene *scene, const void *points, int64_t n, const void *out)
{
    const rt_status st = check_points(ctx, scene, points, n);
    if (st != RT_OK) return st;
    if (n > 0 && !out) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_nearest_points_device(rt_ctx *ctx, const rt_scene *scene, const float *d_points, const float *d_max_dist, int64_t n,
                                              rt_nearest *d_out, void *hip_stream)
{
    rt_status st = check_nearest(ctx, scene, d_points, n, d_out);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    if ((uintptr_t)d_out & 15u) return set_err(ctx, RT_ERR_INVALID, "d_out must be 16-byte aligned");
    rt_nearest_args a = ray_args_scene<rt_nearest_args>(ctx, scene, (uint32_t)n);
    a.points = d_points;
    a.max_dist = d_max_dist;
    a.out = d_out;
    return launch_rays(ctx, scene, a, rt_launch_nearest, false, "launching nearest-surface kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_nearest_points(rt_ctx *ctx, const rt_scene *scene, const float *points, const float *max_dist, int64_t n, rt_nearest *out)
{
    rt_status st = check_nearest(ctx, scene, points, n, out);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3;
    static_assert(sizeof(rt_nearest) == 2 * sizeof(rt_f4), "rt_nearest is two 16-byte units");
    RT_HIP(ctx, ctx->d_query_in.grow(floats + (size_t)n), "allocating the points");
    RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, points, floats * 4, hipMemcpyHostToDevice), "copying the points");
    if (max_dist) RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p + floats, max_dist, (size_t)n * 4, hipMemcpyHostToDevice), "copying the limits");
    st = rt_nearest_points_device(ctx, scene, ctx->d_query_in.p, max_dist ? ctx->d_query_in.p + floats : nullptr, n, (rt_nearest *)ctx->d_query_out.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "nearest-surface kernel");
    RT_HIP(ctx, hipMemcpy(out, ctx->d_query_out.p, (size_t)n * sizeof(rt_nearest), hipMemcpyDeviceToHost), "copying the records to host");
    return RT_OK;
}
