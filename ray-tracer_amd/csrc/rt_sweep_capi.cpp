/*
 * rt_sweep_capi.cpp — the sphere-cast queries of the C ABI (include/rt_amd.h): argument checks, the two launches, the host-buffer form.  The
 * kernel is rt_sweep_kernel.h, the arithmetic rt_sweep.h; the context and the scene are rt_capi.cpp's, and the checks, the argument block's
 * shared part and the launch (in the context's launch order, between its timing events) are rt_internal.h's.
 *
 * A call is the nearest-surface launch over the origins with the radii as its limits - which decides, by that query's own definition, which
 * balls touch the scene at the start - and then the sweep kernel (rt_launch_sweep), which reads those records; both
 * inside one launch bracket, as rt_signed_distance_device chains its two.
 */
#include <cstdint>

#include "rt_internal.h"
#include "rt_nearest.h"
#include "rt_sweep.h"

namespace {

static_assert(RT_SWEEP_MAX_QUERIES == RT_NEAREST_MAX_POINTS, "check_points serves the sweep too");

/* n balls on a scene and where the answers go (the limits may be missing) */
rt_status check_sweep(rt_ctx *ctx, const rt_scene *scene, const void *origins, const void *directions, const void *radius, int64_t n, const void *out)
{
    const rt_status st = check_points(ctx, scene, origins, n);
    if (st != RT_OK) return st;
    if (n > 0 && (!directions || !radius || !out)) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return RT_OK;
}

/* the two launches; d_near: n nearest-surface records to write and read, or NULL: the context's record buffer */
rt_status sweep_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions, const float *d_radius, const float *d_tmax,
                       int64_t n, rt_sweep *d_out, rt_nearest *d_near, hipStream_t stream)
{
    if ((uintptr_t)d_out & 15u) return set_err(ctx, RT_ERR_INVALID, "d_out must be 16-byte aligned");
    if (!d_near) {
        /* the context's record buffer: grown once what may still read the old one has run */
        if (ctx->d_query_out.cap < (size_t)n * 2 || !ctx->d_query_out.p) {
            if (ctx->launched) RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for the launch that uses the records");
            RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
        }
        d_near = (rt_nearest *)ctx->d_query_out.p;
    }
    rt_nearest_args na = ray_args_scene<rt_nearest_args>(ctx, scene, (uint32_t)n);
    na.points = d_origins;
    na.max_dist = d_radius;
    na.out = d_near;
    rt_sweep_args sa = ray_args_scene<rt_sweep_args>(ctx, scene, (uint32_t)n);
    sa.origins = d_origins;
    sa.directions = d_directions;
    sa.radius = d_radius;
    sa.tmax = d_tmax;
    sa.nearest = d_near;
    sa.out = d_out;
    return launch_bracket(ctx, stream, [&]() -> rt_status {
        const rt_status queued = enqueue_rays(ctx, scene, na, rt_launch_nearest, false, "clearing the point counter", "launching nearest-surface kernel", stream);
        if (queued != RT_OK) return queued;
        RT_HIP(ctx, hipEventRecord(ctx->ev_start, stream), "recording start event");        /* (again: rt_last_kernel_ms starts at the sweep kernel) */
        return enqueue_rays(ctx, scene, sa, rt_launch_sweep, false, "clearing the ball counter", "launching sphere-cast kernel", stream);
    });
}

}  // namespace

extern "C" rt_status rt_sweep_spheres_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions, const float *d_radius,
                                             const float *d_tmax, int64_t n, rt_sweep *d_out, void *hip_stream)
{
    const rt_status st = check_sweep(ctx, scene, d_origins, d_directions, d_radius, n, d_out);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    return sweep_device(ctx, scene, d_origins, d_directions, d_radius, d_tmax, n, d_out, nullptr, (hipStream_t)hip_stream);
}

extern "C" rt_status rt_sweep_spheres(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, const float *radius,
                                      const float *tmax, int64_t n, rt_sweep *out)
{
    rt_status st = check_sweep(ctx, scene, origins, directions, radius, n, out);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the origins, the directions, the radii and the limits, one after the other; the sweep records, then the nearest-surface records */
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(2 * floats + 2 * (size_t)n), "allocating the balls");
    RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 5), "allocating the records");
    float *d_o = ctx->d_query_in.p, *d_d = d_o + floats, *d_r = d_d + floats, *d_lim = d_r + (size_t)n;
    RT_HIP(ctx, hipMemcpy(d_o, origins, floats * 4, hipMemcpyHostToDevice), "copying the origins");
    RT_HIP(ctx, hipMemcpy(d_d, directions, floats * 4, hipMemcpyHostToDevice), "copying the directions");
    RT_HIP(ctx, hipMemcpy(d_r, radius, (size_t)n * 4, hipMemcpyHostToDevice), "copying the radii");
    if (tmax) RT_HIP(ctx, hipMemcpy(d_lim, tmax, (size_t)n * 4, hipMemcpyHostToDevice), "copying the limits");
    st = sweep_device(ctx, scene, d_o, d_d, d_r, tmax ? d_lim : nullptr, n, (rt_sweep *)ctx->d_query_out.p, (rt_nearest *)(ctx->d_query_out.p + (size_t)n * 3), nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "sphere-cast kernels");
    RT_HIP(ctx, hipMemcpy(out, ctx->d_query_out.p, (size_t)n * sizeof(rt_sweep), hipMemcpyDeviceToHost), "copying the records to host");
    return RT_OK;
}
