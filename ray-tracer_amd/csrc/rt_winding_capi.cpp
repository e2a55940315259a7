/*
 * rt_winding_capi.cpp — the winding-number queries of the C ABI (include/rt_amd.h): argument checks, the scene's flip bytes on the device,
 * the host-buffer forms.  The kernel is rt_winding_kernel.h, the arithmetic rt_winding.h; rt_signed_distance_device also runs the
 * nearest-surface kernel (as rt_nearest_capi.cpp runs it).  The context, the scene, the launch bracket and the ray kernels' enqueue are
 * rt_internal.h's.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_internal.h"
#include "rt_nearest.h"
#include "rt_winding.h"

namespace {

rt_status check_winding(rt_ctx *ctx, const rt_scene *scene, const void *points, int64_t n, int32_t object, const void *winding, const void *inside)
{
    rt_status st = check_points(ctx, scene, points, n);
    if (st != RT_OK) return st;
    if (object != RT_WINDING_SOLIDS && (object < 0 || (size_t)object >= scene->flat.objects.size()))
        return set_err(ctx, RT_ERR_INVALID, "object is neither RT_WINDING_SOLIDS nor an index of the scene's object list");
    if (n > 0 && !winding && !inside) return set_err(ctx, RT_ERR_INVALID, "null argument (one of the two outputs is needed)");
    return RT_OK;
}

/* what the kernel reads beside the blob, made at the scene's first query: the triangle order (unless an update already made it) and the
 * flip bytes in commit order, four to a word */
rt_status prepare_scene(rt_ctx *ctx, rt_scene *scene)
{
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const rt_status st = ensure_scene_perm(ctx, scene);
    if (st != RT_OK) return st;
    if (scene->d_flip.p) return RT_OK;
    const std::vector<uint8_t> &bytes = scene->flat.tri_flip_commit;
    std::vector<uint32_t> words((bytes.size() + 3) / 4, 0u);
    if (!bytes.empty()) std::memcpy(words.data(), bytes.data(), bytes.size());
    RT_HIP(ctx, scene->d_flip.grow(words.size()), "allocating the scene's flip bytes");
    const hipError_t e = words.empty() ? hipSuccess : hipMemcpy(scene->d_flip.p, words.data(), words.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        scene->d_flip.release();
        return hip_fail(ctx, e, "uploading the scene's flip bytes");
    }
    return RT_OK;
}

rt_winding_args winding_args(const rt_ctx *ctx, const rt_scene *scene, const float *d_points, uint32_t n, int32_t object)
{
    rt_winding_args a;
    std::memset(&a, 0, sizeof a);
    a.blob = scene->d_blob.p;
    a.off_tris = scene->flat.off_tris;
    a.off_objtab = scene->flat.off_objtab;
    a.num_objects = (int32_t)scene->flat.objects.size();
    a.num_tris = scene->flat.num_tris;
    a.perm = scene->d_perm.p;
    a.flip = scene->d_flip.p;
    a.n = n;
    a.num_chunks = (n + 63u) / 64u;
    a.counter = ctx->tile_counter.p;
    a.points = d_points;
    a.object = object;
    return a;
}

rt_status enqueue_winding(rt_ctx *ctx, const rt_winding_args &a, hipStream_t stream)
{
    RT_HIP(ctx, hipMemsetAsync(a.counter, 0, 512, stream), "clearing the point counter");
    RT_HIP(ctx, rt_launch_winding(&a, ctx->num_cus, stream), "launching winding-number kernel");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_winding_numbers_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, int64_t n, int32_t object, float *d_winding,
                                               uint8_t *d_inside, void *hip_stream)
{
    rt_status st = check_winding(ctx, scene, d_points, n, object, d_winding, d_inside);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    if ((st = prepare_scene(ctx, scene)) != RT_OK) return st;
    rt_winding_args a = winding_args(ctx, scene, d_points, (uint32_t)n, object);
    a.winding = d_winding;
    a.inside = d_inside;
    hipStream_t stream = (hipStream_t)hip_stream;
    return launch_bracket(ctx, stream, [&]() -> rt_status { return enqueue_winding(ctx, a, stream); });
}

extern "C" rt_status rt_winding_numbers(rt_ctx *ctx, rt_scene *scene, const float *points, int64_t n, int32_t object, float *winding, uint8_t *inside)
{
    rt_status st = check_winding(ctx, scene, points, n, object, winding, inside);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the points, the winding numbers and the bytes (a float's room each), one after the other */
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(floats + 2 * (size_t)n), "allocating the points");
    float *d_w = ctx->d_query_in.p + floats;
    uint8_t *d_in = (uint8_t *)(d_w + (size_t)n);
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, points, floats * 4, hipMemcpyHostToDevice), "copying the points");
    st = rt_winding_numbers_device(ctx, scene, ctx->d_query_in.p, n, object, winding ? d_w : nullptr, inside ? d_in : nullptr, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "winding-number kernel");
    if (winding) RT_HIP(ctx, hipMemcpy(winding, d_w, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the winding numbers to host");
    if (inside) RT_HIP(ctx, hipMemcpy(inside, d_in, (size_t)n, hipMemcpyDeviceToHost), "copying the containment bytes to host");
    return RT_OK;
}

extern "C" rt_status rt_signed_distance_device(rt_ctx *ctx, rt_scene *scene, const float *d_points, const float *d_max_dist, int64_t n,
                                               rt_nearest *d_nearest, float *d_sdf, void *hip_stream)
{
    rt_status st = check_points(ctx, scene, d_points, n);
    if (st != RT_OK) return st;
    if (n > 0 && !d_sdf) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if ((uintptr_t)d_nearest & 15u) return set_err(ctx, RT_ERR_INVALID, "d_nearest must be 16-byte aligned");
    if (n == 0) return RT_OK;
    if ((st = prepare_scene(ctx, scene)) != RT_OK) return st;
    if (!d_nearest) {
        /* the context's record buffer: grown once what may still read the old one has run */
        static_assert(sizeof(rt_nearest) == 2 * sizeof(rt_f4), "rt_nearest is two 16-byte units");
        if (ctx->d_query_out.cap < (size_t)n * 2 || !ctx->d_query_out.p) {
            if (ctx->launched) RT_HIP(ctx, hipEventSynchronize(ctx->ev_stop), "waiting for the launch that uses the records");
            RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
        }
        d_nearest = (rt_nearest *)ctx->d_query_out.p;
    }
    rt_nearest_args na = ray_args_scene<rt_nearest_args>(ctx, scene, (uint32_t)n);
    na.points = d_points;
    na.max_dist = d_max_dist;
    na.out = d_nearest;
    rt_winding_args wa = winding_args(ctx, scene, d_points, (uint32_t)n, RT_WINDING_SOLIDS);
    wa.nearest = d_nearest;
    wa.sdf = d_sdf;
    hipStream_t stream = (hipStream_t)hip_stream;
    return launch_bracket(ctx, stream, [&]() -> rt_status {
        const rt_status queued = enqueue_rays(ctx, scene, na, rt_launch_nearest, false, "clearing the point counter", "launching nearest-surface kernel", stream);
        return queued != RT_OK ? queued : enqueue_winding(ctx, wa, stream);
    });
}

extern "C" rt_status rt_signed_distance(rt_ctx *ctx, rt_scene *scene, const float *points, const float *max_dist, int64_t n, rt_nearest *nearest,
                                        float *sdf)
{
    rt_status st = check_points(ctx, scene, points, n);
    if (st != RT_OK) return st;
    if (n > 0 && !sdf) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the points, the limits and the signed distances, one after the other; the records in the context's record buffer */
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(floats + 2 * (size_t)n), "allocating the points");
    RT_HIP(ctx, ctx->d_query_out.grow((size_t)n * 2), "allocating the records");
    float *d_lim = ctx->d_query_in.p + floats, *d_sdf = d_lim + (size_t)n;
    RT_HIP(ctx, hipMemcpy(ctx->d_query_in.p, points, floats * 4, hipMemcpyHostToDevice), "copying the points");
    if (max_dist) RT_HIP(ctx, hipMemcpy(d_lim, max_dist, (size_t)n * 4, hipMemcpyHostToDevice), "copying the limits");
    st = rt_signed_distance_device(ctx, scene, ctx->d_query_in.p, max_dist ? d_lim : nullptr, n, (rt_nearest *)ctx->d_query_out.p, d_sdf, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "signed-distance kernels");
    RT_HIP(ctx, hipMemcpy(sdf, d_sdf, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the signed distances to host");
    if (nearest) RT_HIP(ctx, hipMemcpy(nearest, ctx->d_query_out.p, (size_t)n * sizeof(rt_nearest), hipMemcpyDeviceToHost), "copying the records to host");
    return RT_OK;
}
