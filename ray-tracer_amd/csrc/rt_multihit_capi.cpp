/*
 * rt_multihit_capi.cpp — the multi-hit ray queries of the C ABI (include/rt_amd.h): argument checks, the host-buffer form.  The kernel is
 * rt_multihit_kernel.h, the candidate tests, the buffer and the walk rt_multihit.h; the context and the scene are rt_capi.cpp's, and the
 * checks, the argument block's shared part and the launch (in the context's launch order, between its timing events) are rt_internal.h's.
 */
#include <cstdint>

#include "rt_internal.h"
#include "rt_multihit.h"

namespace {

/* n rays on a scene, k records each and where the answers go (the limits may be missing, and the counts while k > 0) */
rt_status check_multi(rt_ctx *ctx, const rt_scene *scene, const void *origins, const void *directions, int64_t n, int32_t k, const void *hits, const void *counts)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (n < 0 || n > RT_MULTIHIT_MAX_RAYS) return set_err(ctx, RT_ERR_INVALID, "bad ray count (0 .. 2^30)");
    if (k < 0 || k > RT_MULTIHIT_MAX) return set_err(ctx, RT_ERR_INVALID, "bad record count per ray (0 .. RT_MULTIHIT_MAX)");
    if (n == 0) return RT_OK;          /* nothing to do: nothing is looked at */
    if (!origins || !directions) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (k > 0 && !hits) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (k == 0 && !counts) return set_err(ctx, RT_ERR_INVALID, "null counts in count-only mode");
    if (scene->flat.objects.size() > RT_MH_MAX_OBJECTS) return set_err(ctx, RT_ERR_INVALID, "scene has too many objects for a multi-hit query (at most 4096)");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_trace_rays_multi_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions, const float *d_tmax,
                                                int64_t n, int32_t k, rt_hit *d_hits, int32_t *d_counts, void *hip_stream)
{
    rt_status st = check_multi(ctx, scene, d_origins, d_directions, n, k, d_hits, d_counts);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    if (k > 0 && ((uintptr_t)d_hits & 15u)) return set_err(ctx, RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    rt_multihit_args a = ray_args_scene<rt_multihit_args>(ctx, scene, (uint32_t)n);
    a.tri_uv = scene->d_tri_uv.p;
    a.origins = d_origins;
    a.directions = d_directions;
    a.tmax = d_tmax;
    a.k = k;
    a.hits = d_hits;
    a.counts = d_counts;
    /* the records on a sphere whose material needs texture coordinates get them in a second pass: only where the scene has such a sphere */
    bool sphere_uv = false;
    for (const rt_object &ob : scene->flat.objects) sphere_uv = sphere_uv || (ob.type == RT_OBJ_SPHERE && ob.need_uv);
    rt_multihit_uv_args uv;
    uv.objlds = scene->d_blob.p + scene->flat.off_objlds;
    uv.hits = d_hits;
    uv.records = n * (int64_t)k;
    const hipStream_t stream = (hipStream_t)hip_stream;
    return launch_bracket(ctx, stream, [&]() -> rt_status {
        const rt_status queued = enqueue_rays(ctx, scene, a, rt_launch_multihit, false, "clearing the ray counter", "launching multi-hit kernel", stream);
        if (queued != RT_OK) return queued;
        if (sphere_uv && k > 0) RT_HIP(ctx, rt_launch_multihit_uv(&uv, ctx->num_cus, stream), "launching multi-hit texture-coordinate kernel");
        return RT_OK;
    });
}

extern "C" rt_status rt_trace_rays_multi(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, const float *tmax, int64_t n, int32_t k,
                                         rt_hit *hits, int32_t *counts)
{
    rt_status st = check_multi(ctx, scene, origins, directions, n, k, hits, counts);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3, records = (size_t)n * (size_t)k;
    static_assert(sizeof(rt_hit) == 3 * sizeof(rt_f4), "rt_hit is three 16-byte units");
    /* in: origins, directions, limits; out: the records, then the counts (n int32 in (n + 3) / 4 units) */
    RT_HIP(ctx, ctx->d_query_in.grow(2 * floats + (size_t)n), "allocating the rays");
    RT_HIP(ctx, ctx->d_query_out.grow(records * 3 + ((size_t)n + 3) / 4), "allocating the hit records");
    float *const d_o = ctx->d_query_in.p, *const d_d = d_o + floats, *const d_t = d_d + floats;
    rt_hit *const d_hits = (rt_hit *)ctx->d_query_out.p;
    int32_t *const d_counts = (int32_t *)(ctx->d_query_out.p + records * 3);
    RT_HIP(ctx, hipMemcpy(d_o, origins, floats * 4, hipMemcpyHostToDevice), "copying ray origins");
    RT_HIP(ctx, hipMemcpy(d_d, directions, floats * 4, hipMemcpyHostToDevice), "copying ray directions");
    if (tmax) RT_HIP(ctx, hipMemcpy(d_t, tmax, (size_t)n * 4, hipMemcpyHostToDevice), "copying the limits");
    st = rt_trace_rays_multi_device(ctx, scene, d_o, d_d, tmax ? d_t : nullptr, n, k, d_hits, d_counts, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "multi-hit kernel");
    if (k > 0) RT_HIP(ctx, hipMemcpy(hits, d_hits, records * sizeof(rt_hit), hipMemcpyDeviceToHost), "copying hit records to host");
    if (counts) RT_HIP(ctx, hipMemcpy(counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost), "copying hit counts to host");
    return RT_OK;
}
