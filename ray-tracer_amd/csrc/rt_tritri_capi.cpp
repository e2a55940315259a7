/*
 * rt_tritri_capi.cpp — the triangle-overlap queries of the C ABI (include/rt_amd.h): argument checks, the launch, the host-buffer form.
 * The kernel is rt_tritri_kernel.h, the tests and the walk rt_tritri.h, the id buffer rt_overlap.h; the context and the scene are
 * rt_capi.cpp's, and the checks, the argument block's shared part and the launch (in the context's launch order, between its timing
 * events) are rt_internal.h's.
 */
#include <cstdint>

#include "rt_internal.h"
#include "rt_tritri.h"

namespace {

/* n query triangles on a scene, k ids each and where the answers go (each output may be missing, not all of them) */
rt_status check_tritri(rt_ctx *ctx, const rt_scene *scene, const void *tris, int64_t n, int32_t k, const void *ids, const void *counts, const void *any, const void *segments)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (n < 0 || n > RT_TRITRI_MAX_TRIANGLES) return set_err(ctx, RT_ERR_INVALID, "bad triangle count (0 .. 2^30)");
    if (k < 0 || k > RT_OVERLAP_MAX) return set_err(ctx, RT_ERR_INVALID, "bad id count per triangle (0 .. RT_OVERLAP_MAX)");
    if (n == 0) return RT_OK;          /* nothing to do: nothing is looked at */
    if (!tris) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (k > 0 && !ids) return set_err(ctx, RT_ERR_INVALID, "null ids while k > 0");
    if (k == 0 && !counts && !any) return set_err(ctx, RT_ERR_INVALID, "no output asked for");
    if (k == 0 && segments) return set_err(ctx, RT_ERR_INVALID, "segments asked for while k == 0");
    if (scene->flat.objects.size() > RT_MH_MAX_OBJECTS) return set_err(ctx, RT_ERR_INVALID, "scene has too many objects for a triangle-overlap query (at most 4096)");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_overlap_triangles_device(rt_ctx *ctx, const rt_scene *scene, const float *d_tris, int64_t n, int32_t k, rt_overlap_id *d_ids,
                                                 int32_t *d_counts, uint8_t *d_any, rt_tri_segment *d_segments, void *hip_stream)
{
    const rt_status st = check_tritri(ctx, scene, d_tris, n, k, d_ids, d_counts, d_any, d_segments);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    if (k > 0 && ((uintptr_t)d_ids & 7u)) return set_err(ctx, RT_ERR_INVALID, "d_ids must be 8-byte aligned");      /* (device memory: the kernel stores whole records) */
    if ((uintptr_t)d_segments & 15u) return set_err(ctx, RT_ERR_INVALID, "d_segments must be 16-byte aligned");
    rt_tritri_args a = ray_args_scene<rt_tritri_args>(ctx, scene, (uint32_t)n);
    a.tris = d_tris;
    a.ids = k > 0 ? d_ids : nullptr;
    a.counts = d_counts;
    a.any = d_any;
    a.segments = d_segments;
    a.k = k;
    a.any_only = (k == 0 && !d_counts) ? 1 : 0;
    return launch_rays(ctx, scene, a, rt_launch_tritri, false, "launching triangle-overlap kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_overlap_triangles(rt_ctx *ctx, const rt_scene *scene, const float *tris, int64_t n, int32_t k, rt_overlap_id *ids, int32_t *counts,
                                          uint8_t *any, rt_tri_segment *segments)
{
    rt_status st = check_tritri(ctx, scene, tris, n, k, ids, counts, any, segments);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 9, records = (size_t)n * (size_t)k;
    /* in: the triangles; out, in 16-byte units: the segments (two each, first: they are stored as whole units), the ids (8 bytes each),
     * the counts (n int32), the bytes (n) */
    const size_t seg_units = segments ? 2 * records : 0, id_units = (records + 1) / 2, count_units = ((size_t)n + 3) / 4, any_units = ((size_t)n + 15) / 16;
    RT_HIP(ctx, ctx->d_query_in.grow(floats), "allocating the triangles");
    RT_HIP(ctx, ctx->d_query_out.grow(seg_units + id_units + count_units + any_units), "allocating the answers");
    float *const d_tris = ctx->d_query_in.p;
    rt_tri_segment *const d_segments = (rt_tri_segment *)ctx->d_query_out.p;
    rt_overlap_id *const d_ids = (rt_overlap_id *)(ctx->d_query_out.p + seg_units);
    int32_t *const d_counts = (int32_t *)(ctx->d_query_out.p + seg_units + id_units);
    uint8_t *const d_any = (uint8_t *)(ctx->d_query_out.p + seg_units + id_units + count_units);
    RT_HIP(ctx, hipMemcpy(d_tris, tris, floats * 4, hipMemcpyHostToDevice), "copying the triangles");
    st = rt_overlap_triangles_device(ctx, scene, d_tris, n, k, k > 0 ? d_ids : nullptr, counts ? d_counts : nullptr, any ? d_any : nullptr,
                                     segments ? d_segments : nullptr, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "triangle-overlap kernel");
    if (k > 0) RT_HIP(ctx, hipMemcpy(ids, d_ids, records * sizeof(rt_overlap_id), hipMemcpyDeviceToHost), "copying the ids to host");
    if (counts) RT_HIP(ctx, hipMemcpy(counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the counts to host");
    if (any) RT_HIP(ctx, hipMemcpy(any, d_any, (size_t)n, hipMemcpyDeviceToHost), "copying the bytes to host");
    if (segments) RT_HIP(ctx, hipMemcpy(segments, d_segments, records * sizeof(rt_tri_segment), hipMemcpyDeviceToHost), "copying the segments to host");
    return RT_OK;
}
