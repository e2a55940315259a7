/*
 * rt_overlap_capi.cpp — the box-overlap queries of the C ABI (include/rt_amd.h): argument checks, the launch, the host-buffer form.  The
 * kernel is rt_overlap_kernel.h, the tests, the id buffer and the walk rt_overlap.h; the context and the scene are rt_capi.cpp's, and the
 * checks, the argument block's shared part and the launch (in the context's launch order, between its timing events) are rt_internal.h's.
 */
#include <cstdint>

#include "rt_internal.h"
#include "rt_overlap.h"

namespace {

/* n boxes on a scene, k ids each and where the answers go (each output may be missing, not all of them) */
rt_status check_overlap(rt_ctx *ctx, const rt_scene *scene, const void *lo, const void *hi, int64_t n, int32_t k, const void *ids, const void *counts, const void *any)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (n < 0 || n > RT_OVERLAP_MAX_BOXES) return set_err(ctx, RT_ERR_INVALID, "bad box count (0 .. 2^30)");
    if (k < 0 || k > RT_OVERLAP_MAX) return set_err(ctx, RT_ERR_INVALID, "bad id count per box (0 .. RT_OVERLAP_MAX)");
    if (n == 0) return RT_OK;          /* nothing to do: nothing is looked at */
    if (!lo || !hi) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (k > 0 && !ids) return set_err(ctx, RT_ERR_INVALID, "null ids while k > 0");
    if (k == 0 && !counts && !any) return set_err(ctx, RT_ERR_INVALID, "no output asked for");
    if (scene->flat.objects.size() > RT_MH_MAX_OBJECTS) return set_err(ctx, RT_ERR_INVALID, "scene has too many objects for a box-overlap query (at most 4096)");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_overlap_boxes_device(rt_ctx *ctx, const rt_scene *scene, const float *d_lo, const float *d_hi, int64_t n, int32_t k,
                                             rt_overlap_id *d_ids, int32_t *d_counts, uint8_t *d_any, void *hip_stream)
{
    const rt_status st = check_overlap(ctx, scene, d_lo, d_hi, n, k, d_ids, d_counts, d_any);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    if (k > 0 && ((uintptr_t)d_ids & 7u)) return set_err(ctx, RT_ERR_INVALID, "d_ids must be 8-byte aligned");      /* (device memory: the kernel stores whole records) */
    rt_overlap_args a = ray_args_scene<rt_overlap_args>(ctx, scene, (uint32_t)n);
    a.lo = d_lo;
    a.hi = d_hi;
    a.ids = k > 0 ? d_ids : nullptr;
    a.counts = d_counts;
    a.any = d_any;
    a.k = k;
    a.any_only = (k == 0 && !d_counts) ? 1 : 0;
    return launch_rays(ctx, scene, a, rt_launch_overlap, false, "launching box-overlap kernel", (hipStream_t)hip_stream);
}

extern "C" rt_status rt_overlap_boxes(rt_ctx *ctx, const rt_scene *scene, const float *lo, const float *hi, int64_t n, int32_t k, rt_overlap_id *ids,
                                      int32_t *counts, uint8_t *any)
{
    rt_status st = check_overlap(ctx, scene, lo, hi, n, k, ids, counts, any);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3, records = (size_t)n * (size_t)k;
    /* in: lo, hi; out, in 16-byte units: the ids (8 bytes each), then the counts (n int32), then the bytes (n) */
    const size_t id_units = (records + 1) / 2, count_units = ((size_t)n + 3) / 4, any_units = ((size_t)n + 15) / 16;
    RT_HIP(ctx, ctx->d_query_in.grow(2 * floats), "allocating the boxes");
    RT_HIP(ctx, ctx->d_query_out.grow(id_units + count_units + any_units), "allocating the answers");
    float *const d_lo = ctx->d_query_in.p, *const d_hi = d_lo + floats;
    rt_overlap_id *const d_ids = (rt_overlap_id *)ctx->d_query_out.p;
    int32_t *const d_counts = (int32_t *)(ctx->d_query_out.p + id_units);
    uint8_t *const d_any = (uint8_t *)(ctx->d_query_out.p + id_units + count_units);
    RT_HIP(ctx, hipMemcpy(d_lo, lo, floats * 4, hipMemcpyHostToDevice), "copying the boxes' lower corners");
    RT_HIP(ctx, hipMemcpy(d_hi, hi, floats * 4, hipMemcpyHostToDevice), "copying the boxes' upper corners");
    st = rt_overlap_boxes_device(ctx, scene, d_lo, d_hi, n, k, k > 0 ? d_ids : nullptr, counts ? d_counts : nullptr, any ? d_any : nullptr, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "box-overlap kernel");
    if (k > 0) RT_HIP(ctx, hipMemcpy(ids, d_ids, records * sizeof(rt_overlap_id), hipMemcpyDeviceToHost), "copying the ids to host");
    if (counts) RT_HIP(ctx, hipMemcpy(counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost), "copying the counts to host");
    if (any) RT_HIP(ctx, hipMemcpy(any, d_any, (size_t)n, hipMemcpyDeviceToHost), "copying the bytes to host");
    return RT_OK;
}
