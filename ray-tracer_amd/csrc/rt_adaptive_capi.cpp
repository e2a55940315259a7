/*
 * rt_adaptive_capi.cpp — per-pixel sample budgets and the adaptive sampling loop of the C ABI (include/rt_amd.h): the budget render's
 * argument checks and launch, the plan's, the driver loop and the host-buffer forms.  The budget kernel is rt_render_kernel.h's
 * rt_budget_kernel, the image-space kernels are rt_adaptive_kernel.h; the parameter checks and a pass's tile list are rt_adaptive.h
 * (no HIP: tests/sanitize/adaptive_host_fuzz.cpp drives them on the host).  The context, the scene, the render kernel's argument block
 * and the launch bracket are rt_capi.cpp's and rt_internal.h's.
 */
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_adaptive.h"
#include "rt_internal.h"

namespace {

rt_status check_budget(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, const rt_tile_spec *t, const void *budget, const void *frame)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!cam || !rs || !budget || !frame) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if ((st = check_image_size(ctx, cam->width, cam->height)) != RT_OK) return st;
    if (rs->reflection_limit < 0) return set_err(ctx, RT_ERR_INVALID, "bad render settings");
    if (!t) return RT_OK;
    if (!t->tile_list) return set_err(ctx, RT_ERR_INVALID, "bad tile spec (a budget render takes the whole image or a tile list, not bands)");
    if (t->compact) return set_err(ctx, RT_ERR_INVALID, "bad tile spec (a budget render writes a full frame: compact must be 0)");
    if (t->tile_cost || t->tile_peak) return set_err(ctx, RT_ERR_INVALID, "bad tile spec (a budget render takes its tiles in list order: no tile_cost / tile_peak)");
    const int tiles_x = (cam->width + 7) / 8, tiles_y = (cam->height + 7) / 8;
    if (const char *bad = rt_sched::tile_spec_error(*t, tiles_x, tiles_y)) return set_err(ctx, RT_ERR_INVALID, bad);
    std::vector<uint32_t> tiles;
    if (!rt_sched::view_tiles(*t, cam->width, cam->height, tiles)) return set_err(ctx, RT_ERR_INVALID, "bad tile spec (a tile index outside the image, or listed twice)");
    return RT_OK;
}

rt_status check_params(rt_ctx *ctx, const rt_adaptive_params *p)
{
    if (!p) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (const char *bad = rt_adaptive::params_error(*p)) return set_err(ctx, RT_ERR_INVALID, bad);
    return RT_OK;
}

/* One budget launch on `stream` in the context's launch bracket, after the checks.  d_list: the tile list on the device (n_list tiles), or
 * NULL for the whole image. */
rt_status launch_budget(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, int32_t time_ms, const uint32_t *d_list, int n_list,
                        const uint16_t *d_budget, uint32_t *d_count, float *d_frame, hipStream_t stream)
{
    rt_tile_spec spec = rt_sched::whole_image_spec();
    uint32_t placeholder = 0;
    if (d_list) { spec.tile_list = &placeholder; spec.num_tiles = n_list; }       /* (the layout reads the list's presence and length only) */
    const rt_sched::Layout L(spec, cam->width, cam->height);
    rt_render_settings one = *rs;
    one.rays_per_pixel = 0;                                   /* not read by the budget kernel */
    rt_kernel_args a = kernel_args(ctx, scene, cam, &one, &time_ms, 1, 0, L, nullptr, d_frame, ctx->tile_counter.p);
    a.tile_list = d_list;
    if (d_list) a.tile_stride = 1;                            /* ticket t is the list's tile t: the caller's order */
    if (a.num_tiles <= 0) return launch_bracket(ctx, stream, []() -> rt_status { return RT_OK; });
    return launch_bracket(ctx, stream, [&]() -> rt_status {
        RT_HIP(ctx, hipMemsetAsync(a.tile_counter, 0, 512, stream), "clearing tile counter");
        RT_HIP(ctx, rt_launch_budget(&a, d_budget, d_count, scene->kernel.shape, launch_blocks(ctx, scene, a.num_tiles), scene->kernel.lds_bytes, stream),
               "launching budget render kernel");
        return RT_OK;
    });
}

rt_plan_args plan_args(int32_t width, int32_t height, const float *d_a, const float *d_b, const uint32_t *d_count, const rt_adaptive_params *p, uint16_t *d_budget,
                       float *d_tile_error, uint32_t *d_tile_active)
{
    rt_plan_args a;
    std::memset(&a, 0, sizeof a);
    a.a = d_a; a.b = d_b; a.count = d_count;
    a.budget = d_budget; a.tile_error = d_tile_error; a.tile_active = d_tile_active;
    a.width = width; a.height = height;
    a.tiles_x = (width + 7) / 8;
    a.num_tiles = a.tiles_x * ((height + 7) / 8);
    a.threshold = p->threshold; a.pixel_threshold = p->pixel_threshold; a.floor = p->floor;
    a.step_spp = (uint32_t)p->step_spp; a.max_spp = (uint32_t)p->max_spp;
    return a;
}

/* a uint16 plane filled with one value on `stream` */
rt_status fill_u16(rt_ctx *ctx, uint16_t *d, uint16_t value, size_t n, hipStream_t stream)
{
    RT_HIP(ctx, hipMemsetD16Async((hipDeviceptr_t)d, value, n, stream), "filling the budget plane");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_render_budget_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                             int32_t time_ms, const rt_tile_spec *tiles, const uint16_t *d_budget, uint32_t *d_count,
                                             float *d_frame, void *hip_stream)
{
    rt_status st = check_budget(ctx, scene, cam, rs, tiles, d_budget, d_frame);
    if (st != RT_OK) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const uint32_t *d_list = nullptr;
    int n_list = 0;
    if (tiles) {
        n_list = tiles->num_tiles;
        if (n_list == 0) return launch_bracket(ctx, stream, []() -> rt_status { return RT_OK; });      /* an empty list: nothing to render */
        if ((st = ctx->tile_lists.on_device(ctx, tiles->tile_list, n_list, stream, &d_list)) != RT_OK) return st;
    }
    return launch_budget(ctx, scene, cam, rs, time_ms, d_list, n_list, d_budget, d_count, d_frame, stream);
}

extern "C" rt_status rt_render_budget(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs,
                                      int32_t time_ms, const rt_tile_spec *tiles, const uint16_t *budget, uint32_t *count, float *frame)
{
    rt_status st = check_budget(ctx, scene, cam, rs, tiles, budget, frame);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the context's adaptive buffers: the frame in A's place, the count in the first count plane */
    const size_t px = (size_t)cam->width * (size_t)cam->height;
    RT_HIP(ctx, ctx->d_adaptive_ab.grow(6 * px), "allocating the frame");
    RT_HIP(ctx, ctx->d_adaptive_count.grow(2 * px), "allocating the count plane");
    RT_HIP(ctx, ctx->d_adaptive_budget.grow(px), "allocating the budget plane");
    RT_HIP(ctx, hipMemcpy(ctx->d_adaptive_ab.p, frame, px * 12, hipMemcpyHostToDevice), "copying the frame to the device");
    if (count) RT_HIP(ctx, hipMemcpy(ctx->d_adaptive_count.p, count, px * 4, hipMemcpyHostToDevice), "copying the counts to the device");
    RT_HIP(ctx, hipMemcpy(ctx->d_adaptive_budget.p, budget, px * 2, hipMemcpyHostToDevice), "copying the budgets to the device");
    st = rt_render_budget_device(ctx, scene, cam, rs, time_ms, tiles, ctx->d_adaptive_budget.p, count ? ctx->d_adaptive_count.p : nullptr, ctx->d_adaptive_ab.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "budget render kernel");
    RT_HIP(ctx, hipMemcpy(frame, ctx->d_adaptive_ab.p, px * 12, hipMemcpyDeviceToHost), "copying the frame to host");
    if (count) RT_HIP(ctx, hipMemcpy(count, ctx->d_adaptive_count.p, px * 4, hipMemcpyDeviceToHost), "copying the counts to host");
    return RT_OK;
}

extern "C" void rt_adaptive_params_default(rt_adaptive_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->pilot_spp = 8;
    p->step_spp = 16;
    p->max_spp = 512;
    p->max_passes = 16;
    p->threshold = 0.05f;
    p->pixel_threshold = std::numeric_limits<float>::infinity();
    p->floor = 0.01f;
}

extern "C" rt_status rt_adaptive_plan_device(rt_ctx *ctx, int32_t width, int32_t height, const float *d_a, const float *d_b, const uint32_t *d_count,
                                             const rt_adaptive_params *params, uint16_t *d_budget, float *d_tile_error, uint32_t *d_tile_active,
                                             void *hip_stream)
{
    if (!ctx) return RT_ERR_INVALID;
    if (!d_a || !d_b || !d_count || !params || !d_budget || !d_tile_error || !d_tile_active) return set_err(ctx, RT_ERR_INVALID, "null argument");
    rt_status st = check_image_size(ctx, width, height);
    if (st != RT_OK) return st;
    if ((st = check_params(ctx, params)) != RT_OK) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    const rt_plan_args a = plan_args(width, height, d_a, d_b, d_count, params, d_budget, d_tile_error, d_tile_active);
    return launch_bracket(ctx, stream, [&]() -> rt_status {
        RT_HIP(ctx, rt_launch_adaptive_plan(&a, stream), "launching the plan kernel");
        return RT_OK;
    });
}

extern "C" rt_status rt_render_adaptive(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, int32_t time_ms,
                                        const rt_adaptive_params *params, float *d_frame, uint32_t *d_count, rt_adaptive_stats *stats,
                                        void *hip_stream)
{
    uint16_t not_null = 0;                                    /* (the budget plane is the context's) */
    rt_status st = check_budget(ctx, scene, cam, rs, nullptr, &not_null, d_frame);
    if (st != RT_OK) return st;
    if ((st = check_params(ctx, params)) != RT_OK) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const int W = cam->width, H = cam->height;
    const size_t px = (size_t)W * (size_t)H;
    const int num_tiles = ((W + 7) / 8) * ((H + 7) / 8);
    RT_HIP(ctx, ctx->d_adaptive_ab.grow(6 * px), "allocating the half buffers");
    RT_HIP(ctx, ctx->d_adaptive_count.grow(2 * px), "allocating the count planes");
    RT_HIP(ctx, ctx->d_adaptive_budget.grow(px), "allocating the budget plane");
    RT_HIP(ctx, ctx->d_adaptive_tiles.grow(3 * (size_t)num_tiles), "allocating the tile planes");
    float *const d_a = ctx->d_adaptive_ab.p, *const d_b = d_a + 3 * px;
    uint32_t *const d_count_a = ctx->d_adaptive_count.p, *const d_count_b = d_count_a + px;
    uint16_t *const d_budget = ctx->d_adaptive_budget.p;
    float *const d_tile_error = (float *)ctx->d_adaptive_tiles.p;
    uint32_t *const d_tile_active = ctx->d_adaptive_tiles.p + num_tiles, *const d_list = ctx->d_adaptive_tiles.p + 2 * (size_t)num_tiles;
    rt_adaptive_stats s;
    std::memset(&s, 0, sizeof s);

    /* pass 0: the pilot.  The counts start at 0, so the half buffers' old content is not read */
    RT_HIP(ctx, hipMemsetAsync(d_count_a, 0, 2 * px * 4, stream), "clearing the count planes");
    if ((st = fill_u16(ctx, d_budget, (uint16_t)params->pilot_spp, px, stream)) != RT_OK) return st;
    const uint32_t t0 = (uint32_t)time_ms;
    if ((st = launch_budget(ctx, scene, cam, rs, (int32_t)t0, nullptr, 0, d_budget, d_count_a, d_a, stream)) != RT_OK) return st;
    if ((st = launch_budget(ctx, scene, cam, rs, (int32_t)(t0 + 1u), nullptr, 0, d_budget, d_count_b, d_b, stream)) != RT_OK) return st;

    const rt_plan_args pa = plan_args(W, H, d_a, d_b, d_count_a, params, d_budget, d_tile_error, d_tile_active);
    std::vector<float> tile_error((size_t)num_tiles);
    std::vector<uint32_t> tile_active((size_t)num_tiles), list;
    for (int k = 1; k <= params->max_passes; k++) {
        if ((st = launch_bracket(ctx, stream, [&]() -> rt_status {
                RT_HIP(ctx, rt_launch_adaptive_plan(&pa, stream), "launching the plan kernel");
                return RT_OK;
            })) != RT_OK) return st;
        /* the two per-tile planes in one copy (they lie one after the other); the wait is the loop's one synchronisation per pass */
        RT_HIP(ctx, hipMemcpyAsync(tile_error.data(), d_tile_error, (size_t)num_tiles * 4, hipMemcpyDeviceToHost, stream), "reading the tile errors");
        RT_HIP(ctx, hipMemcpyAsync(tile_active.data(), d_tile_active, (size_t)num_tiles * 4, hipMemcpyDeviceToHost, stream), "reading the active tiles");
        RT_HIP(ctx, hipStreamSynchronize(stream), "waiting for the plan");
        rt_adaptive::build_tile_list(tile_error.data(), tile_active.data(), num_tiles, list);
        if (list.empty()) break;
        /* (the previous pass's launches, which read the list's buffer, are done: the stream was synchronised) */
        RT_HIP(ctx, hipMemcpyAsync(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, stream), "uploading the tile list");
        if ((st = launch_budget(ctx, scene, cam, rs, (int32_t)(t0 + 2u * (uint32_t)k), d_list, (int)list.size(), d_budget, d_count_a, d_a, stream)) != RT_OK) return st;
        if ((st = launch_budget(ctx, scene, cam, rs, (int32_t)(t0 + 2u * (uint32_t)k + 1u), d_list, (int)list.size(), d_budget, d_count_b, d_b, stream)) != RT_OK) return st;
        s.active_tiles[k - 1] = (int32_t)list.size();
        s.passes = k;
    }
    if ((st = launch_bracket(ctx, stream, [&]() -> rt_status {
            RT_HIP(ctx, rt_launch_adaptive_combine(d_a, d_b, d_count_a, d_frame, d_count, (long long)px, stream), "launching the combine kernel");
            return RT_OK;
        })) != RT_OK) return st;
    /* the total from the count plane (the host has no other copy of it) */
    std::vector<uint32_t> counts(px);
    RT_HIP(ctx, hipMemcpyAsync(counts.data(), d_count_a, px * 4, hipMemcpyDeviceToHost, stream), "reading the counts");
    RT_HIP(ctx, hipStreamSynchronize(stream), "waiting for the frame");
    for (uint32_t c : counts) s.total_samples += 2ull * c;
    if (stats) *stats = s;
    return RT_OK;
}

extern "C" rt_status rt_render_adaptive_host(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const rt_render_settings *rs, int32_t time_ms,
                                             const rt_adaptive_params *params, float *frame, uint32_t *count, rt_adaptive_stats *stats)
{
    uint16_t not_null = 0;
    rt_status st = check_budget(ctx, scene, cam, rs, nullptr, &not_null, frame);
    if (st != RT_OK) return st;
    if ((st = check_params(ctx, params)) != RT_OK) return st;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    /* the outputs in the context's plane buffer: the frame, then the counts */
    const size_t px = (size_t)cam->width * (size_t)cam->height;
    RT_HIP(ctx, ctx->d_query_out.grow((px * 16 + sizeof(rt_f4) - 1) / sizeof(rt_f4)), "allocating the result");
    float *d_frame = (float *)ctx->d_query_out.p;
    uint32_t *d_count = (uint32_t *)(d_frame + 3 * px);
    st = rt_render_adaptive(ctx, scene, cam, rs, time_ms, params, d_frame, count ? d_count : nullptr, stats, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipMemcpy(frame, d_frame, px * 12, hipMemcpyDeviceToHost), "copying the frame to host");
    if (count) RT_HIP(ctx, hipMemcpy(count, d_count, px * 4, hipMemcpyDeviceToHost), "copying the counts to host");
    return RT_OK;
}
