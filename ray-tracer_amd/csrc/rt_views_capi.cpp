/*
 * rt_views_capi.cpp — camera sequences of the C ABI (include/rt_amd.h): many views of one scene in ONE launch, as separate frames or folded
 * into one progressive frame, and the thin-lens camera that makes the latter a depth-of-field renderer.  The kernel is rt_render_kernel.h's
 * rt_views_kernel (the render kernel with a camera per frame of the launch), the fold is rt_capi.cpp's; the argument checks, the host
 * form's chunking and the lens are rt_views.h, the schedule is rt_sched::views_job_order (neither needs HIP:
 * tests/sanitize/views_host_fuzz.cpp drives them on the host).  The context's cached view (rt_ctx::view) is neither read nor written here.
 * The checks, the launch and the host form's loop are functions of rt_detail (rt_internal.h) taking the kernel's launcher: rt_sky_capi.cpp
 * runs the sky variant through them.
 */
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_internal.h"
#include "rt_views.h"

namespace {

constexpr size_t CAM_WORDS = (size_t)RT_VIEWS_MAX * 12;      /* the camera table's place at the head of ViewsState::d_table */

}  // namespace

namespace rt_detail {

/* device: one launch's limit on the number of views applies (rt_views::launch_cap); the host form takes any number */
rt_status check_views(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms, int32_t n_views, const rt_render_settings *rs,
                      int32_t accumulate, int32_t frame_num, const void *frames, bool device)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!cams || !times_ms || !rs || !frames) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if ((st = check_image_size(ctx, cams[0].width, cams[0].height)) != RT_OK) return st;
    const int32_t cap = device ? rt_views::launch_cap(accumulate, batch_cap(ctx, (size_t)cams[0].width * (size_t)cams[0].height * 3)) : std::numeric_limits<int32_t>::max();
    if (const char *bad = rt_views::args_error(cams, n_views, cap, *rs, accumulate, frame_num)) return set_err(ctx, RT_ERR_INVALID, bad);
    return RT_OK;
}

/* The device form of a views launch whose arguments have passed check_views, with the kernel's launcher the caller's: rt_launch_views here,
 * the sky variant's in rt_sky_capi.cpp (this translation unit references only the former). */
rt_status views_launch(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms, int32_t n_views, const rt_render_settings *rs,
                       int32_t accumulate, int32_t frame_num, float *d_frames, hipStream_t stream, const ViewsLauncher &launcher)
{
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const rt_sched::Layout L(rt_sched::whole_image_spec(), cams[0].width, cams[0].height);
    const size_t plane_floats = L.plane_floats();
    /* one plane of per-pixel means per view: the context's when they are folded into one frame, the caller's frames themselves otherwise */
    if (accumulate) RT_HIP(ctx, ctx->d_partial.grow(plane_floats * (size_t)n_views), "allocating the per-view planes");
    rt_kernel_args a = kernel_args(ctx, scene, &cams[0], rs, times_ms, n_views, frame_num, L, nullptr, d_frames, ctx->tile_counter.p);
    a.partial = accumulate ? ctx->d_partial.p : d_frames;
    a.partial_plane = (int64_t)(plane_floats / 3);

    /* the camera table and, where the order matters (a mesh, more than one tile), the schedule: one buffer, one copy */
    ViewsState &vs = ctx->views;
    if (!vs.ev_up.e) RT_HIP(ctx, hipEventCreateWithFlags(&vs.ev_up.e, hipEventDisableTiming), "creating an event");
    if (vs.uploaded) RT_HIP(ctx, hipEventSynchronize(vs.ev_up), "waiting for the previous camera table's upload");
    std::vector<float> table(12 * (size_t)n_views);
    for (int32_t i = 0; i < n_views; i++) camera_floats(cams[i], table.data() + 12 * (size_t)i);
    vs.host.assign(CAM_WORDS, 0u);
    std::memcpy(vs.host.data(), table.data(), table.size() * 4);
    const bool scheduled = scene->flat.num_meshes > 0 && a.num_tiles > 1;
    if (scheduled) {
        std::vector<uint32_t> jobs;
        rt_sched::views_job_order((uint32_t)a.num_tiles, a.tiles_x, table.data(), (uint32_t)n_views, scene->flat.objects, jobs);
        vs.host.insert(vs.host.end(), jobs.begin(), jobs.end());
    }
    RT_HIP(ctx, vs.d_table.grow(vs.host.size()), "allocating the camera table");
    a.job_order = scheduled ? vs.d_table.p + CAM_WORDS : nullptr;
    const long long jobs_total = (long long)a.num_tiles * n_views;
    const int blocks = launch_blocks(ctx, scene, (int)(jobs_total < (1ll << 30) ? jobs_total : (1ll << 30)));

    return launch_bracket(ctx, stream, [&]() -> rt_status {
        RT_HIP(ctx, hipMemcpyAsync(vs.d_table.p, vs.host.data(), vs.host.size() * 4, hipMemcpyHostToDevice, stream), "uploading the camera table");
        RT_HIP(ctx, hipEventRecord(vs.ev_up, stream), "recording the camera table's upload");
        vs.uploaded = true;
        RT_HIP(ctx, hipMemsetAsync(a.tile_counter, 0, 512, stream), "clearing tile counter");
        RT_HIP(ctx, hipEventRecord(ctx->ev_start, stream), "recording start event");        /* (again: rt_last_kernel_ms starts at the render kernel) */
        RT_HIP(ctx, launcher(a, (const float *)vs.d_table.p, scene->kernel.shape, blocks, scene->kernel.lds_bytes, stream), "launching views kernel");
        if (accumulate) return fold(ctx, L, ctx->d_partial.p, n_views, frame_num, d_frames, nullptr, stream);
        /* separate frames: each plane becomes frame 0 of its view in place - (c + 0 * 0) / 1, a NaN as the canonical quiet NaN - which is
         * the blend of one plane at frame_num 0.  All planes in one pass while a launch can index them, else view by view */
        const long long all = (long long)plane_floats * n_views;
        if (all < (1ll << 31)) {
            RT_HIP(ctx, rt_launch_blend(d_frames, 0, 1, 0, d_frames, all, stream), "launching blend kernel");
        } else {
            for (int32_t i = 0; i < n_views; i++)
                RT_HIP(ctx, rt_launch_blend(d_frames + (size_t)i * plane_floats, 0, 1, 0, d_frames + (size_t)i * plane_floats, (long long)plane_floats, stream),
                       "launching blend kernel");
        }
        return RT_OK;
    });
}

/* The host form over a device form (rt_render_views_device, or the sky's): frames through the context's buffer, in launches of up to the
 * device form's limit.  The arguments have passed check_views' host variant. */
rt_status views_host_form(rt_ctx *ctx, const rt_camera *cams, const int32_t *times_ms, int32_t n_views, int32_t accumulate, int32_t *frame_num, float *frames,
                          const ViewsDeviceForm &device_form)
{
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t frame_floats = (size_t)cams[0].width * (size_t)cams[0].height * 3;
    const int32_t cap = rt_views::launch_cap(accumulate, batch_cap(ctx, frame_floats));
    DevBuf<float> &d = ctx->views.d_frames;
    RT_HIP(ctx, d.grow(accumulate ? frame_floats : frame_floats * (size_t)rt_views::next_chunk(n_views, 0, cap)), "allocating the frames");
    if (accumulate && *frame_num > 0) RT_HIP(ctx, hipMemcpy(d.p, frames, frame_floats * 4, hipMemcpyHostToDevice), "copying previous frame");
    for (int32_t done = 0; done < n_views;) {
        const int32_t k = rt_views::next_chunk(n_views, done, cap);
        const rt_status st = device_form(cams + done, times_ms + done, k, accumulate ? *frame_num + done : 0, d.p);
        if (st != RT_OK) return st;
        if (!accumulate) {
            RT_HIP(ctx, hipDeviceSynchronize(), "views kernel");
            RT_HIP(ctx, hipMemcpy(frames + (size_t)done * frame_floats, d.p, frame_floats * 4 * (size_t)k, hipMemcpyDeviceToHost), "copying frames to host");
        }
        done += k;
    }
    if (accumulate) {
        RT_HIP(ctx, hipDeviceSynchronize(), "views kernel");
        RT_HIP(ctx, hipMemcpy(frames, d.p, frame_floats * 4, hipMemcpyDeviceToHost), "copying frame to host");
        *frame_num += n_views;
    }
    RT_HIP(ctx, hipPeekAtLastError(), "final check after render");
    return RT_OK;
}

}  // namespace rt_detail

extern "C" rt_status rt_render_views_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms, int32_t n_views,
                                            const rt_render_settings *rs, int32_t accumulate, int32_t frame_num, float *d_frames, void *hip_stream)
{
    rt_status st = check_views(ctx, scene, cams, times_ms, n_views, rs, accumulate, frame_num, d_frames, true);
    if (st != RT_OK) return st;
    return views_launch(ctx, scene, cams, times_ms, n_views, rs, accumulate, frame_num, d_frames, (hipStream_t)hip_stream,
                        [](const rt_kernel_args &a, const float *d_cams, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream) {
                            return rt_launch_views(&a, d_cams, shape, blocks, lds_bytes, stream);
                        });
}

extern "C" rt_status rt_render_views(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cams, const int32_t *times_ms, int32_t n_views,
                                     const rt_render_settings *rs, int32_t accumulate, int32_t *frame_num, float *frames)
{
    if (!frame_num) return set_err(ctx, RT_ERR_INVALID, "null argument");
    rt_status st = check_views(ctx, scene, cams, times_ms, n_views, rs, accumulate, *frame_num, frames, false);
    if (st != RT_OK) return st;
    return views_host_form(ctx, cams, times_ms, n_views, accumulate, frame_num, frames, [&](const rt_camera *c, const int32_t *t, int32_t k, int32_t fn, float *d) {
        return rt_render_views_device(ctx, scene, c, t, k, rs, accumulate, fn, d, nullptr);
    });
}

extern "C" rt_status rt_camera_lens(const rt_camera *cam, float focal_len, float focus_dist, float lens_u, float lens_v, rt_camera *out)
{
    if (!cam || !out) return RT_ERR_INVALID;
    return rt_views::camera_lens(*cam, focal_len, focus_dist, lens_u, lens_v, *out) ? RT_OK : RT_ERR_INVALID;
}
