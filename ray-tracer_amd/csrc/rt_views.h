/*
 * rt_views.h — what the camera-sequence entry points (rt_views_capi.cpp) share with the host-only sanitizer program
 * (tests/sanitize/views_host_fuzz.cpp): the argument checks, the chunking of the host form and the thin-lens camera.  Plain functions of
 * scalars and PODs; no HIP.  include/rt_amd.h has the definitions; the launch's schedule is rt_sched::views_job_order (rt_schedule.h).
 */
#ifndef RT_VIEWS_H
#define RT_VIEWS_H

#include <stdint.h>

#include <cmath>
#include <limits>

#include "rt_amd.h"

namespace rt_views {

/* What is wrong with a call's arguments beyond its pointers, its scene and its image size (nullptr: nothing).  max_views: what one call
 * takes (the device form: launch_cap; the host form: no limit, INT32_MAX). */
inline const char *args_error(const rt_camera *cams, int32_t n_views, int32_t max_views, const rt_render_settings &rs, int32_t accumulate, int32_t frame_num)
{
    if (n_views < 1 || n_views > max_views) return "bad number of views (1 .. RT_VIEWS_MAX in one launch, at most rt_max_batch_frames when accumulating)";
    if (frame_num < 0 || frame_num > std::numeric_limits<int32_t>::max() - n_views) return "bad frame number";
    if (!accumulate && frame_num != 0) return "bad frame number (separate frames are frame 0: frame_num must be 0 without accumulate)";
    if (rs.rays_per_pixel < 0 || rs.reflection_limit < 0) return "bad render settings";
    for (int32_t i = 1; i < n_views; i++)
        if (cams[i].width != cams[0].width || cams[i].height != cams[0].height) return "the cameras of a sequence must share one image size";
    return nullptr;
}

/* how many views one launch takes: RT_VIEWS_MAX, and when accumulating (one plane of per-pixel means per view in the context's scratch)
 * at most what rt_max_batch_frames allows for the image (batch_frames) */
inline int32_t launch_cap(int32_t accumulate, int32_t batch_frames)
{
    return accumulate && batch_frames < RT_VIEWS_MAX ? (batch_frames < 1 ? 1 : batch_frames) : RT_VIEWS_MAX;
}

/* the host form's next launch: how many of the n_views - done views left it renders */
inline int32_t next_chunk(int32_t n_views, int32_t done, int32_t cap)
{
    return n_views - done < cap ? n_views - done : cap;
}

/* rt_camera_lens (include/rt_amd.h has the definition: binary32, every operation rounded once, in this order; built with
 * -ffp-contract=off like everything else).  false: an argument the definition refuses.  out may be cam. */
inline bool camera_lens(const rt_camera &cam, float focal_len, float focus_dist, float lens_u, float lens_v, rt_camera &out)
{
    if (!(focal_len > 0.0f) || std::isinf(focal_len) || !(focus_dist > 0.0f) || std::isinf(focus_dist)) return false;
    if (!std::isfinite(lens_u) || !std::isfinite(lens_v)) return false;
    const float *du = cam.delta_u, *dv = cam.delta_v;
    const float lu = sqrtf((du[0] * du[0] + du[1] * du[1]) + du[2] * du[2]), lv = sqrtf((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]);
    if (lu == 0.0f || lv == 0.0f) return false;
    const float s = focus_dist / focal_len;
    const float ru = 1.0f / lu, rv = 1.0f / lv;
    rt_camera r = cam;
    for (int k = 0; k < 3; k++) {
        r.delta_u[k] = du[k] * s;
        r.delta_v[k] = dv[k] * s;
        const float arm = (cam.tl_pixel_pos[k] - cam.cam_pos[k]) * s;
        r.tl_pixel_pos[k] = arm + cam.cam_pos[k];
        const float eu = du[k] * ru, ev = dv[k] * rv;
        const float a = eu * lens_u, b = ev * lens_v;
        const float off = a + b;
        r.cam_pos[k] = off + cam.cam_pos[k];
    }
    out = r;
    return true;
}

}  // namespace rt_views

#endif
