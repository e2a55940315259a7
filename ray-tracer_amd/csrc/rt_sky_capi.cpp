/*
 * rt_sky_capi.cpp — environment lighting of the C ABI (include/rt_amd.h): a cube-map sky, and the camera sequences rendered under it.  The
 * kernel is rt_render_kernel.h's rt_sky_kernel (the views kernel whose rays that leave the scene look their light up in the map); the
 * checks, the camera table, the schedule, the launch bracket, the fold and the host form's loop are rt_views_capi.cpp's, called with the sky
 * kernel's launcher; the lookup, its inverse and the map's own checks are rt_sky.h (no HIP: tests/sanitize/sky_host_fuzz.cpp drives them on
 * the host).
 */
#include <cstdint>
#include <vector>

#include "rt_internal.h"
#include "rt_sky.h"

namespace {

/* the sky of a render call: there, and the context's */
rt_status check_sky(rt_ctx *ctx, const rt_sky *sky)
{
    if (!ctx || !sky) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (sky->ctx != ctx) return set_err(ctx, RT_ERR_INVALID, "sky belongs to another context");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_sky_create(rt_ctx *ctx, int32_t face_size, const float *faces_rgb, rt_sky **out)
{
    if (!ctx || !faces_rgb || !out) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (!rt_sky_host::face_size_ok(face_size)) return set_err(ctx, RT_ERR_INVALID, "bad face size (1 .. RT_SKY_MAX_FACE)");
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    std::vector<float> packed(rt_sky_host::device_floats(face_size));
    rt_sky_host::pack(faces_rgb, face_size, packed.data());
    rt_sky *sky = new rt_sky;
    sky->ctx = ctx;
    sky->face_size = face_size;
    hipError_t e = sky->d_texels.grow(packed.size());
    if (e == hipSuccess) e = hipMemcpy(sky->d_texels.p, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete sky;
        return hip_fail(ctx, e, "uploading the sky");
    }
    *out = sky;
    return RT_OK;
}

extern "C" void rt_sky_destroy(rt_sky *sky)
{
    if (!sky) return;
    if (sky->ctx) (void)rt_ctx_synchronize(sky->ctx);       /* a launch in flight may still read the texels */
    delete sky;
}

extern "C" rt_status rt_sky_texel_direction(int32_t face_size, int32_t face, int32_t row, int32_t col, float out[3])
{
    if (rt_sky_host::texel_error(face_size, face, row, col, out)) return RT_ERR_INVALID;
    rt_sky_direction(face_size, face, row, col, out);
    return RT_OK;
}

extern "C" rt_status rt_render_sky_device(rt_ctx *ctx, const rt_scene *scene, const rt_sky *sky, const rt_camera *cams, const int32_t *times_ms, int32_t n_views,
                                          const rt_render_settings *rs, int32_t accumulate, int32_t frame_num, float *d_frames, void *hip_stream)
{
    rt_status st = check_views(ctx, scene, cams, times_ms, n_views, rs, accumulate, frame_num, d_frames, true);
    if (st != RT_OK || (st = check_sky(ctx, sky)) != RT_OK) return st;
    return views_launch(ctx, scene, cams, times_ms, n_views, rs, accumulate, frame_num, d_frames, (hipStream_t)hip_stream,
                        [sky](const rt_kernel_args &a, const float *d_cams, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream) {
                            return rt_launch_sky(&a, d_cams, sky->d_texels.p, sky->face_size, shape, blocks, lds_bytes, stream);
                        });
}

extern "C" rt_status rt_render_sky(rt_ctx *ctx, const rt_scene *scene, const rt_sky *sky, const rt_camera *cams, const int32_t *times_ms, int32_t n_views,
                                   const rt_render_settings *rs, int32_t accumulate, int32_t *frame_num, float *frames)
{
    if (!frame_num) return set_err(ctx, RT_ERR_INVALID, "null argument");
    rt_status st = check_views(ctx, scene, cams, times_ms, n_views, rs, accumulate, *frame_num, frames, false);
    if (st != RT_OK || (st = check_sky(ctx, sky)) != RT_OK) return st;
    return views_host_form(ctx, cams, times_ms, n_views, accumulate, frame_num, frames, [&](const rt_camera *c, const int32_t *t, int32_t k, int32_t fn, float *d) {
        return rt_render_sky_device(ctx, scene, sky, c, t, k, rs, accumulate, fn, d, nullptr);
    });
}
