/*
 * rt_occlusion_capi.cpp — the occlusion (any-hit) ray queries and the light-visibility plane of the C ABI (include/rt_amd.h): argument
 * checks, the context's launch ordering and timing, the host-buffer forms.  The kernels are rt_occlusion_kernel.h; the context and the
 * scene are rt_capi.cpp's (rt_internal.h).  The rules are rt_query_capi.cpp's, entry for entry.
 */
#include <cstdint>
#include <cstring>

#include "rt_internal.h"
#include "rt_occlusion.h"

extern "C" hipError_t rt_launch_occlusion(const rt_occlusion_args *args, rt_shape shape, int vis, int num_cus, size_t lds_bytes, hipStream_t stream);

namespace {

rt_occlusion_args scene_args(const rt_ctx *ctx, const rt_scene *scene, uint32_t n)
{
    rt_occlusion_args a;
    std::memset(&a, 0, sizeof a);
    a.blob = scene->d_blob.p;
    a.blob_f4 = (int32_t)scene->flat.blob.size();
    a.off_nodes = scene->flat.off_nodes;
    a.off_tris = scene->flat.off_tris;
    a.off_objlds = scene->flat.off_objlds;
    a.off_meshes = scene->flat.off_meshes;
    a.off_objtab = scene->flat.off_objtab;
    a.num_objects = (int32_t)scene->flat.objects.size();
    a.num_meshes = scene->flat.num_meshes;
    a.descend_keep = ctx->descend_keep;
    a.n = n;
    a.num_chunks = (n + 63u) / 64u;
    a.counter = ctx->tile_counter;
    return a;
}

/* One occlusion launch on `stream`, in the context's launch order (the ticket counter is shared with the render and query launches) and
 * between its timing events, as launch_query does it (rt_query_capi.cpp). */
rt_status launch_occlusion(rt_ctx *ctx, const rt_scene *scene, const rt_occlusion_args &a, bool vis, hipStream_t stream)
{
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    if (ctx->launched && ctx->last_stream != stream) RT_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_stop, 0), "ordering the launch behind the previous one");
    for (FrameSlot &fs : ctx->pipe.slots)
        if (fs.used) RT_HIP(ctx, hipStreamWaitEvent(stream, fs.ev_done, 0), "ordering the launch behind the frames in flight");
    RT_HIP(ctx, hipEventRecord(ctx->ev_start, stream), "recording start event");
    ctx->have_timing = false;
    RT_HIP(ctx, hipMemsetAsync(a.counter, 0, 512, stream), "clearing the ray counter");
    RT_HIP(ctx, rt_launch_occlusion(&a, scene->kernel.shape, vis ? 1 : 0, ctx->num_cus, scene->kernel.lds_bytes, stream), "launching occlusion kernel");
    RT_HIP(ctx, hipEventRecord(ctx->ev_stop, stream), "recording stop event");
    ctx->have_timing = true;
    ctx->launched = true;
    ctx->last_stream = stream;
    return RT_OK;
}

rt_status check_scene(rt_ctx *ctx, const rt_scene *scene)
{
    if (!ctx || !scene) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (scene->ctx != ctx) return set_err(ctx, RT_ERR_INVALID, "scene belongs to another context");
    return RT_OK;
}

rt_status check_rays(rt_ctx *ctx, const rt_scene *scene, const void *origins, const void *directions, int64_t n, const void *occluded)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (n < 0 || n > RT_QUERY_MAX_RAYS) return set_err(ctx, RT_ERR_INVALID, "bad ray count (0 .. 2^30)");
    if (n > 0 && (!origins || !directions || !occluded)) return set_err(ctx, RT_ERR_INVALID, "null argument");
    return RT_OK;
}

rt_status check_visibility(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float *light_pos, const void *visibility)
{
    rt_status st = check_scene(ctx, scene);
    if (st != RT_OK) return st;
    if (!cam || !light_pos || !visibility) return set_err(ctx, RT_ERR_INVALID, "null argument");
    if (cam->width <= 0 || cam->height <= 0 || cam->width > 32768 || cam->height > 32768 || (int64_t)cam->width * cam->height > (1 << 28))
        return set_err(ctx, RT_ERR_INVALID, "bad image size (at most 32768 pixels on a side and 2^28 in all)");
    return RT_OK;
}

}  // namespace

extern "C" rt_status rt_occluded_rays_device(rt_ctx *ctx, const rt_scene *scene, const float *d_origins, const float *d_directions,
                                             const float *d_tmax, int64_t n, uint8_t *d_occluded, void *hip_stream)
{
    rt_status st = check_rays(ctx, scene, d_origins, d_directions, n, d_occluded);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    rt_occlusion_args a = scene_args(ctx, scene, (uint32_t)n);
    a.origins = d_origins;
    a.directions = d_directions;
    a.tmax = d_tmax;
    a.out = d_occluded;
    return launch_occlusion(ctx, scene, a, false, (hipStream_t)hip_stream);
}

extern "C" rt_status rt_occluded_rays(rt_ctx *ctx, const rt_scene *scene, const float *origins, const float *directions, const float *tmax,
                                      int64_t n, uint8_t *occluded)
{
    rt_status st = check_rays(ctx, scene, origins, directions, n, occluded);
    if (st != RT_OK) return st;
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t floats = (size_t)n * 3;
    RT_HIP(ctx, ctx->d_query_in.grow(2 * floats + (size_t)n), "allocating the rays");
    RT_HIP(ctx, ctx->d_query_out.grow(((size_t)n + sizeof(rt_f4) - 1) / sizeof(rt_f4)), "allocating the answers");
    float *d_o = ctx->d_query_in.p, *d_d = d_o + floats, *d_t = tmax ? d_d + floats : nullptr;
    RT_HIP(ctx, hipMemcpy(d_o, origins, floats * 4, hipMemcpyHostToDevice), "copying ray origins");
    RT_HIP(ctx, hipMemcpy(d_d, directions, floats * 4, hipMemcpyHostToDevice), "copying ray directions");
    if (tmax) RT_HIP(ctx, hipMemcpy(d_t, tmax, (size_t)n * 4, hipMemcpyHostToDevice), "copying ray limits");
    st = rt_occluded_rays_device(ctx, scene, d_o, d_d, d_t, n, (uint8_t *)ctx->d_query_out.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "occlusion kernel");
    RT_HIP(ctx, hipMemcpy(occluded, ctx->d_query_out.p, (size_t)n, hipMemcpyDeviceToHost), "copying the answers to host");
    return RT_OK;
}

extern "C" rt_status rt_render_visibility_device(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float light_pos[3], float bias,
                                                 uint8_t *d_visibility, void *hip_stream)
{
    rt_status st = check_visibility(ctx, scene, cam, light_pos, d_visibility);
    if (st != RT_OK) return st;
    const int tiles_x = (cam->width + 7) / 8, tiles_y = (cam->height + 7) / 8;          /* (at most 2^22 tiles: check_visibility) */
    rt_occlusion_args a = scene_args(ctx, scene, (uint32_t)tiles_x * (uint32_t)tiles_y * 64u);
    a.tiles_x = tiles_x;
    std::memcpy(a.cam + 0, cam->cam_pos, 12);
    std::memcpy(a.cam + 3, cam->tl_pixel_pos, 12);
    std::memcpy(a.cam + 6, cam->delta_u, 12);
    std::memcpy(a.cam + 9, cam->delta_v, 12);
    a.width = cam->width;
    a.height = cam->height;
    std::memcpy(a.light, light_pos, 12);
    a.bias = bias;
    a.out = d_visibility;
    return launch_occlusion(ctx, scene, a, true, (hipStream_t)hip_stream);
}

extern "C" rt_status rt_render_visibility(rt_ctx *ctx, const rt_scene *scene, const rt_camera *cam, const float light_pos[3], float bias,
                                          uint8_t *visibility)
{
    rt_status st = check_visibility(ctx, scene, cam, light_pos, visibility);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipSetDevice(ctx->device), "selecting device");
    const size_t px = (size_t)cam->width * (size_t)cam->height;
    RT_HIP(ctx, ctx->d_query_out.grow((px + sizeof(rt_f4) - 1) / sizeof(rt_f4)), "allocating the plane");
    st = rt_render_visibility_device(ctx, scene, cam, light_pos, bias, (uint8_t *)ctx->d_query_out.p, nullptr);
    if (st != RT_OK) return st;
    RT_HIP(ctx, hipDeviceSynchronize(), "occlusion kernel");
    RT_HIP(ctx, hipMemcpy(visibility, ctx->d_query_out.p, px, hipMemcpyDeviceToHost), "copying the plane to host");
    return RT_OK;
}
