/*
 * rt_query.h — the argument block of the query kernels (rt_query_kernel.h) and the list of their built shapes.  Written by
 * rt_query_capi.cpp, read by the kernels.  The scene fields carry the names rt_kernel_args gives them: rt_stage_scene reads either.
 */
#ifndef RT_QUERY_H
#define RT_QUERY_H

#include <stdint.h>

#include "rt_amd.h"
#include "rt_device_scene.h"

/* The shapes rt_query_kernel<threads, has_mesh, mode, aov> is built for, each with and without the AOV front.  A committed scene's
 * shape (rt_sched::choose_shape) fixes a placement, a workgroup size and an LDS size that fit the blob plus the [entries + 1][threads]
 * traversal stack, which is all the query kernel needs too: the list is the render kernel's, so a scene that renders answers queries. */
inline constexpr rt_shape RT_QUERY_SHAPES[] = {
    {0, RT_SCENE_LDS, 256}, {0, RT_SCENE_LDS, 512}, {0, RT_SCENE_LDS, 768}, {0, RT_SCENE_LDS, 1024},
    {1, RT_SCENE_LDS, 1024}, {1, RT_SCENE_LDS, 768}, {1, RT_SCENE_LDS, 512}, {1, RT_SCENE_LDS, 256},
    {1, RT_SCENE_HYBRID, 1024}, {1, RT_SCENE_HYBRID, 768}, {1, RT_SCENE_HYBRID, 512},
    {0, RT_SCENE_GLOBAL, 256}, {1, RT_SCENE_GLOBAL, 1024},
};
inline constexpr int rt_query_shape_index(rt_shape s)
{
    for (int i = 0; i < (int)(sizeof RT_QUERY_SHAPES / sizeof RT_QUERY_SHAPES[0]); i++)
        if (RT_QUERY_SHAPES[i] == s) return i;
    return -1;
}
inline constexpr bool rt_query_shapes_cover_render()
{
    for (const rt_shape &s : RT_SHAPES)
        if (rt_query_shape_index(s) < 0) return false;
    return true;
}
static_assert(rt_query_shapes_cover_render(), "every render shape needs its query kernels");

#define RT_QUERY_MAX_RAYS (1 << 30)      /* rays of one call (ray ids and the chunk counter are 32-bit) */

typedef struct {
    /* scene (as in rt_kernel_args) */
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;
    const float *tri_uv;
    const float *tex_data;
    /* the work: rays [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    /* ray queries */
    const float *origins, *directions;   /* n x 3 floats each */
    rt_hit *hits;                        /* n records, 16-byte aligned */
    /* AOV pass: a chunk is the 8x8 tile ty * tiles_x + tx of the image (n = 64 * tiles; slots outside the image are skipped); planes are indexed by
     * pixel, py * width + px; a NULL plane is not written */
    float cam[12];                       /* cam_pos, tl_pixel_pos, delta_u, delta_v */
    int32_t width, height, tiles_x;
    float sky[3];
    float *depth, *normal, *albedo, *ray;
    int32_t *object;
} rt_query_args;

#endif
