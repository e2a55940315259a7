/*
 * rt_query.h — the argument block of the query kernels (rt_query_kernel.h).  Written by rt_query_capi.cpp (its scene, work and view
 * fields by rt_internal.h's ray_args_scene / ray_args_view, which fill the like-named fields of rt_occlusion_args too), read by the
 * kernels.  The scene fields carry the names rt_kernel_args gives them: rt_stage_scene reads either.
 */
#ifndef RT_QUERY_H
#define RT_QUERY_H

#include <stdint.h>

#include "rt_amd.h"
#include "rt_device_scene.h"

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
