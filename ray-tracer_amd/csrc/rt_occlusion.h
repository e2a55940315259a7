/*
 * rt_occlusion.h — the argument block of the occlusion kernels (rt_occlusion_kernel.h).  Written by rt_occlusion_capi.cpp, read by the
 * kernels.  The scene fields carry the names rt_kernel_args and rt_query_args give them: rt_stage_scene reads any of the three.
 */
#ifndef RT_OCCLUSION_H
#define RT_OCCLUSION_H

#include <stdint.h>

#include "rt_query.h"

typedef struct {
    /* scene (as in rt_kernel_args) */
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;
    /* the work: rays (or tile slots) [0, n) in chunks of 64, handed out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    /* one byte per ray (1 occluded, 0 not) or per pixel (RT_VIS_*), indexed by ray id or py * width + px */
    uint8_t *out;
    /* ray queries: n x 3 floats each; tmax n floats, or NULL = RT_HIT_MISS_T for every ray */
    const float *origins, *directions, *tmax;
    /* visibility plane: a chunk is the 8x8 tile ty * tiles_x + tx of the image, as in the AOV pass (n = 64 * tiles) */
    float cam[12];                       /* cam_pos, tl_pixel_pos, delta_u, delta_v */
    int32_t width, height, tiles_x;
    float light[3];
    float bias;
} rt_occlusion_args;

#endif
