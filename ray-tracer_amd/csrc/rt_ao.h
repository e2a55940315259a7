/*
 * rt_ao.h — the argument block of the ambient-occlusion kernels (rt_ao_kernel.h).  Written by rt_ao_capi.cpp, read by the kernels.  The
 * scene and view fields carry the names rt_occlusion_args gives them: rt_stage_scene and rt_internal.h's ray_args_view read any of them.
 */
#ifndef RT_AO_H
#define RT_AO_H

#include <stdint.h>

#include "rt_query.h"

typedef struct {
    /* scene (as in rt_kernel_args) */
    const rt_f4 *blob;
    int32_t blob_f4;
    int32_t off_nodes, off_tris, off_objlds, off_meshes, off_objtab;
    int32_t num_objects, num_meshes;
    int32_t descend_keep;
    /* the work: tile slots [0, n) in chunks of 64 (a chunk is the 8x8 tile ty * tiles_x + tx of the image, as in the AOV pass), handed
     * out from `counter` (zeroed before the launch) */
    uint32_t n, num_chunks;
    uint32_t *counter;
    /* per pixel py * width + px: the number of free samples (RT_AO_NO_SURFACE: the primary ray hit nothing) and count / samples;
     * either may be NULL */
    uint16_t *count;
    float *ao;
    float cam[12];                       /* cam_pos, tl_pixel_pos, delta_u, delta_v */
    int32_t width, height, tiles_x;
    int32_t samples;                     /* 1 .. RT_AO_MAX_SAMPLES */
    float radius;                        /* a sample segment's limit, in units of its (unit) direction */
    float bias;
    uint32_t seed;                       /* (uint32)time_ms * 6291469 (src/raytracer.cu:127) */
} rt_ao_args;

#endif
