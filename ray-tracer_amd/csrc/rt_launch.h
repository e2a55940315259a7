/*
 * rt_launch.h — the seam between the library's two halves, stated once: the launchers that rt_kernel.hip defines (each in the header of
 * its kernel family) and the translation units behind the C ABI call.  The functions have C linkage, so the linker ties nothing to a
 * signature; the compilers do, because every side includes this header: a kernel header whose definition differs, a caller's leftover
 * declaration, or a stub of the host tests (tests/sanitize/launcher_stubs.h) is a conflicting declaration, an error.
 * tests/test_launch_seam.py keeps declarations out of every other file, and every file that defines a launcher includes this one.
 * Host code: the HIP runtime's API types and the argument blocks.
 */
#ifndef RT_LAUNCH_H
#define RT_LAUNCH_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_adaptive.h"
#include "rt_ao.h"
#include "rt_denoise.h"
#include "rt_device_scene.h"
#include "rt_multihit.h"
#include "rt_nearest.h"
#include "rt_occlusion.h"
#include "rt_overlap.h"
#include "rt_query.h"
#include "rt_rebuild.h"
#include "rt_sweep.h"
#include "rt_tritri.h"
#include "rt_winding.h"

extern "C" {

/* ---- rt_render_kernel.h: the render kernel and its variants, by shape (hipErrorInvalidValue: the shape is not built) ---- */
/* workgroups of this shape of rt_render_kernel that are resident on one CU, as the runtime reports it; 0 if the shape is not built */
int rt_kernel_blocks_per_cu(rt_shape shape, size_t lds_bytes);
hipError_t rt_launch_render(const rt_kernel_args *args, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream);
/* the budget variant: per pixel budget[] samples, count[] updated; the grid is sized as for the render kernel */
hipError_t rt_launch_budget(const rt_kernel_args *args, const uint16_t *budget, uint32_t *count, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream);
/* the views variant: cams is the device table of args->num_frames x 12 camera floats; the grid is sized as for the render kernel */
hipError_t rt_launch_views(const rt_kernel_args *args, const float *cams, rt_shape shape, int blocks, size_t lds_bytes, hipStream_t stream);
/* the sky variant of the views kernel: texels is the map's device copy (RT_SKY_TEXEL_FLOATS per texel, rt_sky.h), face_size its n */
hipError_t rt_launch_sky(const rt_kernel_args *args, const float *cams, const float *texels, int32_t face_size, rt_shape shape, int blocks, size_t lds_bytes,
                         hipStream_t stream);

/* ---- rt_frame_kernels.h ---- */
/* folds num_frames planes of per-pixel means into `frame` in place, in frame order */
hipError_t rt_launch_blend(const float *partial, long long plane_floats, int num_frames, int frame_num, float *frame, long long n_floats, hipStream_t stream);
/* the same fold for the pixels of a list of tiles (planes and frame are full W x H frames) */
hipError_t rt_launch_blend_tiles(const float *partial, long long plane_floats, int num_frames, int frame_num, float *frame,
                                 const uint32_t *tile_list, int n_tiles, int tiles_x, int W, int H, hipStream_t stream);
/* a tile list's compact image <-> the full frame (to_frame: frame[tile pixels] = compact) */
hipError_t rt_launch_tiles_copy(float *compact, float *frame, const uint32_t *tile_list, int n_tiles, int tiles_x, int W, int H, int to_frame, hipStream_t stream);
hipError_t rt_launch_rgba8(const float *rgb, int n_pixels, uint8_t *out, hipStream_t stream);

/* ---- rt_ray_kernels.h: the ray kernels (hipErrorNotSupported in the development builds) ---- */
/* aov, vis: 0 the caller's rays, 1 the pass over a view; every other kernel here has the one front, whatever `front` says: the signature is
 * kept so that rt_internal.h's enqueue_rays serves them all */
hipError_t rt_launch_query(const rt_query_args *args, rt_shape shape, int aov, int num_cus, size_t lds_bytes, hipStream_t stream);
hipError_t rt_launch_occlusion(const rt_occlusion_args *args, rt_shape shape, int vis, int num_cus, size_t lds_bytes, hipStream_t stream);
hipError_t rt_launch_ao(const rt_ao_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream);
/* rt_multihit_kernel.h, with them */
hipError_t rt_launch_multihit(const rt_multihit_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream);
/* ... and its second pass over the records: the texture coordinates of those on a sphere whose material needs them */
hipError_t rt_launch_multihit_uv(const rt_multihit_uv_args *args, int num_cus, hipStream_t stream);
/* rt_overlap_kernel.h and rt_tritri_kernel.h, with them */
hipError_t rt_launch_overlap(const rt_overlap_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream);
hipError_t rt_launch_tritri(const rt_tritri_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream);

/* ---- rt_denoise_kernel.h ---- */
hipError_t rt_launch_denoise_pack(const rt_denoise_args *args, hipStream_t stream);
hipError_t rt_launch_denoise_level(const rt_denoise_args *args, int last, hipStream_t stream);

/* ---- rt_adaptive_kernel.h ---- */
hipError_t rt_launch_adaptive_plan(const rt_plan_args *args, hipStream_t stream);
hipError_t rt_launch_adaptive_combine(const float *a, const float *b, const uint32_t *count, float *frame, uint32_t *count_out, long long n_pixels, hipStream_t stream);

/* ---- rt_rebuild_kernel.h ---- */
/* queues the whole rebuild on `stream`: the global levels (box and keys per segment, the sort's passes, the new list), the workgroup-local
 * levels, the node and root boxes.  Nothing waits; every kernel's loops are bounded by n and the level count. */
hipError_t rt_launch_rebuild(const rt_rebuild_args *args, hipStream_t stream);

/* ---- rt_cull_kernel.h ---- */
/* the pre-pass on `stream` - one thread per pixel of the width x height image of camera `cam`, the scene's blob walked in global memory;
 * writes rt_cull_words(width, height) words of `plane`, a set bit: the pixel's primary rays reach no leaf of any mesh, and behind them a
 * word per pixel, the subtree cull's dead gates (rt_cull.h: `plane` has rt_cull_alloc_words of those words).  view_flags: RT_CULL_ANTIALIAS
 * (the view's rays are jittered) | RT_CULL_WITH_GATES (compute the gate words; without it, or with more than one mesh, every gate word is
 * written as 0) | RT_CULL_WITH_ENTRY (rt_entry.h: compute the entry words behind the gate words - `plane` then has rt_cull_alloc_words_entry
 * words -, of the triangles that start at 16-byte unit view_flags >> RT_CULL_TRIS_SHIFT of the blob; without it, or with more than one mesh,
 * every entry word is written as 0) */
hipError_t rt_launch_cull(const float *cam, int32_t width, int32_t height, int32_t view_flags, const rt_f4 *blob, int32_t off_nodes, int32_t num_nodes,
                          int32_t off_meshes, int32_t num_meshes, uint32_t *plane, hipStream_t stream);

/* ---- rt_nearest_kernel.h, rt_sweep_kernel.h (in every build) ---- */
/* the signature is the ray kernels', `front` is not read */
hipError_t rt_launch_nearest(const rt_nearest_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream);
/* the sphere-cast kernel reads the records a nearest-surface launch over the origins, with the radii as limits, left in args->nearest */
hipError_t rt_launch_sweep(const rt_sweep_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream);

/* ---- rt_winding_kernel.h (in every build) ---- */
/* the kernel stages nothing in LDS and is the same for every scene placement: no shape */
hipError_t rt_launch_winding(const rt_winding_args *args, int num_cus, hipStream_t stream);

/* ---- rt_debug_kernels.h: the test hooks ---- */
hipError_t rt_launch_eval(int op, const uint32_t *in, uint32_t *out, int n, hipStream_t stream);
hipError_t rt_launch_exhaustive(unsigned long long *out4, hipStream_t stream);

}  /* extern "C" */

#endif
