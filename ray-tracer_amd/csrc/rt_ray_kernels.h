/*
 * rt_ray_kernels.h — the three ray kernels with their launchers or, in the development builds, launchers that refuse: theirs, the
 * multi-hit kernel's two and the two overlap kernels', which rt_multihit_kernel.h, rt_overlap_kernel.h and rt_tritri_kernel.h then leave
 * out.  This is the one place that decides it.
 *
 * The development builds (-DRT_STATS, -DRT_COSTMAP, -DRT_MARK) instrument the render kernel alone.  The ray kernels call rt_descend
 * (rt_traverse.h), which in those builds takes the render kernel's counters (RT_STAT_PARAMS, rt_instrument.h) and counts into them.  To
 * build the ray kernels there too, each would have to declare counters of its own and pass them (RT_STAT_ARGS names the render kernel's
 * variables), or rt_descend would have to take its counters as a template parameter that the ray kernels leave empty.
 */
#ifndef RT_RAY_KERNELS_H
#define RT_RAY_KERNELS_H

#if !defined(RT_STATS) && !defined(RT_COSTMAP) && !defined(RT_MARK)
#define RT_RAY_KERNELS_BUILT 1     /* read by rt_multihit_kernel.h, rt_overlap_kernel.h and rt_tritri_kernel.h, which rt_kernel.hip includes behind everything else */
/* closest-hit ray queries and the AOV pass: rt_query_kernel and its launcher */
#include "rt_query_kernel.h"
/* occlusion (any-hit) ray queries and the light-visibility plane: rt_occlusion_kernel and its launcher */
#include "rt_occlusion_kernel.h"
/* the ambient-occlusion plane: rt_ao_kernel and its launcher */
#include "rt_ao_kernel.h"
#else
#define RT_RAY_KERNELS_BUILT 0
#include <hip/hip_runtime.h>

#include "rt_launch.h"
extern "C" hipError_t rt_launch_query(const rt_query_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rt_launch_occlusion(const rt_occlusion_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rt_launch_ao(const rt_ao_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rt_launch_multihit(const rt_multihit_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rt_launch_multihit_uv(const rt_multihit_uv_args *, int, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rt_launch_overlap(const rt_overlap_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rt_launch_tritri(const rt_tritri_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
#endif

#endif
