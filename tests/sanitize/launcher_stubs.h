// Every kernel launcher of rt_launch.h as a stub for the stand-alone host programs of this directory, which link the library's host
// translation units without rt_kernel.hip: a launcher counts the call and fails, the occupancy probe answers 1.  Included by one
// translation unit per program (the program's own), whichever of the library's translation units it links: a render launch of a mesh
// scene reaches the cull pre-pass's stub, which fails like the rest - the launch then renders without a plane.  rt_launch.h is included first, so a stub whose signature differs from the
// library's does not compile; tests/test_launch_seam.py checks that every launcher has its stub here and nowhere else.
#pragma once

#include "rt_launch.h"

static int g_launches = 0;            // launchers reached so far: stays 0 over calls that are refused

extern "C" {
int rt_kernel_blocks_per_cu(rt_shape, size_t) { return 1; }
hipError_t rt_launch_render(const rt_kernel_args *, rt_shape, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_budget(const rt_kernel_args *, const uint16_t *, uint32_t *, rt_shape, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_views(const rt_kernel_args *, const float *, rt_shape, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_sky(const rt_kernel_args *, const float *, const float *, int32_t, rt_shape, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_blend(const float *, long long, int, int, float *, long long, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_blend_tiles(const float *, long long, int, int, float *, const uint32_t *, int, int, int, int, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_tiles_copy(float *, float *, const uint32_t *, int, int, int, int, int, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_rgba8(const float *, int, uint8_t *, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_query(const rt_query_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_occlusion(const rt_occlusion_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_ao(const rt_ao_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_multihit(const rt_multihit_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_multihit_uv(const rt_multihit_uv_args *, int, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_overlap(const rt_overlap_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_tritri(const rt_tritri_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_denoise_pack(const rt_denoise_args *, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_denoise_level(const rt_denoise_args *, int, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_adaptive_plan(const rt_plan_args *, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_adaptive_combine(const float *, const float *, const uint32_t *, float *, uint32_t *, long long, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_rebuild(const rt_rebuild_args *, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_cull(const float *, int32_t, int32_t, int32_t, const rt_f4 *, int32_t, int32_t, int32_t, int32_t, uint32_t *, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_nearest(const rt_nearest_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_sweep(const rt_sweep_args *, rt_shape, int, int, size_t, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_winding(const rt_winding_args *, int, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_eval(int, const uint32_t *, uint32_t *, int, hipStream_t) { g_launches++; return hipErrorUnknown; }
hipError_t rt_launch_exhaustive(unsigned long long *, hipStream_t) { g_launches++; return hipErrorUnknown; }
}
