// The multi-hit kernel's launcher (rt_multihit.h) as a stub for tests/sanitize/multihit_host_check.cpp, which links rt_multihit_capi.cpp
// without rt_kernel.hip: it counts the call and fails.  rt_multihit.h is included first, so a stub whose signature differs from the
// library's does not compile.  (The launchers of rt_launch.h are launcher_stubs.h's.)
#pragma once

#include "rt_multihit.h"

static int g_multihit_launches = 0;

extern "C" {
hipError_t rt_multihit_launch(const rt_multihit_args *, rt_shape, int, int, size_t, hipStream_t) { g_multihit_launches++; return hipErrorUnknown; }
hipError_t rt_multihit_uv_launch(const rt_multihit_uv_args *, int, hipStream_t) { g_multihit_launches++; return hipErrorUnknown; }
}
