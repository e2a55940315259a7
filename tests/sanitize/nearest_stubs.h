// The nearest-surface kernel's launcher (rt_nearest.h) as a stub for tests/sanitize/nearest_host_check.cpp, which links rt_nearest_capi.cpp
// without rt_kernel.hip: it counts the call and fails.  rt_nearest.h is included first, so a stub whose signature differs from the library's
// does not compile.  (The launchers of rt_launch.h are launcher_stubs.h's.)
#pragma once

#include "rt_nearest.h"

static int g_nearest_launches = 0;

extern "C" {
hipError_t rt_nearest_launch(const rt_nearest_args *, rt_shape, int, int, size_t, hipStream_t) { g_nearest_launches++; return hipErrorUnknown; }
}
