// The winding-number kernel's launcher (rt_winding.h) as a stub for tests/sanitize/winding_host_check.cpp, which links rt_winding_capi.cpp
// without rt_kernel.hip: it counts the call and fails.  rt_winding.h is included first, so a stub whose signature differs from the library's
// does not compile.  (The launchers of rt_launch.h are launcher_stubs.h's, the nearest-surface kernel's nearest_stubs.h's.)
#pragma once

#include "rt_winding.h"

static int g_winding_launches = 0;

extern "C" {
hipError_t rt_winding_launch(const rt_winding_args *, int, hipStream_t) { g_winding_launches++; return hipErrorUnknown; }
}
