// The rebuild kernels' launcher (rt_rebuild.h) as a stub for tests/sanitize/update_host_check.cpp, which links rt_update_capi.cpp without
// rt_kernel.hip: it counts the call and fails.  rt_rebuild.h is included first, so a stub whose signature differs from the library's does not
// compile.  (The launchers of rt_launch.h are launcher_stubs.h's; these are not in that list yet: DESIGN.md section 21.)
#pragma once

#include "rt_rebuild.h"

static int g_rebuild_launches = 0;

extern "C" {
hipError_t rt_rebuild_enqueue(const rt_rebuild_args *, hipStream_t) { g_rebuild_launches++; return hipErrorUnknown; }
}
