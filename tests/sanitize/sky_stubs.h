// The sky kernel's launcher (rt_sky.h) as a stub for tests/sanitize/sky_host_fuzz.cpp, which links rt_sky_capi.cpp without rt_kernel.hip: it
// counts the call and fails.  rt_sky.h is included first, so a stub whose signature differs from the library's does not compile.  (The
// launchers of rt_launch.h are launcher_stubs.h's; this one is declared apart from them so that the programs which link the other translation
// units go on linking without it: DESIGN.md section 22.)
#pragma once

#include "rt_sky.h"

static int g_sky_launches = 0;

extern "C" {
hipError_t rt_sky_enqueue(const rt_kernel_args *, const float *, const float *, int32_t, rt_shape, int, size_t, hipStream_t) { g_sky_launches++; return hipErrorUnknown; }
}
