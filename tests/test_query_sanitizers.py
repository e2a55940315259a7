"""The ray-query / AOV entry points' argument checks (ray-tracer_amd/csrc/rt_query_capi.cpp) as host C++ under AddressSanitizer +
UndefinedBehaviorSanitizer, driven by tests/sanitize/query_host_fuzz.cpp with the kernel launchers of tests/sanitize/launcher_stubs.h (CPU only)."""
from sanitizer_programs import build_and_run


def test_query_entry_points_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "query_host_fuzz", ['rt_query_capi.cpp', 'rt_capi.cpp', 'rt_host.cpp'], seeds=(1, 2), iterations=2000)
