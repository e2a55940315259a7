"""The host side of the budget render and the adaptive driver (ray-tracer_amd/csrc/rt_adaptive_capi.cpp, rt_adaptive.h) as host C++ under
AddressSanitizer + UndefinedBehaviorSanitizer, driven by tests/sanitize/adaptive_host_fuzz.cpp - a stand-alone program with the kernel launchers
of tests/sanitize/launcher_stubs.h (CPU only): a pass's tile list, the parameter validation, every refusal of the entry points."""
from sanitizer_programs import build_and_run


def test_adaptive_host_side_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "adaptive_host_fuzz", ['rt_adaptive_capi.cpp', 'rt_capi.cpp', 'rt_host.cpp'], seeds=(1, 2), iterations=2000)
