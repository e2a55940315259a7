"""The host side of the fast winding numbers (ray-tracer_amd/csrc/rt_winding.h, rt_winding_capi.cpp) as host C++ under AddressSanitizer +
UndefinedBehaviorSanitizer, driven by tests/sanitize/winding_fast_host_check.cpp - a stand-alone program with its own main, the kernel launchers
of tests/sanitize/launcher_stubs.h, nothing preloaded (CPU only).  It runs the cluster-tree builder on triangle counts around the leaf size, the
gather, the moments and the walk - the text the kernels compile - against a plain binary64 sum of solid angles on seeded random meshes and a
degenerate mesh of zero area, drives every refusal of the four new entry points, and checks that a preparation the device refuses leaves the
scene as it was."""
from sanitizer_programs import build_and_run

SOURCES = ["rt_winding_capi.cpp", "rt_capi.cpp", "rt_host.cpp"]


def test_winding_fast_host_side_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "winding_fast_host_check", SOURCES, seeds=(1, 2), iterations=100)
