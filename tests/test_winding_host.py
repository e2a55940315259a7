"""The host side of the winding-number queries (ray-tracer_amd/csrc/rt_winding.h, rt_winding_capi.cpp) as host C++ under AddressSanitizer +
UndefinedBehaviorSanitizer, driven by tests/sanitize/winding_host_check.cpp - a stand-alone program with its own main, the kernel launchers of
tests/sanitize/launcher_stubs.h, nothing preloaded (CPU only).  It runs rt_winding.h's text - what the
kernel compiles - against a straightforward binary64 sum on seeded random meshes and closed shapes, checks the flip bytes of every
rt_scene_add_* path against the construction, drives every refusal of the four entry points, and the scene's order list when the device gives
no memory."""
from sanitizer_programs import build_and_run

SOURCES = ["rt_winding_capi.cpp", "rt_capi.cpp", "rt_host.cpp"]


def test_winding_host_side_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "winding_host_check", SOURCES, seeds=(1, 2), iterations=100)
