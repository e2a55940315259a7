"""The host side of the cube-map sky (ray-tracer_amd/csrc/rt_sky.h, rt_sky_capi.cpp and the camera sequences' checks in rt_views_capi.cpp
they share) as host C++ under AddressSanitizer + UndefinedBehaviorSanitizer, driven by tests/sanitize/sky_host_fuzz.cpp - a stand-alone
program with the kernel launchers of tests/sanitize/launcher_stubs.h (CPU only): the lookup on random and special directions,
the round trip, the packing of a map, every refusal of the entry points."""
from sanitizer_programs import build_and_run


def test_sky_host_side_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "sky_host_fuzz", ['rt_sky_capi.cpp', 'rt_views_capi.cpp', 'rt_capi.cpp', 'rt_host.cpp'], seeds=(1, 2), iterations=3000)
