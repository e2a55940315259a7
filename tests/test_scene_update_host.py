"""The host side of rt_scene_update_mesh[_device] (ray-tracer_amd/csrc/rt_update_capi.cpp, rt_rebuild.h) as host C++ under AddressSanitizer +
UndefinedBehaviorSanitizer, driven by tests/sanitize/update_host_check.cpp - a stand-alone program with its own main, the kernel launchers of
tests/sanitize/launcher_stubs.h, nothing preloaded (CPU only).  It checks the plan - a mesh's tree from its
triangle count alone - against the builder's tree for every count from 0 to 3,000 and larger ones up to 2^20 - 1; runs the device algorithm as plain host
code (the same __host__ __device__ arithmetic, a std::sort of the composite words, ordered box reductions) on random, tied, signed-zero and
textured meshes against a fresh flatten, byte for byte; and drives every refusal of both entry points."""
from sanitizer_programs import build_and_run


def test_update_host_side_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "update_host_check", ["rt_update_capi.cpp", "rt_capi.cpp", "rt_host.cpp"], seeds=(1,), iterations=3000)
