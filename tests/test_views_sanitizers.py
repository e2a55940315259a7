"""The host side of the camera sequences (ray-tracer_amd/csrc/rt_views_capi.cpp, rt_views.h, rt_sched::views_job_order) as host C++ under
AddressSanitizer + UndefinedBehaviorSanitizer, driven by tests/sanitize/views_host_fuzz.cpp - a stand-alone program with the kernel launchers
of tests/sanitize/launcher_stubs.h (CPU only): the launch schedule as a permutation of all (tile, view) jobs, the host form's chunks, rt_camera_lens, every
refusal of the entry points."""
from sanitizer_programs import build_and_run


def test_views_host_side_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "views_host_fuzz", ['rt_views_capi.cpp', 'rt_capi.cpp', 'rt_host.cpp'], seeds=(1, 2), iterations=1500)
