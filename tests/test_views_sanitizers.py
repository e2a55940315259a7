"""The host side of the camera sequences (ray-tracer_amd/csrc/rt_views_capi.cpp, rt_views.h, rt_sched::views_job_order) as host C++ under
AddressSanitizer + UndefinedBehaviorSanitizer, driven by tests/sanitize/views_host_fuzz.cpp - a stand-alone program with kernel-launcher
stubs of its own (CPU only): the launch schedule as a permutation of all (tile, view) jobs, the host form's chunks, rt_camera_lens, every
refusal of the entry points."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_views_host_side_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    rocm = "/opt/rocm"
    if gxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ or no HIP headers")
    csrc = os.path.join(ROOT, "ray-tracer_amd", "csrc")
    exe = str(tmp_path / "views_fuzz")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "sanitize", "views_host_fuzz.cpp"), os.path.join(csrc, "rt_views_capi.cpp"), os.path.join(csrc, "rt_capi.cpp"),
           os.path.join(csrc, "rt_host.cpp"), "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in (r.stderr or "") and "unrecognized" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")          # (the HIP runtime keeps what it allocates at start-up)
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed), "1500"], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])
