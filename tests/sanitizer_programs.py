"""The recipe the stand-alone host programs of tests/sanitize/ share: one program (its own main, every kernel launcher of rt_launch.h from launcher_stubs.h) and
the library's host translation units it drives, compiled as host C++ with -fsanitize=address,undefined against the HIP runtime's API header,
linked with the runtime library and run directly, once per seed, with nothing preloaded.  CPU only.

A program that brings a runtime of its own (order_host_check.cpp: a fake one that records) is linked without the HIP runtime library:
compile_objects() builds the library's translation units once, link_program() the program with them - once per set of -D flags."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracer_amd", "csrc")
SANITIZE = os.path.join(ROOT, "tests", "sanitize")
ROCM = "/opt/rocm"
RUN_ENV = dict(ASAN_OPTIONS="detect_leaks=0")          # (the HIP runtime keeps what it allocates at start-up)


def _compiler():
    gxx = shutil.which("g++")
    if gxx is None or not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ or no HIP headers")
    return [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
            "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"), "-I", CSRC]


def _run_compiler(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in (r.stderr or "") and "unrecognized" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]


def build_and_run(tmp_path, program, sources, seeds, iterations):
    """tests/sanitize/<program>.cpp with csrc/<sources>, then `<program> <seed> <iterations>` for every seed: each run ends with status 0
    and says "sanitizers silent" """
    exe = str(tmp_path / program)
    _run_compiler(_compiler() + [os.path.join(SANITIZE, program + ".cpp")] + [os.path.join(CSRC, s) for s in sources] + [
                  "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    env = dict(os.environ, **RUN_ENV)
    for seed in seeds:
        r = subprocess.run([exe, str(seed), str(iterations)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])


def compile_objects(tmp_path, sources):
    """csrc/<sources> as object files under the sanitizers, a few at a time; -> their paths"""
    base = _compiler()
    objects = [str(tmp_path / (os.path.splitext(s)[0] + ".o")) for s in sources]
    with ThreadPoolExecutor(max_workers=min(4, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda so: _run_compiler(base + ["-c", os.path.join(CSRC, so[0]), "-o", so[1]]), zip(sources, objects)))
    return objects


def link_program(tmp_path, program, objects, name=None, defines=()):
    """tests/sanitize/<program>.cpp (with -D<defines>) and `objects`, without the HIP runtime library: the program defines what they call"""
    exe = str(tmp_path / (name or program))
    _run_compiler(_compiler() + ["-D" + d for d in defines] + [os.path.join(SANITIZE, program + ".cpp")] + list(objects) + ["-o", exe])
    return exe


def run_program(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
