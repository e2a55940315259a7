"""The recipe the stand-alone host programs of tests/sanitize/ share: one program (its own main, kernel launchers from launcher_stubs.h) and
the library's host translation units it drives, compiled as host C++ with -fsanitize=address,undefined against the HIP runtime's API header,
linked with the runtime library and run directly, once per seed, with nothing preloaded.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracer_amd", "csrc")
ROCM = "/opt/rocm"


def build_and_run(tmp_path, program, sources, seeds, iterations):
    """tests/sanitize/<program>.cpp with csrc/<sources>, then `<program> <seed> <iterations>` for every seed: each run ends with status 0
    and says "sanitizers silent" """
    gxx = shutil.which("g++")
    if gxx is None or not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path / program)
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "sanitize", program + ".cpp")] + [os.path.join(CSRC, s) for s in sources] + [
           "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in (r.stderr or "") and "unrecognized" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")          # (the HIP runtime keeps what it allocates at start-up)
    for seed in seeds:
        r = subprocess.run([exe, str(seed), str(iterations)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])
