"""Every header under ray-tracer_amd/csrc/ includes what it uses: a file that holds nothing but `#include "X.h"` compiles (-fsyntax-only;
templates are not instantiated, so a header takes seconds).  A header that reaches <hip/hip_runtime.h>, directly or through its own includes,
is device code and goes through hipcc for gfx950; the others are host code and go through g++ against the HIP runtime's API headers, as in
test_sanitizers.py.  And build.HEADERS - what needs_build() watches - is exactly the directory's listing plus include/rt_amd.h, so an edited
header cannot leave a stale library behind.  CPU test: nothing runs on a GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
ROCM = "/opt/rocm"
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h")))


def _reaches_hip_runtime(path, seen=None):
    """does `path` include <hip/hip_runtime.h>, itself or through the project's headers it includes?"""
    seen = set() if seen is None else seen
    if path in seen:
        return False
    seen.add(path)
    with open(path) as f:
        text = f.read()
    if re.search(r'^\s*#\s*include\s*<hip/hip_runtime\.h>', text, re.M):
        return True
    for name in re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, re.M):
        for d in (os.path.dirname(path), CSRC, INCLUDE):
            inc = os.path.normpath(os.path.join(d, name))
            if os.path.exists(inc):
                if _reaches_hip_runtime(inc, seen):
                    return True
                break
    return False


def test_the_listing_has_device_and_host_headers():
    kinds = {_reaches_hip_runtime(h) for h in HEADERS}
    assert kinds == {True, False}, HEADERS


@pytest.mark.parametrize("header", HEADERS, ids=[os.path.basename(h) for h in HEADERS])
def test_header_compiles_on_its_own(header, tmp_path):
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    name = os.path.basename(header)
    includes = ["-I", CSRC, "-I", INCLUDE]
    if _reaches_hip_runtime(header):
        src = tmp_path / "only.hip"
        cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only"] + includes + [str(src)]
    else:
        gxx = shutil.which("g++")
        if gxx is None:
            pytest.skip("no g++")
        src = tmp_path / "only.cpp"
        cmd = [gxx, "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include")] + includes + [str(src)]
    src.write_text('#include "%s"\n' % name)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, r.stderr[-3000:])


def test_build_watches_every_header(rt):
    want = set(HEADERS) | {os.path.join(INCLUDE, "rt_amd.h")}
    got = [os.path.normpath(h) for h in rt.build.HEADERS]
    assert len(got) == len(set(got)) and set(got) == want, sorted(set(got) ^ want)
