"""Which descend loop a render-kernel shape runs and which descend_keep it gets (rt_device_scene.h: rt_descend_pops,
RT_DEF_DESCEND_KEEP_POP_LDS; rt_schedule.h: rt_sched::render_descend_keep), checked on the host: a small C++ program against the headers.
  - the 1024-thread shapes pop inside the descend loop, the smaller ones do not (tests/test_gpu_descend_pop.py relies on it: it runs its
    scenes on 1024 threads so that they reach rt_descend_pop);
  - without RT_AMD_DESCEND_KEEP a mesh scene in LDS on 1024 threads gets RT_DEF_DESCEND_KEEP_POP_LDS, every other shape RT_DEF_DESCEND_KEEP;
  - an explicit RT_AMD_DESCEND_KEEP reaches every shape as given, over its whole range: 63 is 63.
CPU test: nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include "rt_schedule.h"
int main()
{
    using rt_sched::Knobs;
    int bad = 0;
    for (const rt_shape &s : RT_SHAPES) {
        const bool pops = rt_descend_pops(s.threads, s.mode);
        if (pops != (s.threads == 1024)) { std::printf("rt_descend_pops(%d, %d) = %d\n", s.threads, s.mode, (int)pops); bad++; }
        const int want = s.has_mesh && s.threads == 1024 && s.mode == RT_SCENE_LDS ? RT_DEF_DESCEND_KEEP_POP_LDS : RT_DEF_DESCEND_KEEP;
        const int got = rt_sched::render_descend_keep(Knobs(), s);
        if (got != want) { std::printf("default of shape (%d, %d, %d): %d, not %d\n", s.has_mesh, s.mode, s.threads, got, want); bad++; }
        for (int v = 0; v <= 64; v++) {
            Knobs k;
            k.descend_keep = v;
            k.descend_keep_given = true;
            if (rt_sched::render_descend_keep(k, s) != v) { std::printf("explicit %d on shape (%d, %d, %d): %d\n", v, s.has_mesh, s.mode, s.threads, rt_sched::render_descend_keep(k, s)); bad++; }
            if (rt_sched::kernel_knobs(k, s.threads).descend_keep != v) bad++;
        }
    }
    if (RT_DEF_DESCEND_KEEP_POP_LDS < 0 || RT_DEF_DESCEND_KEEP_POP_LDS > 64) bad++;
    std::printf("%d\n", bad);
    return bad != 0;
}
"""


def test_shape_defaults_and_explicit_values(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src, exe = tmp_path / "keep.cpp", tmp_path / "keep"
    src.write_text(PROGRAM)
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "ray-tracer_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "0", r.stdout[-2000:]
