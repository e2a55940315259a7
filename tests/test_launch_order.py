"""The launch-order contract of include/rt_amd.h ("one launch in flight per context", "queued behind frames in flight") on the host: the
C ABI's host translation units under AddressSanitizer + UndefinedBehaviorSanitizer, linked with the fake recording runtime and the recording
kernel launchers of tests/sanitize/order_host_check.cpp instead of the HIP runtime library (a stand-alone program, CPU only, nothing
preloaded).  Its checker computes happens-before over every copy, fill, event and launch the entry points queue - the fixed sequences of
tests/test_gpu_streams.py and seeded random ones over several streams and contexts - and must find nothing; built with
-DORDER_CHECK_NO_WAITS, which makes the fake hipStreamWaitEvent do nothing, it must find what is then missing."""
import os
import re

import pytest

from sanitizer_programs import SANITIZE, compile_objects, link_program, run_program
from test_launch_seam import DECLARED, DEFINITION, _names

SOURCES = ["rt_capi.cpp", "rt_pipeline_capi.cpp", "rt_query_capi.cpp", "rt_occlusion_capi.cpp", "rt_ao_capi.cpp", "rt_denoise_capi.cpp",
           "rt_adaptive_capi.cpp", "rt_views_capi.cpp", "rt_host.cpp", "rt_multi_capi.cpp", "rt_sky_capi.cpp", "rt_update_capi.cpp", "rt_nearest_capi.cpp",
           "rt_multihit_capi.cpp", "rt_winding_capi.cpp", "rt_sweep_capi.cpp", "rt_overlap_capi.cpp", "rt_tritri_capi.cpp"]
SEEDS = (1, 2, 3)
ITERATIONS = 4000


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    return compile_objects(tmp_path_factory.mktemp("launch_order"), SOURCES)


def test_the_recorders_define_every_launcher_once():
    assert sorted(_names(DEFINITION, os.path.join(SANITIZE, "launcher_recorders.h"))) == sorted(DECLARED)


def test_every_entry_point_keeps_the_launch_order(objects, tmp_path):
    exe = link_program(tmp_path, "order_host_check", objects)
    for seed in SEEDS:
        r = run_program(exe, seed, ITERATIONS)
        assert r.returncode == 0 and "no violation, sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])
        calls, refused, launches = (int(x) for x in re.search(r"(\d+) calls \((\d+) refused\), (\d+) launches", r.stdout).groups())
        assert calls > ITERATIONS // 2 and refused > 50 and launches > calls, r.stdout
        # the tile-list cache (its capacity lowered by the driver) recycled entries, some of them too small for their new list: what rewrites a
        # pinned buffer an upload may still read, and frees a device buffer a pending launch may still read
        recycled, regrown = (int(x) for x in re.search(r"(\d+) tile-list entries recycled \((\d+) of them regrown\)", r.stdout).groups())
        assert recycled > 100 and regrown > 0, r.stdout


def test_the_checker_finds_missing_waits(objects, tmp_path):
    """the same program, the same sequences, with hipStreamWaitEvent a no-op in the test program's runtime (the library is the same objects)"""
    exe = link_program(tmp_path, "order_host_check", objects, name="order_host_check_no_waits", defines=("ORDER_CHECK_NO_WAITS",))
    r = run_program(exe, SEEDS[0], ITERATIONS)
    assert r.returncode == 3 and re.search(r"launch order: [1-9]\d* violations", r.stdout), (r.returncode, (r.stderr or r.stdout)[-3000:])
    assert "sanitizers silent" not in r.stdout
    # what it names: the shared scratch of two calls on two streams, and the frames in flight
    assert "ticket counter" in r.stderr and "is not ordered behind" in r.stderr, r.stderr[-3000:]
    # ... and what the later families share: the view's cull plane, a scene's blob under an update, the context's query records (the program
    # prints the first violation of every buffer, so these are not lost behind the first twelve)
    for kernel, buffer in (("cull pre-pass", "cull plane"), ("rebuild", "scene blob"), ("nearest", "nearest records"),
                           ("sphere cast", "sweep start records")):
        assert re.search(r"order violation: \w+ of %s \[\d+, \d+\) by %s in " % (buffer, kernel), r.stderr), (buffer, r.stderr[-3000:])
