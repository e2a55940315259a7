"""The host side of rt_nearest_points[_device] (ray-tracer_amd/csrc/rt_nearest.h, rt_nearest_capi.cpp) as host C++ under AddressSanitizer +
UndefinedBehaviorSanitizer, driven by tests/sanitize/nearest_host_check.cpp - a stand-alone program with its own main, the kernel launchers of
tests/sanitize/launcher_stubs.h, nothing preloaded (CPU only).  It runs the kernel's
traversal - the text the kernel compiles - as plain host code against the exhaustive minimum over every candidate, byte for byte, on seeded
random and adversarial scenes, and drives every refusal of both entry points.  The second test sets the same host code against the NumPy
yardstick (tests/nearest_ref.py) on scenes of the suite: two independent statements of the header's definition, equal as bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import nearest_ref as R
from sanitizer_programs import CSRC, ROCM, RUN_ENV, SANITIZE, _compiler, _run_compiler

SOURCES = ["rt_nearest_capi.cpp", "rt_capi.cpp", "rt_host.cpp"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """the program, built once for both tests by sanitizer_programs' recipe"""
    exe = str(tmp_path_factory.mktemp("nearest_host") / "nearest_host_check")
    _run_compiler(_compiler() + [os.path.join(SANITIZE, "nearest_host_check.cpp")] + [os.path.join(CSRC, s) for s in SOURCES] + [
                  "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    return exe


def test_nearest_host_side_under_asan_and_ubsan(program):
    for seed in (1, 2):
        r = subprocess.run([program, str(seed), "120"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])


def host_records(program, tmp_path, flat, points, max_dist):
    points = np.ascontiguousarray(points, np.float32)
    n = points.shape[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<9i", flat["blob"].shape[0], flat["off_nodes"], flat["off_tris"], flat["off_meshes"], flat["num_meshes"], len(flat["objects"]),
                            flat["stack_entries"], n, int(max_dist is not None)))
        f.write(np.ascontiguousarray(flat["blob"], np.float32).tobytes())
        f.write(points.tobytes())
        if max_dist is not None:
            f.write(np.ascontiguousarray(max_dist, np.float32).tobytes())
    r = subprocess.run([program, "file", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
    assert r.returncode == 0 and "sanitizers silent" in r.stdout, (r.stderr or r.stdout)[-3000:]
    return np.fromfile(tmp_path / "out.bin", R.DTYPE)


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey", "reference_scene0", "random13", "random15"])
def test_host_code_equals_the_yardstick(rt, program, tmp_path, name):
    from random_scenes import random_scene
    objs = random_scene(int(name[6:]))[0] if name.startswith("random") else rt.scenes.CONFIG_SCENES[name]()[0]
    flat = rt.SceneObjects(objs).debug_flatten()
    pts = R.query_points(flat, 7, 300, n_sample=25)
    want = R.nearest(flat, pts)
    got = host_records(program, tmp_path, flat, pts, None)
    assert got.tobytes() == want.tobytes(), (name, np.nonzero(got != want)[0][:10])
    # limits: the answer's own distance, one ulp down, one ulp up
    d = want["distance"]
    for lim in (d, np.nextafter(d, np.float32(0)), np.nextafter(d, np.float32(np.inf))):
        want_l = R.nearest(flat, pts, lim)
        got_l = host_records(program, tmp_path, flat, pts, lim)
        assert got_l.tobytes() == want_l.tobytes(), (name, np.nonzero(got_l != want_l)[0][:10])
