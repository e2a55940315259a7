"""The host side of rt_sweep_spheres[_device] (ray-tracer_amd/csrc/rt_sweep.h, rt_sweep_capi.cpp) as host C++ under AddressSanitizer +
UndefinedBehaviorSanitizer, driven by tests/sanitize/sweep_host_check.cpp - a stand-alone program with its own main, the kernel launchers of
tests/sanitize/launcher_stubs.h, nothing preloaded (CPU only).  It runs the kernel's traversal - the text the kernel compiles - as plain
host code against the exhaustive minimum over every candidate, byte for byte, on seeded random and adversarial scenes, and drives every
refusal of both entry points.  The second test sets the same host code against the NumPy yardstick (tests/sweep_ref.py) on scenes of the
suite: two independent statements of the header's definition, equal as bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import sweep_ref as R
from sanitizer_programs import CSRC, ROCM, RUN_ENV, SANITIZE, _compiler, _run_compiler

SOURCES = ["rt_sweep_capi.cpp", "rt_capi.cpp", "rt_host.cpp"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """the program, built once for both tests by sanitizer_programs' recipe"""
    exe = str(tmp_path_factory.mktemp("sweep_host") / "sweep_host_check")
    _run_compiler(_compiler() + [os.path.join(SANITIZE, "sweep_host_check.cpp")] + [os.path.join(CSRC, s) for s in SOURCES] + [
                  "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    return exe


def test_sweep_host_side_under_asan_and_ubsan(program):
    for seed in (1, 2):
        r = subprocess.run([program, str(seed), "120"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])


def host_records(program, tmp_path, flat, o, d, r, tmax):
    n = o.shape[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<9i", flat["blob"].shape[0], flat["off_nodes"], flat["off_tris"], flat["off_meshes"], flat["num_meshes"], len(flat["objects"]),
                            flat["stack_entries"], n, int(tmax is not None)))
        f.write(np.ascontiguousarray(flat["blob"], np.float32).tobytes())
        for a in (o, d, r):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        if tmax is not None:
            f.write(np.ascontiguousarray(tmax, np.float32).tobytes())
    run = subprocess.run([program, "file", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
    assert run.returncode == 0 and "sanitizers silent" in run.stdout, (run.stderr or run.stdout)[-3000:]
    return np.fromfile(tmp_path / "out.bin", R.DTYPE)


def differing(got, want):
    return np.nonzero(got.view(np.uint8).reshape(-1, R.DTYPE.itemsize) != want.view(np.uint8).reshape(-1, R.DTYPE.itemsize))[0][:10]


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey", "reference_scene0", "random13", "random15"])
def test_host_code_equals_the_yardstick(rt, program, tmp_path, name):
    from random_scenes import random_scene
    objs = random_scene(int(name[6:]))[0] if name.startswith("random") else rt.scenes.CONFIG_SCENES[name]()[0]
    flat = rt.SceneObjects(objs).debug_flatten()
    o, d, r = R.query_sweeps(flat, 7, 400)
    detail = {}
    want = R.sweep(flat, o, d, r, detail=detail)
    got = host_records(program, tmp_path, flat, o, d, r, None)
    assert got.tobytes() == want.tobytes(), (name, differing(got, want))
    # limits: the winner's own key, one ulp down, one ulp up (1 where there is no winner)
    key = np.where(np.isnan(detail["key"]), np.float32(1), detail["key"]).astype(np.float32)
    for lim in (key, np.nextafter(key, np.float32(0)), np.nextafter(key, np.float32(np.inf))):
        want_l = R.sweep(flat, o, d, r, lim)
        got_l = host_records(program, tmp_path, flat, o, d, r, lim)
        assert got_l.tobytes() == want_l.tobytes(), (name, differing(got_l, want_l))
