"""The host side of rt_overlap_triangles[_device] (ray-tracer_amd/csrc/rt_tritri.h, rt_tritri_capi.cpp) as host C++ under AddressSanitizer +
UndefinedBehaviorSanitizer, driven by tests/sanitize/tritri_host_check.cpp - a stand-alone program with its own main, the kernel launchers
of tests/sanitize/launcher_stubs.h, nothing preloaded (CPU only).  It runs the kernel's traversal, triangle test, id insert and segment -
the text the kernel compiles - as plain host code against the exhaustive loop over every candidate, as bytes, on seeded random and
adversarial scenes, and drives every refusal of both entry points.  The second test sets the same host code against the NumPy yardstick
(tests/tritri_ref.py) on scenes of the suite: two independent statements of the header's definition, equal as bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tritri_ref as R
from sanitizer_programs import CSRC, ROCM, RUN_ENV, SANITIZE, _compiler, _run_compiler

SOURCES = ["rt_tritri_capi.cpp", "rt_capi.cpp", "rt_host.cpp"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """the program, built once for both tests by sanitizer_programs' recipe"""
    exe = str(tmp_path_factory.mktemp("tritri_host") / "tritri_host_check")
    _run_compiler(_compiler() + [os.path.join(SANITIZE, "tritri_host_check.cpp")] + [os.path.join(CSRC, s) for s in SOURCES] + [
                  "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    return exe


def test_tritri_host_side_under_asan_and_ubsan(program):
    for seed in (1, 2):
        r = subprocess.run([program, str(seed), "100"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])


def host_answers(program, tmp_path, flat, tris, k):
    n = tris.shape[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<9i", flat["blob"].shape[0], flat["off_nodes"], flat["off_tris"], flat["off_meshes"], flat["num_meshes"], len(flat["objects"]),
                            flat["stack_entries"], n, k))
        f.write(np.ascontiguousarray(flat["blob"], np.float32).tobytes())
        f.write(np.ascontiguousarray(tris, np.float32).tobytes())
    run = subprocess.run([program, "file", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
    assert run.returncode == 0 and "sanitizers silent" in run.stdout, (run.stderr or run.stdout)[-3000:]
    raw = (tmp_path / "out.bin").read_bytes()
    assert len(raw) == n * (5 + 40 * k)
    return (np.frombuffer(raw, np.int32, n), np.frombuffer(raw, np.uint8, n, 4 * n), np.frombuffer(raw, R.ID_DTYPE, n * k, 5 * n).reshape(n, k),
            np.frombuffer(raw, R.SEG_DTYPE, n * k, 5 * n + 8 * n * k).reshape(n, k))


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey", "reference_scene0", "random13", "random15"])
def test_host_code_equals_the_yardstick(rt, program, tmp_path, name):
    from random_scenes import random_scene
    objs = random_scene(int(name[6:]))[0] if name.startswith("random") else rt.scenes.CONFIG_SCENES[name]()[0]
    flat = rt.SceneObjects(objs).debug_flatten()
    tris = np.concatenate([R.query_triangles(flat, 7, 240), R.anchored_triangles(flat, 8, 60)])
    for k in (3, 8):
        counts, flags, ids, segs = R.overlap(flat, tris, k, segments=True)
        got = host_answers(program, tmp_path, flat, tris, k)
        assert got[0].tobytes() == counts.tobytes(), (name, k, np.nonzero(got[0] != counts)[0][:10])
        assert got[1].tobytes() == flags.tobytes(), (name, k)
        assert got[2].tobytes() == ids.tobytes(), (name, k, np.argwhere(got[2] != ids)[:10].tolist())
        assert got[3].tobytes() == segs.tobytes(), (name, k, np.argwhere(got[3]["kind"] != segs["kind"])[:10].tolist())
    # (three_sphere has three candidates in all, and a triangle of these sizes cuts at most seven of the cube scene's: no query there meets more than eight)
    assert (counts > 0).any() and (counts == 0).any() and (name in ("three_sphere", "cube") or (counts > 8).any()), (name, "the queries do not reach every case")
    assert (segs["kind"] == 1).any() or name == "three_sphere", name
