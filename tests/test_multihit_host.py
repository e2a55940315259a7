"""The host side of rt_trace_rays_multi[_device] (ray-tracer_amd/csrc/rt_multihit.h, rt_multihit_capi.cpp) as host C++ under
AddressSanitizer + UndefinedBehaviorSanitizer, driven by tests/sanitize/multihit_host_check.cpp - a stand-alone program with its own main,
the kernel launchers of tests/sanitize/launcher_stubs.h, nothing preloaded (CPU only).  It
runs the kernel's walk and insert - the text the kernel compiles - as plain host code against the exhaustive sort over every candidate,
byte for byte, on seeded random and adversarial scenes, and drives every refusal of both entry points.  The second test sets the same host
code against the NumPy yardstick (tests/multihit_ref.py) on scenes of the suite: two independent statements of the header's definition,
equal as bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import multihit_ref as R
from sanitizer_programs import CSRC, ROCM, RUN_ENV, SANITIZE, _compiler, _run_compiler

SOURCES = ["rt_multihit_capi.cpp", "rt_capi.cpp", "rt_host.cpp"]
REC = np.dtype([("t", np.float32), ("object", np.int32), ("triangle", np.int32)])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """the program, built once for both tests by sanitizer_programs' recipe"""
    exe = str(tmp_path_factory.mktemp("multihit_host") / "multihit_host_check")
    _run_compiler(_compiler() + [os.path.join(SANITIZE, "multihit_host_check.cpp")] + [os.path.join(CSRC, s) for s in SOURCES] + [
                  "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    return exe


def test_multihit_host_side_under_asan_and_ubsan(program):
    for seed in (1, 2):
        r = subprocess.run([program, str(seed), "60"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])


def host_records(program, tmp_path, flat, o, d, k, tmax):
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<10i", flat["blob"].shape[0], flat["off_nodes"], flat["off_tris"], flat["off_meshes"], flat["num_meshes"], len(flat["objects"]),
                            flat["stack_entries"], n, int(tmax is not None), k))
        f.write(np.ascontiguousarray(flat["blob"], np.float32).tobytes())
        f.write(o.tobytes())
        f.write(d.tobytes())
        if tmax is not None:
            f.write(np.ascontiguousarray(tmax, np.float32).tobytes())
    r = subprocess.run([program, "file", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **RUN_ENV))
    assert r.returncode == 0 and "sanitizers silent" in r.stdout, (r.stderr or r.stdout)[-3000:]
    raw = (tmp_path / "out.bin").read_bytes()
    return np.frombuffer(raw[:4 * n], np.int32), np.frombuffer(raw[4 * n:], REC).reshape(n, k)


def same(got, want_hits, want_counts, what):
    counts, recs = got
    assert counts.tobytes() == want_counts.tobytes(), (what, np.nonzero(counts != want_counts)[0][:10])
    for field in ("t", "object", "triangle"):
        a, b = recs[field], want_hits[field]
        assert a.tobytes() == b.tobytes(), (what, field, np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:10])


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey", "reference_scene0", "random13", "random15"])
def test_host_code_equals_the_yardstick(rt, program, tmp_path, name):
    from random_scenes import random_scene
    objs = random_scene(int(name[6:]))[0] if name.startswith("random") else rt.scenes.CONFIG_SCENES[name]()[0]
    flat = rt.SceneObjects(objs).debug_flatten()
    o, d = R.query_rays(flat, 7, 400)
    cand = R.candidates(flat, o, d)
    for k in (0, 1, 3, 8):
        hits, counts = R.multi(flat, o, d, k, cand=cand)
        same(host_records(program, tmp_path, flat, o, d, k, None), hits, counts, (name, k))
    # limits: the key of each ray's second candidate (its first where it has one only), one ulp down, one ulp up
    col = np.minimum(1, np.maximum(cand.total - 1, 0))
    key = np.where(cand.total > 0, np.take_along_axis(cand.key, col[:, None].astype(np.int64), axis=1)[:, 0], np.float32(1)).astype(np.float32)
    for lim in (key, np.nextafter(key, np.float32(0)), np.nextafter(key, np.float32(np.inf))):
        for k in (0, 2):
            hits, counts = R.multi(flat, o, d, k, lim)
            same(host_records(program, tmp_path, flat, o, d, k, lim), hits, counts, (name, k, "limits"))
