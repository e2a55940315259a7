"""The primary-ray cull on the CPU (ray-tracer_amd/csrc/rt_cull.h): the predicate is sound against the slab test's three forms
(tests/sanitize/cull_soundness.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer), it is not vacuous on the monkey scene
(tools/primary_cull_estimate.py), the context's bookkeeping of the plane follows the view (tests/sanitize/cull_key_check.cpp), and the host
evaluation writes the plane's bits where the kernels read them.  Nothing runs on a GPU."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracer_amd", "csrc")


def sanitized(tmp_path, source):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / os.path.splitext(source)[0])
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", source), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in (r.stderr or "") and "unrecognized" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_the_predicate_is_sound_against_the_three_slab_forms(tmp_path):
    """1.2 million (pixel, jitter, box) triples per seed, adversarial and degenerate boxes and zero direction components among them: not one in
    which a slab form accepts a box the predicate calls certainly missed"""
    exe = sanitized(tmp_path, "cull_soundness.cpp")
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed), "1200000"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "no counter-example, sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])
        print(r.stdout.strip())


def test_the_plane_bookkeeping_follows_the_view(tmp_path):
    exe = sanitized(tmp_path, "cull_key_check.cpp")
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])


def test_the_library_has_the_pre_pass_launcher(rt):
    """rt_capi.cpp refers to rt_cull_enqueue weakly, so that the host programs of tests/sanitize/ link without rt_kernel.hip; a library built
    without the kernel would load and render every launch without a plane.  The shipped library must define the launcher, and says so itself."""
    L = rt.lib()
    assert hasattr(L, "rt_cull_enqueue"), "libraytracer_amd.so does not define rt_cull_enqueue"
    assert L.rt_debug_primary_cull_linked() == 1


def estimate_tool():
    spec = importlib.util.spec_from_file_location("primary_cull_estimate", os.path.join(ROOT, "tools", "primary_cull_estimate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_predicate_is_not_vacuous_on_the_monkey(rt):
    """at 128x72 at least a quarter of the pixels whose jitter cone may enter the monkey's root box are flagged (a floor with headroom under the
    44 % an approximate, non-conservative estimate gave: conservative margins that cost more than that are too loose)"""
    st = estimate_tool().estimate("monkey", 128, 72, True)
    print(st)
    assert st["root_entering"] > 2000 and st["flagged_share_of_root_entering"] >= 0.25, st
    assert 0.0 < st["step_share_of_flagged"] < 1.0, st


def test_the_host_plane_has_a_pixel_per_bit(rt):
    """bit (pixel & 31) of word pixel >> 5, pixel = py * width + px, on a ragged size; without a mesh nothing is reachable and every pixel is
    flagged; a camera inside the mesh's root box flags none"""
    objs, _ = rt.scenes.monkey()
    w, h = 37, 21
    words, st = rt.primary_cull_host(rt.SceneObjects(objs), rt.Camera(w, h), True)
    bits = rt.cull.plane_bits(words, w, h)
    assert words.size == rt.cull.plane_words(w, h) == st["words"] and int(bits.sum()) == st["flagged"]
    assert bits[0, 0] == 1 and bits[h // 2, w // 2] == 0, "the corner sees no mesh, the centre sees the monkey"
    tail = np.unpackbits(words.view(np.uint8), bitorder="little")[w * h:]
    assert not tail.any(), "bits past the image stay clear"
    assert not rt.cull.plane_bits(rt.primary_cull_host(rt.SceneObjects(objs), rt.Camera(w, h), False)[0], w, h)[h // 2, w // 2]
    inside, st_in = rt.primary_cull_host(rt.SceneObjects(objs), rt.Camera(w, h, pos=(0.1, -0.1, 1.6)), True)
    assert st_in["flagged"] == 0 and st_in["root_entering"] == w * h
    spheres, _ = rt.scenes.three_sphere()
    none, st_none = rt.primary_cull_host(rt.SceneObjects(spheres), rt.Camera(w, h), True)
    assert st_none["flagged"] == w * h and st_none["root_entering"] == 0
