"""The sub-entry words on the CPU (ray-tracer_amd/csrc/rt_entry.h, "The sub-entry words"): for a pixel whose own entry word is 0 each of the 64
sub-boxes of its jitter cube gets rt_entry_word of its sub-cone.  For every table pixel and every sub-box with a non-zero word the kernel's
float traversal from the root and the start from the sub-word end with the same (w_prim, w_best) bits (tests/sanitize/subentry_soundness.cpp,
under AddressSanitizer + UndefinedBehaviorSanitizer, a stand-alone program; it also shows that it finds the loss of the predicate's margins);
the index function agrees with a brute-force interval search and is monotone; no slot word reads as `triangle`, `nothing` or 0; a pixel without
a slot keeps 0; the plane's bookkeeping holds the tables and the threshold policy; and the tables are not vacuous.  Nothing here runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_primary_cull import sanitized
from test_primary_entry import F, NOTHING, SCENE_NAMES, scenes, wide_cone_cameras
from test_subtree_cull import cameras, flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene_file(rt, tmp_path, name, objs):
    """tests/test_primary_entry.py's file with four views: the default one at 128x72 and at 5x3, a two-degree field of view, a camera close to the
    surface (64 sub-cones per table pixel make a view cost what 64 views of the entry words' test do)"""
    _so, blob, info = flat(rt, objs)
    assert info["num_meshes"] == 1
    views = [cameras(rt, 128, 72)[0], cameras(rt, 5, 3)[0]] + wide_cone_cameras(rt)
    path = str(tmp_path / (name.replace(" ", "_") + ".bin"))
    with open(path, "wb") as f:
        f.write(np.array([info["blob_f4"], info["off_nodes"], info["num_nodes"], info["off_meshes"], info["off_tris"], info["num_triangles"], len(views)], np.int32).tobytes())
        f.write(blob.astype(F).tobytes())
        for c in views:
            f.write(np.asarray(c.floats(), F).tobytes())
            f.write(np.array([c.c.width, c.c.height], np.int32).tobytes())
    return path, len(views)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return sanitized(tmp_path_factory.mktemp("subentry_soundness"), "subentry_soundness.cpp")


def run(program, *args, timeout=600):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "sanitizers silent" in r.stdout, (args, (r.stderr or r.stdout)[-3000:])
    print(r.stdout.strip())
    return r.stdout


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_start_from_a_sub_word_ends_where_the_traversal_does(rt, tmp_path, program, name):
    """4 views (128x72 and 5x3, a two-degree field of view, a camera close to the surface), jittered: every table pixel, every sub-box with
    a non-zero word, at the 27 points of the sub-box (its ends are the thresholds -J/2, 0, J/2 and +-J, so each is held against both
    neighbouring sub-boxes' words), at -0.0f and at 8 random jitters, each also against the word the index function picks for it"""
    path, views = scene_file(rt, tmp_path, name, scenes(rt)[name])
    assert views == 4
    out = run(program, "scene", path, 1, 8, timeout=900)
    assert "no counter-example" in out and "over %d views" % views in out, out
    rays = int(out.split("subentry soundness: ")[1].split(" rays")[0])
    if name in ("monkey", "coplanar", "soup of 200"):
        assert rays > 10000, (name, "the scene has table pixels with resolved sub-boxes, so the check has rays to walk", out)
    if name == "box faces":
        assert rays == 0, out


def test_the_program_finds_the_loss_of_the_margins(tmp_path, program):
    """adversarial triangles and boxes at the corners of sub-cones: none is a counter-example with the header's margins; built with
    RT_ENTRY_E = 0 the same program finds one"""
    out = run(program, "adversarial", 1, 300000, timeout=300)
    assert "no counter-example" in out
    exe = str(tmp_path / "subentry_soundness_e0")
    cmd = [shutil.which("g++"), "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRT_ENTRY_E=0.0", "-I",
           os.path.join(ROOT, "ray-tracer_amd", "csrc"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "subentry_soundness.cpp"), "-o", exe]
    assert subprocess.run(cmd, capture_output=True, text=True, timeout=600).returncode == 0
    found = [subprocess.run([exe, "adversarial", str(seed), "300000"], capture_output=True, text=True, timeout=300) for seed in (1, 2, 3)]
    assert all(r.returncode == 1 and "UNSOUND" in r.stderr for r in found), [(r.returncode, r.stderr[-300:]) for r in found]


def test_the_index_agrees_with_a_brute_force_interval_search(program):
    """every float within 4096 ulp of each threshold and of +-J, -0.0f, and two million values over rt_jitter's range: the index names a closed
    sub-interval that holds the jitter and is monotone; the centre of sub-box (jx, jy, jz) has the index jx + 4 jy + 16 jz"""
    run(program, "index")


def test_no_slot_word_reads_as_triangle_nothing_or_zero(program):
    """the encoding (slot + 1) << 2 | 2 and the regions behind the entry words; only an unflagged pixel whose word is 0 wants a table"""
    run(program, "encoding")


def test_a_pixel_without_a_slot_keeps_zero(rt, tmp_path, program):
    """the compaction and the refinement replayed on a host array of the allocation's size, with cap forced to 0 and to 1"""
    path, _ = scene_file(rt, tmp_path, "monkey", scenes(rt)["monkey"])
    run(program, "complete", path)
    # the host hook with the same caps: no table, one table - the first table pixel's
    objs = scenes(rt)["monkey"]
    cam = rt.Camera(128, 72)
    p_all, w_all, st = rt.primary_subentry_host(rt.SceneObjects(objs), cam, True)
    assert st["tables"] == st["pixels_wanting_table"] == p_all.size > 100 and (np.diff(p_all.astype(np.int64)) > 0).all()
    p0, w0, st0 = rt.primary_subentry_host(rt.SceneObjects(objs), cam, True, cap=0)
    assert p0.size == 0 and st0["tables"] == 0 and st0["pixels_wanting_table"] == p_all.size
    p1, w1, st1 = rt.primary_subentry_host(rt.SceneObjects(objs), cam, True, cap=1)
    assert p1.tolist() == [int(p_all[0])] and np.array_equal(w1[0], w_all[0])


def test_the_plane_bookkeeping_holds_the_tables_and_the_policy(program):
    """rt_cull_host::Plan: same view, changed view, scene revision, growth, refused tables (the plane alone is then asked for), a refused
    allocation; below the threshold no refinement, the first reuse refines once, at or above the threshold at once, switched off never, a view
    without jitter never, a refinement that failed computes the view again"""
    for seed in (1, 2):
        run(program, "plan", seed, timeout=120)


@pytest.mark.parametrize("name", ["monkey", "soup of 200", "5 triangles"])
def test_the_tables_are_only_for_pixels_whose_own_word_is_zero(rt, name):
    """table pixels are exactly the unflagged pixels with the entry word 0; `triangle`, `nothing` and flagged pixels have none; every sub-word is 0,
    `nothing` or a tagged triangle of the mesh; a view without jitter has no tables"""
    objs = scenes(rt)[name]
    cam = rt.Camera(37, 21)
    bits = rt.cull.plane_bits(rt.primary_cull_host(rt.SceneObjects(objs), cam, True)[0], 37, 21).reshape(-1)
    own, _ = rt.primary_entry_host(rt.SceneObjects(objs), cam, True)
    pixels, words, st = rt.primary_subentry_host(rt.SceneObjects(objs), cam, True)
    want = np.flatnonzero((bits == 0) & (own.reshape(-1) == 0))
    assert np.array_equal(pixels, want.astype(np.uint32)), name
    nz = words[(words != 0) & (words != NOTHING)]
    assert (nz & 1).all() and ((nz >> 1) < flat(rt, objs)[2]["num_triangles"]).all()
    assert st["sub_triangle"] == nz.size and st["sub_nothing"] == int((words == NOTHING).sum()) and st["sub_unknown"] == int((words == 0).sum())
    p_off, _, st_off = rt.primary_subentry_host(rt.SceneObjects(objs), cam, False)
    assert p_off.size == 0 and st_off["pixels_wanting_table"] == 0


def test_the_sub_words_resolve_a_share_of_the_open_pixels(rt):
    """the floor, so that empty tables cannot pass: three quarters of what the host hook measures.
    Monkey at 128x72: 597 table pixels, 67.65 % of their sub-boxes resolved, 66.05 % weighted by the centre ray's gated node steps: floors 0.507
    and 0.495.  Monkey at 128x72 with a two-degree field of view (fov = 0.035: a cone spans several pixels): 4,871 pixels want a table, the 1,152
    the image's allocation holds get one; 70.28 % and 70.20 %: floors 0.527 and 0.526.  (At 1920x1080 with every 6th pixel the design's own run
    gave 70.3 % and 69.1 %.)"""
    objs = scenes(rt)["monkey"]
    for cam, floor, floor_w in ((rt.Camera(128, 72), 0.507, 0.495), (rt.Camera(128, 72, fov=0.035), 0.527, 0.526)):
        _p, _w, st = rt.primary_subentry_host(rt.SceneObjects(objs), cam, True)
        total = st["sub_triangle"] + st["sub_nothing"] + st["sub_unknown"]
        share, weighted = (st["sub_triangle"] + st["sub_nothing"]) / total, st["centre_steps_resolved"] / st["centre_steps_all"]
        print(st, "resolved %.4f step-weighted %.4f" % (share, weighted))
        assert st["tables"] > 100 and total == 64 * st["tables"]
        assert share >= floor and weighted >= floor_w, (share, weighted)
        assert st["sub_triangle"] > 0
