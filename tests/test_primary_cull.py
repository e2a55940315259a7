"""The primary-ray cull on the CPU (ray-tracer_amd/csrc/rt_cull.h): the predicate is sound against the slab test's three forms
(tests/sanitize/cull_soundness.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer), it is not vacuous on the monkey scene
(tools/primary_cull_estimate.py), the context's bookkeeping of the plane follows the view (tests/sanitize/cull_key_check.cpp), and the host
evaluation writes the plane's bits where the kernels read them.  The last section holds the inputs of tests/test_gpu_primary_cull_views.py (its
cameras, scenes and sizes, built by that file's own functions) to what its cases rely on, from the host predicate and the oracle alone, so that a
later change to a generator cannot quietly empty a case.  Nothing runs on a GPU."""
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
    """rt_capi.cpp calls rt_launch_cull like every other launcher of rt_launch.h: a library without the pre-pass kernel does not link, and
    the host programs of tests/sanitize/ link launcher_stubs.h's stand-in, which fails, so that they render without a plane.  The shipped
    library defines the launcher."""
    L = rt.lib()
    assert hasattr(L, "rt_launch_cull"), "libraytracer_amd.so does not define rt_launch_cull"


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


# ---------------------------------------------------------------- the inputs of tests/test_gpu_primary_cull_views.py

import test_gpu_primary_cull_views as views  # noqa: E402  (its top needs no GPU: cameras, scenes, sizes and check (c))


def view_bits(rt, name, antialias, models_dir):
    objs, _, cam12 = views.view(rt, name)
    words, st = rt.primary_cull_host(rt.SceneObjects(objs, models_dir), rt.Camera(views.W, views.H, floats=cam12), antialias)
    return rt.cull.plane_bits(words, views.W, views.H), st


def runs_the_traits_kernel(rt, objs, models_dir):
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    return flat["kernel_variant"] == "traits" and flat["traits"] == {"SPHERES_ONLY", "ONE_MESH", "PLAIN_MATERIALS"} and flat["num_meshes"] == 1


@pytest.mark.parametrize("antialias", [True, False], ids=["antialias", "no antialias"])
def test_the_sweep_of_views_is_not_empty(rt, models_dir, antialias):
    """at least 10 of the 14 random views have 50 or more rim pixels and at least 3 % of their pixels unflagged, and none has a plane that is
    all zero; the generator draws pos, rot, fov per view in that order from default_rng(2024)"""
    cams = views.sweep_cameras()
    assert len(cams) == views.N_SWEEP == 14 and len(set(cams)) == 14
    for pos, rot, fov in cams:
        assert all(-b <= p <= b for p, b in zip(pos[:2], (0.8, 0.5))) and -0.8 <= pos[2] <= 0.5 and all(abs(r) <= 0.3 for r in rot) and 0.6 <= fov <= 1.6
    good = 0
    for i in range(views.N_SWEEP):
        bits, _ = view_bits(rt, "view %d" % i, antialias, models_dir)
        rim, unflagged = int(views.rim_pixels(bits).sum()), 1.0 - bits.mean()
        print("view %d: %.1f %% flagged, %d rim pixels" % (i, 100 * bits.mean(), rim))
        assert bits.any(), ("view %d flags nothing" % i)
        good += rim >= 50 and unflagged >= 0.03
    assert good >= 10, good


def test_the_named_views_are_what_their_names_say(rt, models_dir):
    F = np.float32
    W, H = views.W, views.H
    for name in views.NAMED:
        assert runs_the_traits_kernel(rt, views.view(rt, name)[0], models_dir), name
    # axis-aligned: the central column's direction has x == 0 exactly, the central row's y == 0; the mesh has no thickness in z
    objs, _, cam12 = views.view(rt, "axis-aligned camera")
    P = views.primaries(cam12, W, H)
    assert not P[:, W // 2, 0].any() and not P[H // 2, :, 1].any() and P[:, W // 2 + 1, 0].all() and not cam12[0:3].any()
    tris = objs[0][1].reshape(-1, 3, 3)
    assert len(tris) >= 200 and np.all(tris[..., 2] == tris[0, 0, 2]) and np.ptp(tris[..., 0]) > 1 and np.ptp(tris[..., 1]) > 1
    assert objs[1][0] == "sphere" and objs[1][2] == 100
    bits, st = view_bits(rt, "axis-aligned camera", True, models_dir)
    assert st["root_entering"] > 1000 and 0 < int(bits.sum()) < W * H and int(views.rim_pixels(bits).sum()) >= 50
    # ... and over the scattered mesh the same camera flags pixels of the row with y == 0, next to pixels that see the mesh
    objs2, _, cam12b = views.view(rt, "axis-aligned camera, scattered mesh")
    assert np.array_equal(cam12b, cam12) and (objs2[0][1].reshape(-1, 3)[:, 0] == 0).mean() > 0.25 and (objs2[0][1].reshape(-1, 3)[:, 1] == 0).mean() > 0.25
    bits, st = view_bits(rt, "axis-aligned camera, scattered mesh", True, models_dir)
    assert bits[H // 2].any() and not bits[H // 2].all() and int(views.rim_pixels(bits).sum()) >= 50 and 0.03 < bits.mean() < 0.97
    # far: the whole mesh inside one or two pixels
    bits, st = view_bits(rt, "far camera", True, models_dir)
    assert 1 <= st["root_entering"] <= 2 and int(bits.sum()) >= W * H - 2
    # near: focal length 0.05, the camera outside the root box by a few centimetres, part of the image flagged and part not
    lo, hi = np.array(views.MONKEY_BOX[0]), np.array(views.MONKEY_BOX[1])
    blob = rt.SceneObjects(rt.scenes.monkey()[0], models_dir).debug_flatten()
    box = blob["blob"][blob["off_meshes"]:blob["off_meshes"] + 2].reshape(8)[:6]
    assert np.allclose(box, np.concatenate([lo, hi]), atol=1e-4), box
    pos = np.array(views.NEAR_POS)
    outside = np.maximum(np.maximum(lo - pos, pos - hi), 0)
    assert 0.01 <= np.linalg.norm(outside) <= 0.06, outside
    _, _, cam12 = views.view(rt, "near camera")
    centre = cam12[3:6] + cam12[6:9] * F(W / 2) + cam12[9:12] * F(H / 2) - cam12[0:3]
    assert abs(float(np.linalg.norm(centre)) - views.NEAR_FOCAL) < 1e-3, centre
    bits, st = view_bits(rt, "near camera", True, models_dir)
    assert 0.2 < bits.mean() < 0.8 and st["root_entering"] > 1000


def test_check_c_on_the_host_plane(rt, orc, models_dir):
    """the rim check of tests/test_gpu_primary_cull_views.py (a necessary condition, not a proof) on the host's planes of four random views and
    the two axis-aligned ones; and its convention: the oracle names the mesh by its place in the object list, which the centre rays of unflagged
    pixels of view 0 do report"""
    for name in ["view %d" % i for i in views.ORACLE_VIEWS] + ["axis-aligned camera", "axis-aligned camera, scattered mesh"]:
        objs, _, cam12 = views.view(rt, name)
        oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
        for antialias in (True, False):
            bits, _ = view_bits(rt, name, antialias, models_dir)
            bad, rays = views.mesh_winners(oracle, cam12, views.rim_pixels(bits), antialias, views.mesh_index(objs))
            assert rays >= 50 and not bad, (name, antialias, bad[:10])
        if name == "view 0":
            won, rays = views.mesh_winners(oracle, cam12, bits == 0, False, views.mesh_index(objs))
            assert len(won) > rays // 2 > 100, (len(won), rays)
    d = views.cone_directions(np.array([0.6, 0.0, 0.8], np.float32), True)
    assert d.shape == (9, 3) and d.dtype == np.float32 and len({tuple(x) for x in d}) == 9 and np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    assert views.cone_directions(np.array([0.6, 0.0, 0.8], np.float32), False).shape == (1, 3)


def test_the_placements_sizes_and_sequences_have_what_their_cases_need(rt, models_dir):
    # 2. the mesh's place: all five carry every trait, and the mesh is where the name says
    assert [views.mesh_index(views.place(w)) for w in views.PLACES] == [0, 1, 2, 0, 0]
    assert len(views.place("only")) == 1 and views.place("emissive")[0][-1][0] == "emissive"
    planes = []
    for where in views.PLACES:
        assert runs_the_traits_kernel(rt, views.place(where), models_dir), where
        planes.append(rt.primary_cull_host(rt.SceneObjects(views.place(where)), rt.Camera(views.W, views.H), True)[0])
    assert all(np.array_equal(planes[0], p) for p in planes), "the plane depends on the mesh alone"
    assert not runs_the_traits_kernel(rt, views.two_meshes(), models_dir)
    # 3. sizes: the word counts, ragged against 32 and 64, the host's tail clear
    objs, _ = rt.scenes.monkey()
    assert views.WORDS == {(5, 3): 2, (8, 8): 2, (13, 5): 4, (33, 2): 4, (65, 1): 4, (101, 67): 212} and sorted(views.WORDS) == sorted(views.SIZES)
    for w, h in views.SIZES:
        words, st = rt.primary_cull_host(rt.SceneObjects(objs, models_dir), rt.Camera(w, h), True)
        assert words.size == rt.cull.plane_words(w, h) == views.WORDS[(w, h)]
        assert not np.unpackbits(words.view(np.uint8), bitorder="little")[w * h:].any()
        assert 0 < st["flagged"] < w * h, (w, h, st)
    assert sum((w * h) % 32 != 0 for w, h in views.SIZES) >= 5 and all((w * h) % 64 != 0 for w, h in views.ID_SIZES[1:])
    # 5. bands and tile lists own part of the image, the list is shuffled and has no repeats
    for w, h in views.ID_SIZES:
        rows = views.band_rows_owned(h)
        assert rows == [y for y in range(h) if (y // 8) % 3 == 1] and len(rows) == 24
        tiles = views.random_tile_list(w, h)
        n = ((w + 7) // 8) * ((h + 7) // 8)
        assert n // 2 < tiles.size < n and np.unique(tiles).size == tiles.size and tiles.max() < n and not np.array_equal(tiles, np.sort(tiles))
        assert views.tile_mask(w, h, tiles).sum() > w * h // 2
    # 4. every sequence alternates between planes that differ (the GPU cases assert the same before they launch)
    W, H = views.W, views.H
    monkey = rt.SceneObjects(objs, models_dir)

    def plane(scene, cam, antialias=True):
        return rt.primary_cull_host(scene, cam, antialias)[0]
    cam_a, cam_b = rt.Camera(W, H), rt.Camera(W, H, pos=(0.6, 0.2, 0.3))
    assert not np.array_equal(plane(monkey, cam_a, True), plane(monkey, cam_a, False)), "antialias on and off"
    assert not np.array_equal(plane(monkey, cam_a), plane(monkey, cam_b)), "camera a and b"
    wide, tall = plane(monkey, rt.Camera(96, 64)), plane(monkey, rt.Camera(64, 96))
    assert wide.size == tall.size and not np.array_equal(wide, tall), "96 x 64 and 64 x 96"
    assert plane(monkey, rt.Camera(24, 16)).size < wide.size < plane(monkey, rt.Camera(192, 128)).size
    left, right = views.left_and_right()
    sa, sb = rt.SceneObjects([("mesh", left, views.GREY), views.GROUND]), rt.SceneObjects([("mesh", right, views.GREY), views.GROUND])
    assert runs_the_traits_kernel(rt, [("mesh", left, views.GREY), views.GROUND], models_dir)
    assert int((plane(sa, cam_a) != plane(sb, cam_a)).sum()) > 50, "mesh left and mesh right"
