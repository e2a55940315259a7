"""The primary entry words on the CPU (ray-tracer_amd/csrc/rt_entry.h): for a pixel whose word is `triangle T` or `nothing` the kernel's float
traversal from the root and the start from the word end with the same (w_prim, w_best) bits (tests/sanitize/entry_soundness.cpp, under
AddressSanitizer + UndefinedBehaviorSanitizer, which also shows that it finds the loss of the predicate's margins), the words have the layout
the kernel reads, a flagged pixel has the word 0, the plane's bookkeeping holds the third region, and the words are not vacuous on the monkey.
That RT_AMD_PRIMARY_ENTRY=0 writes zeros is checked where a context can be made, in tests/test_gpu_primary_entry.py.  Nothing here runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

from test_primary_cull import estimate_tool, sanitized
from test_subtree_cull import GREY, GROUND, SIZES, cameras, flat, scenes as gate_scenes

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTHING = 2


def grid(nx, ny, z=1.5, x0=-0.5, x1=0.7, y0=-0.5, y1=0.5, tilt=0.0):
    """nx x ny quads of two triangles each, coplanar neighbours sharing every edge; tilt = 0: the plane z = const, so every leaf's box is flat and its
    triangles lie in a face of it"""
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    tris = []
    for i in range(nx):
        for j in range(ny):
            p = [(xs[i + a], ys[j + b], z + tilt * (xs[i + a] + 0.5 * ys[j + b])) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
            tris.append(p[0] + p[1] + p[2])
            tris.append(p[0] + p[2] + p[3])
    return np.array(tris, F)


def slivers(seed, n):
    """thin triangles: a long edge and a height of a thousandth of it, fanned around the view's centre"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = np.array((0.1, 0.0, 1.5)) + rng.normal(0, 0.15, 3)
        e = rng.normal(0, 0.3, 3)
        h = np.cross(e, rng.normal(0, 1, 3))
        h *= 1e-3 * np.linalg.norm(e) / (np.linalg.norm(h) + 1e-12)
        out.append(np.concatenate([c - e / 2, c + e / 2, c + h]))
    return np.array(out, F)


def shells():
    """two nested sheets a few ulp apart: the tilted grid and a copy of it moved by three ulp towards the camera"""
    a = grid(6, 5, tilt=0.2)
    b = a.copy()
    for _ in range(3):
        b[:, 2::3] = np.nextafter(b[:, 2::3], F(-np.inf))
    return np.concatenate([a, b])


def scenes(rt):
    """the subtree cull's scenes - the monkey, a 200-triangle soup, meshes of 1, 3, 5 and 12 triangles - and the adversarial ones"""
    out = dict(gate_scenes(rt))
    out["slivers"] = [("mesh", slivers(5, 60), GREY), GROUND]
    out["coplanar"] = [("mesh", grid(7, 5, tilt=0.3), GREY), GROUND]
    out["shells"] = [("mesh", shells(), GREY), GROUND]
    out["box faces"] = [("mesh", grid(6, 4), GREY), GROUND]
    return out


SCENE_NAMES = ["monkey", "soup of 200", "1 triangles", "3 triangles", "5 triangles", "12 triangles", "slivers", "coplanar", "shells", "box faces"]


def wide_cone_cameras(rt):
    """views whose jitter cone spans many pixels: a field of view of about two degrees, and a camera close to the surface"""
    return [rt.Camera(128, 72, fov=0.035), rt.Camera(128, 72, pos=(0.1, 0.0, 1.1), fov=0.3)]


def scene_file(rt, tmp_path, name, objs):
    _so, blob, info = flat(rt, objs)
    assert info["num_meshes"] == 1
    views = [c for w, h in SIZES for c in cameras(rt, w, h)] + wide_cone_cameras(rt)
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
    return sanitized(tmp_path_factory.mktemp("entry_soundness"), "entry_soundness.cpp")


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_start_from_the_word_ends_where_the_traversal_does(rt, tmp_path, program, name):
    """10 views (8 at 128x72 and 5x3, a two-degree field of view, a camera close to the surface), antialias on and off: every pixel with a non-zero
    word at the 27 corners, edges, face centres and centre of the jitter cube and 8 random draws; flagged pixels have the word 0; a non-zero word
    is `nothing` or a tagged triangle of the mesh"""
    path, views = scene_file(rt, tmp_path, name, scenes(rt)[name])
    assert views == 10
    r = subprocess.run([program, "scene", path, "1", "8"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no counter-example, sanitizers silent" in r.stdout, (name, (r.stderr or r.stdout)[-3000:])
    assert "over %d views" % views in r.stdout, r.stdout
    print(r.stdout.strip())
    rays = int(r.stdout.split("entry soundness: ")[1].split(" rays")[0])
    if name in ("monkey", "coplanar", "soup of 200"):
        assert rays > 10000, (name, "the scene resolves pixels, so the check has rays to walk", r.stdout)
    if name == "box faces":
        # (a flat box is entered by no ray - tmin < tmax fails - so the kernel never sees this mesh, and the predicate may not say otherwise)
        assert rays == 0, r.stdout


def test_the_program_finds_the_loss_of_the_margins(tmp_path, program):
    """adversarial triangles and boxes: none is a counter-example with the header's margins; built with RT_ENTRY_E = 0 the same program finds one"""
    r = subprocess.run([program, "adversarial", "1", "300000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no counter-example, sanitizers silent" in r.stdout, (r.stderr or r.stdout)[-3000:]
    import shutil
    gxx = shutil.which("g++")
    exe = str(tmp_path / "entry_soundness_e0")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRT_ENTRY_E=0.0", "-I",
           os.path.join(ROOT, "ray-tracer_amd", "csrc"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "entry_soundness.cpp"), "-o", exe]
    assert subprocess.run(cmd, capture_output=True, text=True, timeout=600).returncode == 0
    found = [subprocess.run([exe, "adversarial", str(seed), "300000"], capture_output=True, text=True, timeout=300) for seed in (1, 2, 3)]
    assert all(r.returncode == 1 and "UNSOUND" in r.stderr for r in found), [(r.returncode, r.stderr[-300:]) for r in found]


def test_the_plane_bookkeeping_holds_the_entry_words(program):
    """rt_cull_host::Plan with the allocation of rt_cull_alloc_words_entry: same and changed view, scene revision, growth, allocation failure;
    every run writes the three regions as the pre-pass does"""
    for seed in (1, 2):
        r = subprocess.run([program, "plan", str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "sanitizers silent" in r.stdout, (seed, (r.stderr or r.stdout)[-3000:])


@pytest.mark.parametrize("name", ["monkey", "soup of 200", "5 triangles", "box faces"])
def test_the_words_have_the_layout_the_kernel_reads(rt, name):
    """bit 0 tags `triangle T` (T << 1 | 1, T a triangle of the mesh), `nothing` is 2, a flagged pixel has 0; a camera that looks away has 0
    everywhere; without antialias the words are computed too"""
    objs = scenes(rt)[name]
    _so, _blob, info = flat(rt, objs)
    for antialias in (True, False):
        for cam in (rt.Camera(37, 21), rt.Camera(37, 21, rot=(0.0, float(np.pi), 0.0))):
            bits = rt.cull.plane_bits(rt.primary_cull_host(rt.SceneObjects(objs), cam, antialias)[0], 37, 21)
            words, st = rt.primary_entry_host(rt.SceneObjects(objs), cam, antialias)
            assert words.shape == (21, 37)
            assert (words[bits == 1] == 0).all(), (name, "flagged pixels have entry word 0")
            nz = words[(words != 0) & (words != NOTHING)]
            assert (nz & 1).all() and ((nz >> 1) < info["num_triangles"]).all(), name
            assert st["pixels_triangle"] == nz.size and st["pixels_nothing"] == int((words == NOTHING).sum())
        assert bits.all() and not words.any(), "the camera looks away: every pixel is flagged, every word is 0"
    if name == "monkey":
        w, _ = rt.primary_entry_host(rt.SceneObjects(objs), rt.Camera(37, 21), True)
        assert ((w & 1) == 1).sum() > 20, (name, "the default view resolves pixels to a triangle")


def test_the_entry_words_resolve_a_share_of_the_monkeys_pixels(rt):
    """the floor: at 128x72 at least 43 % of the monkey's unflagged root-entering pixels have a non-zero entry word.  Measured 64.6 % (679
    `triangle`, 410 `nothing`, 597 not known of 1,686; they carry 57.2 % of those pixels' gated centre-ray node steps); the floor is two
    thirds of that.  A binary64 brute force over 27 directions per pixel bounds what any sound predicate can reach at about 75 %."""
    st = estimate_tool().estimate("monkey", 128, 72, True)
    print(st)
    px = st["entry_pixels_triangle"] + st["entry_pixels_nothing"] + st["entry_pixels_unknown"]
    assert px == st["root_entering"] - st["flagged_root_entering"] > 1000, st
    assert st["entry_resolved_share"] >= 0.43, st
    assert st["entry_pixels_triangle"] > 0 and st["entry_pixels_nothing"] > 0, st
    assert 0.0 < st["entry_step_share_removed"] < 1.0 and 0.0 < st["entry_test_share_removed"] < 1.0, st
