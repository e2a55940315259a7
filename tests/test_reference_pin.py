"""Pins the CPU oracle to frames, hit records and intermediates the REFERENCE ITSELF produced.

tests/golden/ref/ holds what the reference's own sources computed when oracle/ref_build.py compiled them for the CPU
(tools/make_reference_golden.py; compiler, flags and glibc in meta.json).  The oracle's LIBM mode - the same restatement
as the DET mode the HIP kernel equals, bound to the platform libm as the reference's CPU build is - must reproduce every
one of them bit for bit.  Like the frame pins of test_oracle_pin.py these depend on glibc's logf / cosf / tanf bits and
skip, loudly, on another libm.

Where oracle/_ref is built (a reference checkout was there when build() ran) the second half regenerates the fixtures,
reproduces SURVEY.md App. C.2's hashes from the committed recipe and runs randomised scenes through both sides.
"""
import ctypes as C
import filecmp
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import reference_fixtures as RF
from conftest import ROOT
from oracle import ref_build
from test_oracle_pin import libm_matches_survey_container

META = RF.meta()
OTHER_LIBM = "platform libm differs from the glibc 2.35 the fixtures were recorded with"
NO_BINARIES = "oracle/_ref is not built: build() found no reference checkout (RT_REFERENCE_DIR) on this machine"


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def libm_ok(orc):
    if not libm_matches_survey_container(orc):
        pytest.skip(OTHER_LIBM)


def test_fixture_files_are_the_recorded_ones_and_small():
    """every file's sha256 as meta.json recorded it; none above the largest fixture committed before (196,736 bytes)"""
    for name, sha in META["sha256"].items():
        assert hashlib.sha256(np.ascontiguousarray(RF.load(name)).tobytes()).hexdigest() == sha, name
        assert os.path.getsize(os.path.join(RF.REF, name)) <= 196736, name
    assert META["libc"] == "glibc 2.35" and "-ftrivial-auto-var-init=zero" in META["flags"]


def test_det_mode_stays_within_the_cap_the_issue_sets():
    """conditions on the fixtures, checked when they were generated: DET mode differs from no reference frame in more than
    3 of 3,072 pixels, and from the three config scenes' frames in none"""
    for name, e in META["frames"].items():
        assert all(d["pixels"] <= 3 for d in e["det_vs_reference"]), name
    for name in ("three_sphere", "cube", "monkey"):
        assert [d["pixels"] for d in META["frames"][name]["det_vs_reference"]] == [0], name


# ---- frames ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(META["frames"]))
def test_frame_equals_oracle_libm(orc, rt, models_dir, libm_ok, name):
    """the oracle's LIBM mode, given the fixture's 12 camera floats and scene (scenes 0-3: rt.scenes' transcription of
    src/main.cu, against frames of the reference's OWN SceneObjects(n)), renders the reference's frame bit for bit; a
    progressive fixture is rendered as the chain it is, each frame fed the one before"""
    e = META["frames"][name]
    objs, sky = RF.scene(rt, e)
    assert list(sky) == e["sky"]
    sc = orc.Scene(objs, orc.MATH_LIBM, models_dir)
    cam = np.asarray(e["camera"], np.float32)
    prev = None
    for k, (t, ref) in enumerate(zip(e["time_ms"], RF.frames(e))):
        prev = sc.render(cam, e["W"], e["H"], e["spp"], e["limit"], sky, time_ms=t, frame_num=k, antialias=e["antialias"], prev=prev)
        differing = int((u32(prev) != u32(ref)).any(axis=2).sum())
        assert differing == 0, (name, k, differing)


def test_frame_fixtures_cover_what_they_claim():
    f = META["frames"]
    assert [f["builtin%d" % n]["builtin"] for n in range(4)] == [0, 1, 2, 3]
    assert len(f["progressive"]["time_ms"]) == 3 and len(set(f["progressive"]["time_ms"])) == 3
    assert f["no_antialias"]["antialias"] is False and (f["limit1_spp1"]["spp"], f["limit1_spp1"]["limit"]) == (1, 1)
    assert f["negative_time"]["time_ms"][0] < 0 and f["refraction"]["limit"] == 8
    n = sorted(o[-1][2] for o in META["scenes"]["refraction"]["objects"] if o[-1][0] == "refractive" and o[0] == "sphere")
    assert n == [0.5, 1.0, 1.5, 1.5, 2.0] and any(o[0] == "quad" and o[-1][0] == "refractive" for o in META["scenes"]["refraction"]["objects"])
    kinds = [o[0] for o in META["scenes"]["tie"]["objects"]]
    assert kinds.count("one_way_quad") == 2 and "cuboid" in kinds and "obj" in kinds
    assert all((e["W"], e["H"]) == (64, 48) for e in f.values())


# ---- hit records ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(META["hits"]))
def test_hit_records_equal_trace_one(orc, rt, models_dir, libm_ok, name):
    """get_ray_collision's record for 2,048 primary and 2,048 random rays (256 of them axis-parallel) against the oracle's:
    the hit flag and the distance of every ray; point, normal and object of every hit; the texture coordinates of every hit
    whose material has need_uv.  Elsewhere the reference never assigns texture_uv (src/objects.cu:68, :160) - the value is
    whatever the stack held - so it is not compared there, nor are a miss's point and normal."""
    e = META["hits"][name]
    objs, _ = RF.scene(rt, e)
    sc = orc.Scene(objs, orc.MATH_LIBM, models_dir)
    rec = RF.records(e)
    o, d = RF.rays()
    assert rec.shape == (4096, 11) and 0.25 <= e["hit_fraction"] <= 0.9
    got_hit = np.zeros(len(o), bool)
    got = np.zeros((len(o), 10), np.float32)
    for i in range(len(o)):
        got_hit[i], got[i] = sc.trace_one_uv(o[i], d[i])
    h = rec[:, RF.HIT] != 0
    assert np.array_equal(got_hit, h)
    assert np.array_equal(u32(got[:, 0]), rec[:, RF.DIST])
    assert np.array_equal(u32(got[h, 1:4]), rec[h, RF.POINT]) and np.array_equal(u32(got[h, 4:7]), rec[h, RF.NORMAL])
    assert np.array_equal(got[h, 7].astype(np.int32), rec[h, RF.OBJECT].view(np.int32))
    uv = h.copy()
    uv[h] = RF.need_uv(objs)[rec[h, RF.OBJECT].view(np.int32)]
    assert np.array_equal(u32(got[uv, 8:10]), rec[uv, RF.UV])
    print("%s: %d hits, texture coordinates compared on %d of them" % (name, int(h.sum()), int(uv.sum())))
    if name in ("builtin0", "refraction", "tie"):
        assert uv.sum() > 100, name          # checkerboard floor quad / ground sphere / quad: the UV paths are exercised


def test_tie_scene_has_ties_and_the_later_object_wins():
    """The fixture's rays do meet the coincident spheres and the coplanar quads, and the reference kept the later object's
    MATERIAL.  get_ray_collision's record names no object: the driver writes the one with the winning distance whose material
    equals the record's hit_mesh_material, and the tied objects of this scene all differ in colour, so for every one of the
    rays with a distance tie the object column is the reference's own choice, not a rule the driver applied
    (object_not_singled_out_by_material is 0 for this fixture).  The tie FRAME is the other evidence, through the colours."""
    e = META["hits"]["tie"]
    assert e["distance_ties"] > 40 and e["object_not_singled_out_by_material"] == 0
    rec = RF.records(e)
    ob = rec[rec[:, RF.HIT] != 0, RF.OBJECT].view(np.int32)
    counts = np.bincount(ob, minlength=9)
    assert counts[1] == 0 and counts[2] > 20 and counts[3] == 0 and counts[4] > 20      # `<=`: objects 2 and 4 shadow 1 and 3
    assert counts[5] > 0 and counts[6] > 0 and counts[7] > 0 and counts[8] > 0          # both one-way quads, cuboid, flat cube


# ---- intermediates --------------------------------------------------------------------------------------------

def test_camera_floats(orc, libm_ok):
    assert sorted(META["cameras"]) == ["1920x1080", "256x256", "3840x2160", "64x48"]
    for size, floats in META["cameras"].items():
        w, h = (int(v) for v in size.split("x"))
        assert np.array_equal(u32(orc.camera_default(w, h, orc.MATH_LIBM)), u32(floats)), size
    for name, e in META["frames"].items():
        assert e["camera"] == META["cameras"]["64x48"], name


@pytest.mark.parametrize("name", ["cube", "monkey"])
def test_transformed_triangles_and_bvh(orc, rt, models_dir, libm_ok, name):
    """ObjFileMesh's transforms (libm sin / cos) and the reference's tree, node for node in its array order: boxes, children,
    triangle counts and every node's triangle index list - which pins the merge sort's order on equal keys (SURVEY.md
    App. A.10), beyond the leaf-size histogram test_oracle_pin.py checks"""
    m = META["meshes"][name]
    objs, _ = RF.scene(rt, {"builtin": None, "scene": m["scene"]})
    kind, fname, transforms, _ = objs[m["object"]]
    assert kind == "obj"
    ob = orc.Obj(os.path.join(models_dir, fname), orc.MATH_LIBM)
    for t in transforms:
        getattr(ob, t[0])(*t[1:])
    assert np.array_equal(u32(ob.triangles()), u32(RF.load(m["triangles"])))
    tree = orc.Scene(objs, orc.MATH_LIBM, models_dir).bvh_dump(m["object"])
    links = RF.load(m["links"])
    assert m["nodes"] == 2047 and tree["root"] == m["root"]
    assert np.array_equal(tree["left"], links[:, 0]) and np.array_equal(tree["right"], links[:, 1]) and np.array_equal(tree["count"], links[:, 2])
    assert np.array_equal(tree["list"], RF.load(m["list"]))
    assert np.array_equal(u32(tree["boxes"]), u32(RF.load(m["boxes"])))


def test_bvh_fixture_has_equal_keys():
    """the tree fixtures can tell a stable merge from the reference's: some node's split met equal sort keys (the cube's 12
    triangles start at 8 vertices, so first vertices - the key's only input - repeat)"""
    tris = RF.load(META["meshes"]["cube"]["triangles"]).reshape(-1, 3, 3)
    first = [tuple(t[0]) for t in tris]
    assert len(set(first)) < len(first)


def test_rgba8(orc, rt, tmp_path):
    """parse_pixel_colours' bytes for a frame with values above 1 and exactly 0 against every float -> 8-bit conversion here
    that needs no GPU: the oracle's, the C++ mirror's rtamd::parse_pixel_colours (host/raytracer.hpp, compiled with g++ as
    tests/test_png.py does) and the float path of save_png"""
    e = META["frames"]["monkey"]
    frame = np.ascontiguousarray(RF.frames(e)[-1])
    assert (frame > 1).any() and (frame == 0).any()
    want = RF.load(e["rgba8"])
    assert (want[..., 3] == 255).all() and want[..., :3].max() == 255 and want[..., :3].min() == 0
    got = np.zeros_like(want)
    orc.lib().orc_to_rgba8(frame.ctypes.data_as(C.POINTER(C.c_float)), e["W"], e["H"], got.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert np.array_equal(got, want)
    # the C++ mirror
    src = tmp_path / "rgba8.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "raytracer.hpp"\n'
                   'int main(int argc, char **argv) { int w = atoi(argv[1]), h = atoi(argv[2]); std::vector<float> f((size_t)w * h * 3);\n'
                   '  FILE *in = fopen(argv[3], "rb"); if (!in || fread(f.data(), 4, f.size(), in) != f.size()) return 1; fclose(in);\n'
                   '  std::vector<uint8_t> px = rtamd::parse_pixel_colours(f, w, h);\n'
                   '  FILE *out = fopen(argv[4], "wb"); if (!out || fwrite(px.data(), 1, px.size(), out) != px.size()) return 1; fclose(out); return 0; }\n')
    exe = tmp_path / "rgba8"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "ray-tracer_amd", "host"), str(src), "-o", str(exe)])
    frame.tofile(str(tmp_path / "frame.f32"))
    subprocess.check_call([str(exe), str(e["W"]), str(e["H"]), str(tmp_path / "frame.f32"), str(tmp_path / "rgba.u8")])
    assert np.array_equal(np.fromfile(str(tmp_path / "rgba.u8"), np.uint8).reshape(want.shape), want)
    # save_png's float path
    from test_png import decode_png
    rt.save_png(str(tmp_path / "frame.png"), frame)
    assert np.array_equal(decode_png(tmp_path / "frame.png"), want[..., :3])


# ---- with the reference's programs present -------------------------------------------------------------------

needs_binaries = pytest.mark.skipif(not ref_build.available(), reason=NO_BINARIES)


@needs_binaries
def test_fixtures_are_what_the_recipe_produces_today(tmp_path):
    """regenerate every fixture and compare with the committed file byte for byte"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_reference_golden as G
    G.generate(str(tmp_path), verbose=False)
    names = sorted(os.listdir(RF.REF))
    assert sorted(os.listdir(str(tmp_path))) == names
    match, mismatch, errors = filecmp.cmpfiles(RF.REF, str(tmp_path), names, shallow=False)
    assert not mismatch and not errors


SURVEY_C2 = [("three_sphere", 4, "479589c110c5b34e", 0.472370008), ("cube", 8, "b4dcdd058b1bc676", 0.650935728), ("monkey", 8, "24682f69ae058766", 0.19924736)]


@needs_binaries
@pytest.mark.parametrize("name,limit,sha,mean", SURVEY_C2, ids=[c[0] for c in SURVEY_C2])
def test_recorded_hashes_from_the_reference_binary(rt, libm_ok, name, limit, sha, mean):
    """SURVEY.md App. C.2 (256x256, 16 spp, time_ms 12345) from the committed recipe - with -ftrivial-auto-var-init=zero,
    which therefore changes none of the three"""
    from oracle import ref_driver
    objs, sky = rt.scenes.CONFIG_SCENES[name]()
    job = ref_driver.Job(256, 256)
    job.scene(objs)
    job.settings(16, limit, True, sky)
    k = job.render(12345)
    img = job.run()[k]
    assert hashlib.sha256(img.tobytes()).hexdigest()[:16] == sha
    assert float("%.9g" % img.mean(dtype=np.float64)) == mean


@needs_binaries
def test_reference_binary_is_deterministic_across_thread_counts(rt):
    from oracle import ref_driver
    out = []
    for threads in (1, 16):
        job = ref_driver.Job(64, 48, threads=threads)
        job.builtin(0)
        job.settings(4, 5, True)
        a, b = job.render(4242), job.render(4243)
        res = job.run()
        out.append((res[a], res[b]))
    assert np.array_equal(u32(out[0][0]), u32(out[1][0])) and np.array_equal(u32(out[0][1]), u32(out[1][1]))
    assert not np.array_equal(out[0][0], out[0][1])


@needs_binaries
def test_data_file_mode_equals_the_reference_scene_builder(rt, libm_ok):
    """the driver's data-file mode and the reference's own SceneObjects(n) render the same frame from rt.scenes'
    description of scene n: the mode the other fixtures and the differential run rely on adds nothing of its own"""
    from oracle import ref_driver
    for n in range(4):
        frames = []
        for builtin in (True, False):
            job = ref_driver.Job(64, 48)
            objs, sky = rt.scenes.CONFIG_SCENES["reference_scene%d" % n]()
            if builtin:
                job.builtin(n, rt.scenes.procedural_image())
                job.settings(4, 5, True)
            else:
                job.scene(objs)
                job.settings(4, 5, True, sky)
            k = job.render(31337)
            frames.append(job.run()[k])
        assert np.array_equal(u32(frames[0]), u32(frames[1])), n


DIFFERENTIAL_SEEDS = [11, 12, 13, 14, 15, 16] + list(range(101, 115))


@needs_binaries
@pytest.mark.parametrize("seed", DIFFERENTIAL_SEEDS)
def test_random_scenes_oracle_libm_equals_the_reference(orc, rt, models_dir, libm_ok, seed):
    """tests/test_gpu_parity.py's seeded mix of every primitive and material kind (its six seeds and 14 more), 64x48, 4 spp:
    the reference's program in data-file mode against the oracle's LIBM mode, bit for bit"""
    from oracle import ref_driver
    from test_gpu_parity import _random_scene
    objs, sky = _random_scene(seed)
    limit = 3 + seed % 6
    job = ref_driver.Job(64, 48)
    job.scene(objs)
    job.settings(4, limit, True, sky)
    k, c = job.render(1000 + seed), job.camera()
    res = job.run()
    want = orc.Scene(objs, orc.MATH_LIBM, models_dir).render(res[c], 64, 48, 4, limit, sky, time_ms=1000 + seed)
    differing = int((u32(res[k]) != u32(want)).any(axis=2).sum())
    assert differing == 0, (seed, differing)
