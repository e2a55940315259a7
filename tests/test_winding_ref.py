"""The winding-number yardstick (tests/winding_ref.py) held to account without a GPU:
  - its orientation against binary64 winding numbers computed straight from the .obj fixtures with quads fanned consistently - nothing of
    the product's flip bits - on the cube (at its centre and outside) and the monkey (three interior points, a far one), and the same sum
    with every flip cleared, which must FAIL to enclose the cube's centre: the bit matters;
  - the flip bytes debug_flatten() reports against the construction: the second triangle of every quad face, nothing else;
  - the cuboid rule against the constructor's arguments on reference_scene0;
  - its accuracy: |w32 - w64| <= k * 2^-24 over the uniform points at least 1e-3 of the triangle-bounds diagonal from the surface, k from
    tests/golden/winding_meta.json (python tests/winding_ref.py measured it: four times the worst ratio seen), the share left out capped;
  - its constants against the header's text, and the ABI table against the header on the four new entry points."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import nearest_ref as NR
import winding_ref as W
from conftest import ROOT
from random_scenes import random_scene

META = json.load(open(W.META))


def obj_faces(path):
    """(vertices [n, 3] float64, faces as lists of 0-based indices) of a Wavefront file: v and f lines, the index before any slash"""
    verts, faces = [], []
    for line in open(path):
        t = line.split()
        if t and t[0] == "v":
            verts.append([float(x) for x in t[1:4]])
        elif t and t[0] == "f":
            faces.append([int(x.split("/")[0]) - 1 for x in t[1:]])
    return np.array(verts, np.float64), faces


def fan(faces):
    """every face as triangles (f0, f_i, f_i+1): one orientation per face"""
    return [(f[0], f[i], f[i + 1]) for f in faces for i in range(1, len(f) - 1)]


def as_stored(faces):
    """... and as the library's records turn: a quad's second triangle is (f0, f3, f2)"""
    out = []
    for f in faces:
        out.append((f[0], f[1], f[2]))
        if len(f) == 4:
            out.append((f[0], f[3], f[2]))
    return out


def winding_of(verts, tris, p):
    """binary64 generalized winding number of the triangles (vertex index triples) at the points p [n, 3]"""
    A = np.zeros(p.shape[0])
    for i, j, k in tris:
        a, b, c = verts[i] - p, verts[j] - p, verts[k] - p
        la, lb, lc = (np.sqrt((v * v).sum(axis=1)) for v in (a, b, c))
        det = (a * np.cross(b, c)).sum(axis=1)
        den = la * lb * lc + (a * b).sum(axis=1) * lc + (a * c).sum(axis=1) * lb + (b * c).sum(axis=1) * la
        A += np.arctan2(det, den)
    return A / (2 * np.pi)


def mesh_alone(rt, models_dir, file):
    return rt.SceneObjects([("obj", file, [], ("standard", (1, 1, 1), 0.0))], models_dir).debug_flatten()


def test_cube_orientation_and_that_the_flip_bit_matters(rt, models_dir):
    verts, faces = obj_faces(os.path.join(models_dir, "cube.obj"))
    assert len(faces) == 6 and all(len(f) == 4 for f in faces)
    centre = verts.mean(axis=0)
    p = np.array([centre, centre + 5.0 * (verts.max(axis=0) - verts.min(axis=0))])
    truth = winding_of(verts, fan(faces), p)
    assert abs(abs(truth[0]) - 1.0) < 1e-5 and abs(truth[1]) < 1e-5, truth
    assert abs(winding_of(verts, as_stored(faces), p)[0]) < 1e-5, "the records as stored cancel at the centre: the finding the flip bit answers"
    flat = mesh_alone(rt, models_dir, "cube.obj")
    assert flat["tri_flip"].sum() == 6 and flat["tri_flip"].shape == (12,)
    w = W.winding(flat, p.astype(np.float32), 0)
    assert abs(float(w[0]) - truth[0]) < 1e-5 and abs(float(w[1])) < 1e-5, (w, truth)
    same = W.winding(flat, p.astype(np.float32))
    assert same.tobytes() == w.tobytes()
    cleared = dict(flat, tri_flip=np.zeros_like(flat["tri_flip"]))
    assert abs(float(W.winding(cleared, p.astype(np.float32), 0)[0])) < 0.1, "with every flip cleared the cube's centre is not enclosed"


def test_monkey_orientation(rt, models_dir):
    verts, faces = obj_faces(os.path.join(models_dir, "low_poly_monkey.obj"))
    assert len(faces) == 723 and all(len(f) == 3 for f in faces)
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    mid = (lo + hi) / 2
    inner = np.array([mid, mid + 0.1 * (hi - lo) * [1, 0, 0], mid + 0.1 * (hi - lo) * [0, 1, 0]])
    p = np.concatenate([inner, [mid + 10.0 * (hi - lo)]])
    truth = winding_of(verts, fan(faces), p)
    assert (np.abs(truth[:3]) > 0.9).all() and (np.abs(truth[:3]) < 1.1).all() and abs(truth[3]) < 1e-3, truth
    flat = mesh_alone(rt, models_dir, "low_poly_monkey.obj")
    assert flat["tri_flip"].sum() == 0
    w = W.winding(flat, p.astype(np.float32), 0)
    assert np.abs(w.astype(np.float64) - truth).max() < 1e-4, (w, truth)
    assert (W.inside(w) == [1, 1, 1, 0]).all()


def test_flip_bytes_follow_the_construction(rt, models_dir):
    """a mesh given as triangles has none; a mesh from a file has one per quad face, on the record that came from its second triangle;
    records of objects that are not meshes have none"""
    rng = np.random.default_rng(3)
    soup = rng.normal(0, 1, (40, 9)).astype(np.float32)
    verts, faces = obj_faces(os.path.join(models_dir, "cube.obj"))
    objs = [("quad", (0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), ("standard", (1, 1, 1), 0.0)), ("mesh", soup, ("standard", (1, 1, 1), 0.0)),
            ("cuboid", (0, 0, 3), 1, 1, 1, ("standard", (1, 1, 1), 0.0)), ("obj", "cube.obj", [], ("standard", (1, 1, 1), 0.0))]
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    flip = flat["tri_flip"]
    assert flip.dtype == np.uint8 and flip.shape == (2 + 40 + 12 + 12,)
    assert flip[:54].sum() == 0, "a quad's, a triangle mesh's and a cuboid's records carry no flip byte"
    tris = NR.sections(flat)[2][54:66].astype(np.float64)
    # each record of the file's mesh is found among the stored triangles: flip says whether it is a quad's second one
    stored = as_stored(faces)
    for rec, f in zip(tris, flip[54:66]):
        corners = np.stack([rec[0:3], rec[0:3] + rec[3:6], rec[0:3] + rec[6:9]])
        hits = [k for k, t in enumerate(stored) if np.abs(verts[list(t)] - corners).max() < 1e-6]
        assert len(hits) == 1 and int(f) == hits[0] % 2, (hits, f)


def test_cuboid_rule_against_the_constructor(rt):
    objs = rt.scenes.CONFIG_SCENES["reference_scene0"]()[0]
    flat = rt.SceneObjects(objs).debug_flatten()
    found = 0
    for i, o in enumerate(objs):
        if o[0] != "cuboid":
            continue
        found += 1
        tl_near, w, h, d = np.float32(o[1]), np.float32(o[2]), np.float32(o[3]), np.float32(o[4])
        a = tl_near
        b = np.array([(tl_near[0] + w), (tl_near[1] - h), (tl_near[2] + d)], np.float32)
        lo, hi = W.cuboid_box(flat, i)
        assert lo.tobytes() == np.minimum(a, b).tobytes() and hi.tobytes() == np.maximum(a, b).tobytes(), (lo, hi, a, b)
        mid = ((lo + hi) / np.float32(2)).astype(np.float32)
        p = np.array([mid, lo, hi, [mid[0], mid[1], hi[2]], np.nextafter(hi, lo), mid + (hi - lo)], np.float32)
        assert W.winding(flat, p, i).tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        # summing its records instead would not do: the near and the far face are stored with the same orientation
        first = int(flat["objects"][i]["prim_start"])
        summed = sum(W.term32(NR.sections(flat)[2][k], p[:1]) * (-1 if k % 2 else 1) for k in range(first, first + 12)) * W.INV_2PI
        assert abs(float(summed[0])) < 0.9
    assert found >= 1


SCENES = ["cube", "monkey", "reference_scene0", "random13", "random15"]


@pytest.mark.parametrize("name", SCENES)
def test_accuracy_bound_away_from_the_surface(rt, name):
    objs = random_scene(int(name[6:]))[0] if name.startswith("random") else rt.scenes.CONFIG_SCENES[name]()[0]
    flat = rt.SceneObjects(objs).debug_flatten()
    n = 400
    pts = W.query_points(flat, 7, n)[:n]
    D, _ = NR.nearest64(flat, pts)
    keep = D >= W.NEAR * W.triangle_diagonal(flat)
    assert 1.0 - keep.mean() <= 0.02, (name, "share of the uniform points left to the byte comparison alone", 1.0 - keep.mean())
    w32, w64 = W.winding(flat, pts[keep]).astype(np.float64), W.winding64(flat, pts[keep])
    ratio = np.abs(w32 - w64).max() / 2.0 ** -24
    print("%s: worst |w32 - w64| = %.2f * 2^-24 over %d points (k = %.1f)" % (name, ratio, int(keep.sum()), META["k"]))
    assert ratio <= META["k"], (name, ratio, META["k"])
    assert META["k"] == 4.0 * META["worst_ratio"] and set(META["seeds"]) == set(W.META_SEEDS)


def test_constants_and_the_arctangent(rt):
    text = open(os.path.join(ROOT, "include", "rt_amd.h")).read()

    def macro(name):
        m = re.search(r"#define %s \(?(-?0x[0-9a-f.]+p[+-]?\d+)f\)?" % name, text)
        assert m, name
        return np.float32(float.fromhex(m.group(1)))
    for k in range(9):
        assert macro("RT_WN_C%d" % k) == W.COEFFS[k], k
    assert macro("RT_WN_PI") == W.PI == np.float32(np.pi) and macro("RT_WN_PI_2") == W.PI_2 == np.float32(np.pi / 2)
    assert macro("RT_INV_2PI") == W.INV_2PI == np.float32(1.0 / (2.0 * np.pi))
    assert re.search(r"#define RT_WINDING_SOLIDS \(-1\)", text) and rt.WINDING_SOLIDS == W.SOLIDS == -1
    # the arctangent: the quadrants, the axes, and the measured error the header states
    y = np.array([0.0, 1.0, 1.0, 1.0, 0.0, -1.0, -1.0, -1.0, 2.0, -3.0], np.float32)
    x = np.array([1.0, 1.0, 0.0, -1.0, -1.0, -1.0, 0.0, 1.0, 1.0, -0.5], np.float32)
    got = W.atan2_32(y, x).astype(np.float64)
    assert np.abs(got - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 6 * 2.0 ** -24
    assert W.atan2_error(1_000_000) <= META["atan2_error_ulp24"] + 0.01 <= 6.0


def test_winding_kernel_budget(rt, tmp_path):
    """the one winding kernel in the shipped library's code object: no spill, no scratch, few enough registers for eight waves per SIMD"""
    from test_query_abi import LLVM, kernel_notes
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools")
    notes = {n: v for n, v in kernel_notes(rt, tmp_path).items() if "rt_winding_kernel" in n}
    assert len(notes) == 1, sorted(notes)
    v = next(iter(notes.values()))
    print("rt_winding_kernel: %d VGPRs" % v["vgpr_count"])
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, v
    assert v["agpr_count"] == 0 and v["vgpr_count"] <= 64, v


def test_abi_table_and_header_agree_on_the_new_entry_points(rt):
    L = rt.lib()
    vp, fp, i64, i32 = C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.c_int32
    want = {"rt_winding_numbers_device": [vp, vp, vp, i64, i32, vp, vp, vp], "rt_winding_numbers": [vp, vp, fp, i64, i32, fp, vp],
            "rt_signed_distance_device": [vp, vp, vp, vp, i64, vp, vp, vp], "rt_signed_distance": [vp, vp, fp, fp, i64, vp, fp]}
    text = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    for name, argtypes in want.items():
        assert name in rt.ABI_SYMBOLS and getattr(L, name).argtypes == argtypes and getattr(L, name).restype == i32, name
        m = re.search(r"rt_status %s\(([^;]*)\);" % name, text)
        assert m and len(m.group(1).split(",")) == len(argtypes), name
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("winding_numbers", "winding_numbers_device", "contains_points", "signed_distance", "signed_distance_device", "signed_distance_grid"):
        assert callable(getattr(rt, name)), name
    # refused before HIP is touched: no GPU needed
    three = (C.c_float * 3)(0, 0, 0)
    one = (C.c_float * 1)(0)
    assert L.rt_winding_numbers(None, None, three, 1, -1, one, None) == rt.RT_ERR_INVALID
    assert L.rt_winding_numbers_device(None, None, None, 1, -1, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_signed_distance(None, None, three, None, 1, None, one) == rt.RT_ERR_INVALID
    assert L.rt_signed_distance_device(None, None, None, None, 0, None, None, None) == rt.RT_ERR_INVALID
