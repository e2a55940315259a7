"""Every built kernel shape and every control path of the scheduling knobs against the CPU oracle, bit for bit.

The other GPU tests run whatever shape rt_sched::choose_shape picks for their scenes from the runtime's occupancy answers, at the default
knobs.  Here every entry of RT_SHAPES (parsed out of rt_device_scene.h: a shape added later without a way to reach it fails) is FORCED -
RT_AMD_THREADS and RT_AMD_SCENE_MODE, read when a scene is committed, or a scene of the size that needs it - and each case first asserts
from scene.info() that the shape under test is the one launched.  On that shape all five entry points run: the render kernel (one
frame, and six frames in one launch so that every wave refills its lanes mid-flight), closest-hit queries, the first-hit planes, occlusion
queries and the visibility plane.  The knob matrix renders with each RT_AMD_* knob (read when a context is created) at the values that
force one control path of the render kernel's wave loop; every value lies inside the accepted ranges, for which
tests/sanitize/capi_host_fuzz.cpp (check_progress) proves that the loop makes progress.

Tolerance: none.  Every comparison is uint32 / byte equality with oracle/ (MATH_DET).  One exception is named where it is made: the
albedo plane at unlit hits, compared with the plane of the scene's default shape.  The oracle's answers are computed once per scene and
shared by the cases.  Run with -m gpu on an MI355X."""
import functools
import os
import re

import numpy as np
import pytest

from test_gpu_occlusion import N_BASE, check_batch, oracle_hits, oracle_visibility
from test_gpu_parity import _random_scene, eq
from test_gpu_query import MISS_T, _rays, assert_equal_to_oracle, assert_triangles_and_uv, oracle_records, primaries, scene_rays, u32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 163840                  # RT_LDS_LIMIT (rt_schedule.h)
MODE_NAMES = {0: "global", 1: "lds", 2: "hybrid"}


def _parse_shapes():
    """RT_SHAPES' initialiser as [(has_mesh, mode, threads)], the RT_SCENE_* names resolved from their #defines in the same header"""
    text = open(os.path.join(ROOT, "ray-tracer_amd", "csrc", "rt_device_scene.h")).read()
    modes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(RT_SCENE_\w+)\s+(\d+)", text)}
    body = re.search(r"RT_SHAPES\[\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    shapes = [(int(m.group(1)), modes[m.group(2)], int(m.group(3))) for m in re.finditer(r"\{\s*(\d+)\s*,\s*(RT_SCENE_\w+)\s*,\s*(\d+)\s*\}", body)]
    assert shapes and len(shapes) == body.count("{"), "RT_SHAPES not understood"
    return shapes


SHAPES = _parse_shapes()
RANDOM_SEED = 13                    # of test_gpu_parity._random_scene: asserted below to hold a mesh and a textured or refractive object
NO_MESH_SCENES = ["three_sphere", "reference_scene2", "reference_scene3", "reference_scene4"]
MESH_SCENES = ["cube", "monkey", "reference_scene0", "random"]


def plan(shape):
    """(environment at commit, scenes) that reach `shape`; a shape nothing here reaches is a failure"""
    has_mesh, mode, threads = shape
    if mode == 1:
        return {"RT_AMD_THREADS": str(threads)}, (MESH_SCENES if has_mesh else NO_MESH_SCENES)
    if mode == 2 and has_mesh:
        return {"RT_AMD_THREADS": str(threads)}, ["soup6k"]
    if shape == (1, 0, 1024):
        return {"RT_AMD_SCENE_MODE": "0"}, ["soup6k"]
    if shape == (0, 0, 256):
        return {}, ["spheres_beyond_lds"]
    return None, []


def _id(shape):
    return "%s-%s-%d" % ("mesh" if shape[0] else "nomesh", MODE_NAMES.get(shape[1], str(shape[1])), shape[2])


CASES = [(s, name) for s in SHAPES for name in (plan(s)[1] or ["unreachable"])]


@functools.lru_cache(maxsize=None)
def spheres_beyond_lds(rt):
    """the smallest N for which reference_scene4(num_spheres=N)'s blob exceeds a CU's LDS (the flattened size grows with N)"""
    def blob_bytes(n):
        return rt.SceneObjects(rt.scenes.reference_scene4(num_spheres=n)[0]).debug_flatten()["blob"].nbytes
    lo, hi = 100, 3000
    assert blob_bytes(lo) <= LDS_LIMIT < blob_bytes(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if blob_bytes(mid) > LDS_LIMIT else (mid, hi)
    return hi


def scene_of(rt, name):
    if name == "random":
        objs, sky = _random_scene(RANDOM_SEED)
        kinds = [o[0] for o in objs]
        mats = [o[-1][0] for o in objs]
        assert ("mesh" in kinds or "obj" in kinds) and any(m in ("checkerboard", "gradient", "image", "refractive") for m in mats), (kinds, mats)
        return objs, sky
    if name == "spheres_beyond_lds":
        return rt.scenes.reference_scene4(num_spheres=spheres_beyond_lds(rt))
    return rt.scenes.CONFIG_SCENES[name]()


W1, H1, SPP, LIMIT, FRAMES = 100, 67, 3, 5, 6          # ragged: 13 x 9 tiles, the last column and row partial
WA, HA = 67, 45
TIMES = [987654321 + 37 * i for i in range(FRAMES)]
AOV_SKY = (1.0, 1.0, 1.0)
LIGHT, BIAS = (1.5, 2.0, 0.2), 1e-3
_REFS = {}


def oracle_frames(rt, orc, models_dir, name):
    """the oracle's progressive frames 0 .. FRAMES-1 of the scene (frame by frame); [0] is the single frame"""
    key = ("frames", name)
    if key not in _REFS:
        objs, sky = scene_of(rt, name)
        o = orc.Scene(objs, orc.MATH_DET, models_dir)
        cam = rt.Camera(W1, H1).floats()
        out, prev = [], None
        for i, t in enumerate(TIMES):
            prev = o.render(cam, W1, H1, SPP, LIMIT, sky, time_ms=t, frame_num=i, prev=prev)
            out.append(prev.copy())
        _REFS[key] = out
    return _REFS[key]


def oracle_queries(rt, orc, models_dir, name):
    """everything the ray entry points are compared with, from the oracle alone"""
    key = ("queries", name)
    if key not in _REFS:
        objs, _ = scene_of(rt, name)
        oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
        r = {}
        # (3) check_scene's rays; the scenes whose oracle is slow per ray take 500 scattered ones
        r["o"], r["d"], r["n_random"] = scene_rays(rt, n=500 if name in ("soup6k", "spheres_beyond_lds") else 2000)
        r["hit"], r["out"] = oracle_records(oracle, r["o"], r["d"])
        frac = r["hit"][:r["n_random"]].mean()
        assert 0.25 <= frac <= 0.90, (name, frac)
        # (4) the planes' primary rays
        cam = rt.Camera(WA, HA).floats()
        pd = primaries(cam, WA, HA).reshape(-1, 3)
        po = np.broadcast_to(np.asarray(cam[0:3], np.float32), pd.shape)
        r["phit"], r["pout"] = oracle_records(oracle, po, pd)
        r["one_bounce"] = oracle.render(cam, WA, HA, 1, 1, AOV_SKY, time_ms=4242, antialias=False)
        # (5) the occlusion batch of test_gpu_occlusion.check_scene
        r["oo"], r["od"] = _rays(N_BASE, 5)
        r["ohit"], r["ot"], _ = oracle_hits(oracle, r["oo"], r["od"])
        assert 0.10 <= r["ohit"].mean() <= 0.90, (name, r["ohit"].mean())
        # (6)
        r["vis"] = oracle_visibility(oracle, cam, WA, HA, LIGHT, BIAS)
        _REFS[key] = r
    return _REFS[key]


def commit_as(rt, ctx, monkeypatch, objs, models_dir, env):
    """the scene committed under `env` (read by rt_scene_commit), the overrides removed again before anything else runs"""
    with monkeypatch.context() as m:
        for k in ("RT_AMD_THREADS", "RT_AMD_SCENE_MODE", "RT_AMD_BLOCKS_PER_CU"):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    assert not any(k in os.environ for k in env)
    return scene


def check_frames(rt, ctx, scene, sky, want, what):
    """(1) one frame; (2) FRAMES progressive frames of the same view in one launch, from frame 0"""
    cam, rd = rt.Camera(W1, H1), rt.RenderData(SPP, LIMIT, True, sky)
    one = rt.VariableRenderData(W1, H1)
    rt.render(ctx, scene, cam, rd, one, TIMES[0])
    assert eq(one.previous_render, want[0]), (what, "one frame", int((one.previous_render.view(np.uint32) != want[0].view(np.uint32)).sum()))
    many = rt.VariableRenderData(W1, H1)
    many.previous_render[...] = 7.0                                   # garbage: frame 0 ignores it
    assert ctx.max_batch_frames(W1, H1) >= FRAMES                     # one launch, not several
    rt.render_frames(ctx, scene, cam, rd, many, TIMES)
    assert many.frame_num == FRAMES
    assert eq(many.previous_render, want[-1]), (what, "%d frames in one launch" % FRAMES, int((many.previous_render.view(np.uint32) != want[-1].view(np.uint32)).sum()))


def default_albedo(rt, models_dir, name):
    """the albedo plane of the scene on the shape it gets by default, on a context of its own"""
    key = ("albedo", name)
    if key not in _REFS:
        c = rt.Context(0)
        _REFS[key] = rt.render_aov(c, c.commit(rt.SceneObjects(scene_of(rt, name)[0], models_dir)), rt.Camera(WA, HA), AOV_SKY, planes=("albedo",))["albedo"]
    return _REFS[key]


def check_aov(rt, ctx, scene, objs, models_dir, q, name, what):
    """(4) all planes: ray, depth, normal, object against the oracle on every pixel; albedo against the oracle's one-bounce frame where that
    shows it (sky and emissive hits: sky (1,1,1), 1 spp, limit 1, no antialiasing - see test_albedo_is_the_one_bounce_render) and elsewhere
    against the default shape's plane, which the albedo tests of test_gpu_query.py tie to the oracle"""
    cam = rt.Camera(WA, HA)
    aov = rt.render_aov(ctx, scene, cam, AOV_SKY)
    assert sorted(aov) == sorted(rt.AOV_PLANES)
    assert np.array_equal(u32(aov["ray"]), u32(primaries(cam.floats(), WA, HA))), what
    h, out = q["phit"], q["pout"]
    obj, depth, normal, albedo = aov["object"].reshape(-1), aov["depth"].reshape(-1), aov["normal"].reshape(-1, 3), aov["albedo"].reshape(-1, 3)
    assert np.array_equal(obj >= 0, h) and np.array_equal(obj[h], out[h, 7].astype(np.int32)) and np.all(obj[~h] == -1), what
    assert np.array_equal(u32(depth[h]), u32(out[h, 0])) and np.all(u32(depth[~h]) == u32(MISS_T)), what
    assert np.array_equal(u32(normal[h]), u32(out[h, 4:7])) and not u32(normal[~h]).any(), what
    emissive = np.array([o[-1][0] == "emissive" for o in objs] + [False])
    lit = (obj < 0) | emissive[obj]
    assert np.array_equal(u32(albedo[lit]), u32(q["one_bounce"].reshape(-1, 3)[lit])), what
    assert aov["albedo"].tobytes() == default_albedo(rt, models_dir, name).tobytes(), what


@pytest.mark.parametrize("shape,name", CASES, ids=["%s-%s" % (_id(s), n) for s, n in CASES])
def test_shape_equals_oracle(rt, orc, ctx, models_dir, monkeypatch, shape, name):
    env, scenes = plan(shape)
    assert scenes, "RT_SHAPES has the shape %s and this file has no scene that reaches it" % (shape,)
    objs, sky = scene_of(rt, name)
    if name == "spheres_beyond_lds":
        # the count is the smallest that leaves LDS: one sphere fewer is still staged
        fewer = ctx.commit(rt.SceneObjects(rt.scenes.reference_scene4(num_spheres=spheres_beyond_lds(rt) - 1)[0], models_dir)).info()
        assert fewer["scene_in_lds"] == 1, fewer
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    print("%s: %s" % (name, info))
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    what = "%s on %s" % (name, _id(shape))
    check_frames(rt, ctx, scene, sky, oracle_frames(rt, orc, models_dir, name), what)                       # (1), (2)
    q = oracle_queries(rt, orc, models_dir, name)
    hits = rt.trace_rays(ctx, scene, q["o"], q["d"])                                                        # (3)
    assert_equal_to_oracle(hits, q["hit"], q["out"], what)
    checked = assert_triangles_and_uv(rt, objs, models_dir, q["o"], q["d"], hits, what)
    assert checked > 0 or not any(o[0] != "sphere" for o in objs), what
    check_aov(rt, ctx, scene, objs, models_dir, q, name, what)                                              # (4)
    check_batch(rt, ctx, scene, q["oo"], q["od"], q["ohit"], q["ot"], what)                                 # (5): no limit, and limits around the oracle's distances
    for k in (1, 63, 64, 65):
        check_batch(rt, ctx, scene, q["oo"][:k], q["od"][:k], q["ohit"][:k], q["ot"][:k], "%s n=%d" % (what, k))
    got = rt.render_visibility(ctx, scene, rt.Camera(WA, HA), LIGHT, BIAS)                                  # (6)
    assert got.tobytes() == q["vis"].tobytes(), (what, int((got != q["vis"]).sum()))


def test_every_shape_has_a_case():
    assert len(SHAPES) == len(set(SHAPES)) and all(plan(s)[1] for s in SHAPES), [s for s in SHAPES if not plan(s)[1]]
    assert {s for s, _ in CASES} == set(SHAPES)


# ---- the knob matrix ------------------------------------------------------------------------------------------------------------------
# each row forces one control path of the render kernel's wave loop (rt_render_kernel.h); every value is inside rt_ctx_create's ranges
KNOB_ROWS = {
    "yield-whenever-ready": {"RT_AMD_WORK_THRESHOLD": "64"},                     # the traversal loop leaves whenever any lane is ready
    "never-yield": {"RT_AMD_WORK_THRESHOLD": "1", "RT_AMD_READY_BREAK": "65", "RT_AMD_HIT_BREAK": "65", "RT_AMD_HIT_LOW": "0"},   # ... only when no lane traverses
    "batches-of-one": {"RT_AMD_HIT_BREAK": "1", "RT_AMD_HIT_LOW": "1", "RT_AMD_MIX_BREAK": "1", "RT_AMD_READY_BREAK": "1"},
    "hit-break-below-hit-low": {"RT_AMD_HIT_BREAK": "8"},                        # (hit_low defaults to 16: clamped by rt_sched::kernel_knobs)
    "mix-rule-off": {"RT_AMD_MIX_BREAK": "0"},
    "descents-to-their-end": {"RT_AMD_DESCEND_KEEP": "0"},
    "descents-left-at-once": {"RT_AMD_DESCEND_KEEP": "64"},
    "shade-batch-1": {"RT_AMD_SHADE_BATCH": "1"},
    "shade-batch-64": {"RT_AMD_SHADE_BATCH": "64"},
}
KNOB_SCENES = ["monkey", "cube", "reference_scene0", "reference_scene4"]
KNOB_CASES = [(row, name, None) for row in KNOB_ROWS for name in KNOB_SCENES if not row.startswith("shade-batch") or name == "reference_scene4"]
KNOB_CASES.append(("descents-left-at-once", "monkey", 512))                      # the two axes crossed once: partial descents on a stack stride of 512


@pytest.mark.parametrize("row,name,threads", KNOB_CASES, ids=["%s-%s%s" % (r, n, "-%d" % t if t else "") for r, n, t in KNOB_CASES])
def test_knobs_do_not_change_an_image(rt, orc, models_dir, monkeypatch, row, name, threads):
    objs, sky = scene_of(rt, name)
    want = oracle_frames(rt, orc, models_dir, name)
    with monkeypatch.context() as m:
        for k in [k for k in os.environ if k.startswith("RT_AMD_") and k not in ("RT_AMD_LIB", "RT_AMD_NO_TORCH")]:
            m.delenv(k)
        for k, v in KNOB_ROWS[row].items():
            m.setenv(k, v)
        ctx = rt.Context(0)                                           # the knobs are read here
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": str(threads)} if threads else {})
    if threads:
        assert scene.info()["threads_per_block"] == threads and scene.info()["scene_in_lds"] == 1, scene.info()
    check_frames(rt, ctx, scene, sky, want, "%s with %s" % (name, KNOB_ROWS[row]))
    print("%s, %s: %d frames in %.3f ms on %s" % (name, row, FRAMES, ctx.last_kernel_ms(), scene.info()))       # (shown with -s: the rows differ in time, not in bits)
    del scene, ctx
