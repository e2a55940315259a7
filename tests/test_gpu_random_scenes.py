"""Random mixed scenes (tests/random_scenes.py) through EVERY kernel family, not only the render kernel: closest-hit queries, the first-hit
planes, occlusion queries, the visibility plane, the ambient-occlusion plane, sample budgets and camera sequences, each against the
yardstick its own test file uses (the CPU oracle in det mode, tests/ao_ref.py, tests/adaptive_ref.py, tests/views_ref.py) plus two that are
new here: the winner's texture coordinates of oracle/binding.py::Scene.trace_one_uv for every hit, spheres included, and the albedo of
tests/texture_ref.py at every ordinary hit.  Every ray and pixel is compared as uint32 or bytes; nothing is sampled, nothing has a tolerance.

What the nine config scenes of the other files never hold and these do (tests/test_random_scenes.py asserts it from the oracle alone): two to
six meshes per scene, so that a lane leaves one tree and enters the next with its stack back at 0 and a mesh's triangles sit behind an
earlier mesh's in the flattened layout; meshes, cuboids and one-way quads with checkerboard, gradient and image textures and refractive
materials; emissive meshes; every primitive kind winning hits next to every other.

The placement axis: the two richest seeds (13: five meshes, 15: six) run every family on the shape the scene picks by itself, forced to 1024
threads (where the budget and views kernels walk with rt_descend_pop) and from global memory.  RT_AMD_SCENE_MODE=0 only turns the hybrid
placement off - a scene that fits LDS stays there - so the global cases add FILLER, one more mesh behind the scene that alone outgrows LDS:
the seed's objects keep their indices and every mesh of the seed still lies before it.  Two triangle soups (random_soup_scene: leaves of
several triangles, a refractive mesh) run the ray families on the hybrid and the global placement they get by themselves.  Each case first
asserts its placement from scene.info().

The oracle's answers are computed once per scene and shared by the cases.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import adaptive_ref
import ao_ref
import texture_ref
import views_ref
from random_scenes import random_scene, random_soup_scene, scene_rays_for
from test_gpu_adaptive import assert_frame
from test_gpu_ao import BOTH, assert_planes
from test_gpu_occlusion import check_batch, oracle_visibility
from test_gpu_query import MISS_T, assert_equal_to_oracle, assert_triangles_and_uv, primaries, u32
from test_gpu_shapes import SHAPES, commit_as
from test_gpu_views import assert_frames, cameras, on_device, single_launches

pytestmark = pytest.mark.gpu

F = np.float32
SEEDS = list(range(11, 23)) + [66]         # 66: six meshes, the second and third image-textured and in view of the default camera (11-22 show no such pixel)
PLACED_SEEDS = (13, 15)
SOUPS = {"hybrid": 0, "global": 16}         # random_soup_scene seeds: two meshes whose trees fit LDS beside 512 threads' stacks; two whose trees do not
W, H, SPP = 44, 28, 3                       # ragged against the 8 x 8 tiles, narrower than a wave's 64 lanes
N_RAYS, RAY_W, RAY_H = 2000, 40, 30
AO = dict(samples=4, bias=1e-3)
AO_RADII = (0.5, np.inf)
N_VIEWS = 3
AOV_SKY = (0.25, 0.5, 0.75)
LIGHTS = (((1.5, 2.0, 0.2), 1e-3), ((0.0, 0.3, 2.2), 0.0))       # in the open with a bias; among the objects without one
GARBAGE = F(7.0)
BRIGHT_SKY = (0.8, 1.0, 1.0)
ENVS = {"own": {}, "threads1024": {"RT_AMD_THREADS": "1024"}, "global": {"RT_AMD_SCENE_MODE": "0"}}
_FILLER_RNG = np.random.default_rng(99)
FILLER = ("mesh", (np.array([0.0, 0.1, 4.6]) + _FILLER_RNG.normal(0, 0.3, (3000, 1, 3)) + _FILLER_RNG.normal(0, 0.05, (3000, 3, 3))).astype(np.float32).reshape(3000, 9),
          ("standard", (0.6, 0.6, 0.7), 0.1))
_REFS = {}


class Case:
    """one scene under one placement: kind 'random' or 'soup', the generator's seed, and how it is committed"""

    def __init__(self, kind, seed, placement="own"):
        self.kind, self.seed, self.placement = kind, seed, placement
        self.objs, sky = random_scene(seed) if kind == "random" else random_soup_scene(seed)
        # Half the seeds draw a black sky, and then a frame is 0 wherever no emissive object is met (all of seed 21's, all but 13 pixels of
        # seed 15's): a wrong texel or a wrong second hit multiplies a throughput that never reaches the frame.  The render families here
        # light those scenes with the generator's other sky; tests/test_gpu_parity.py renders the seeds under the sky they drew.
        self.sky = sky if any(sky) else BRIGHT_SKY
        if kind == "random" and placement == "global":
            self.objs = list(self.objs) + [FILLER]
        self.name = "%s%d%s" % (kind, seed, "+filler" if len(self.objs) and self.objs[-1] is FILLER else "")       # the key of everything the oracle answers
        self.limit = 2 + seed % 7
        self.time_ms = 1000 + seed
        self.id = "%s%d-%s" % (kind, seed, placement)

    def commit(self, rt, ctx, monkeypatch, models_dir):
        """the scene committed under the placement's environment, the placement asserted from scene.info()"""
        scene = commit_as(rt, ctx, monkeypatch, self.objs, models_dir, ENVS[self.placement] if self.kind == "random" else {})
        info = scene.info()
        shape = (1, info["scene_in_lds"], info["threads_per_block"])
        assert shape in SHAPES and int(rt.SceneObjects(self.objs, models_dir).debug_flatten()["has_mesh"]) == 1, (self.id, info)
        if self.kind == "soup":
            assert info["scene_in_lds"] == {"hybrid": 2, "global": 0}[self.placement], (self.id, info)
        elif self.placement == "own":
            assert info["scene_in_lds"] == 1, (self.id, info)
        elif self.placement == "threads1024":
            assert shape == (1, 1, 1024), (self.id, info)
        else:
            assert shape == (1, 0, 1024), (self.id, info)
        return scene


def ref(case, what, make):
    """make() once per (scene, what); callers leave the answer unchanged"""
    key = (case.name, what)
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def oracle_of(orc, models_dir, case):
    return ref(case, "oracle", lambda: orc.Scene(case.objs, orc.MATH_DET, models_dir))


def uv_records(oracle, o, d):
    """Scene.trace_one_uv for every ray: hit flags and {dist, point, normal, object, u, v}"""
    hit, rec = np.zeros(len(o), bool), np.zeros((len(o), 10), F)
    for i in range(len(o)):
        hit[i], rec[i] = oracle.trace_one_uv(o[i], d[i])
    return hit, rec


def ray_records(orc, models_dir, case):
    """the scene's rays (scene_rays_for) and the oracle's closest hit of each, from trace_one and from trace_one_uv"""
    def make():
        oracle = oracle_of(orc, models_dir, case)
        o, d, n = scene_rays_for(case.seed, N_RAYS, RAY_W, RAY_H)
        hit, rec = uv_records(oracle, o, d)
        hit8 = np.zeros(len(o), bool)
        out8 = np.zeros((len(o), 8), F)
        for i in range(len(o)):
            hit8[i], out8[i] = oracle.trace_one(o[i], d[i])
        return dict(o=o, d=d, n=n, hit=hit8, out=out8, hit_uv=hit, rec=rec)
    return ref(case, "rays", make)


def plane_records(rt, orc, models_dir, case):
    """the W x H view's primary rays and the oracle's closest hit of each, with the winner's texture coordinates"""
    def make():
        cam = rt.Camera(W, H).floats()
        d = primaries(cam, W, H).reshape(-1, 3)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(cam[0:3], F), d.shape))
        hit, rec = uv_records(oracle_of(orc, models_dir, case), o, d)
        return dict(o=o, d=d, hit=hit, rec=rec)
    return ref(case, "planes", make)


def expected_albedo(case, hit, rec, sky):
    """the albedo plane from the oracle's records alone: the sky on a miss, an emissive winner's light, else tests/texture_ref.py's colour of
    the winner's material at the oracle's (u, v)"""
    out = np.empty((len(hit), 3), F)
    out[~hit] = np.asarray(sky, F)
    obj = rec[:, 7].astype(np.int32)
    for k in np.unique(obj[hit]):
        sel = hit & (obj == k)
        out[sel] = texture_ref.albedo(case.objs[k][-1], rec[sel, 8], rec[sel, 9])
    return out


# ---- the families: check_<family>(rt, orc, ctx, models_dir, case, scene) ---------------------------------------------------------------------
def check_trace_rays(rt, orc, ctx, models_dir, case, scene):
    """rt_trace_rays on 2000 random rays and a 40 x 30 primary grid: the record against trace_one, u and v against trace_one_uv on every hit
    (a sphere's latitude / longitude too, which assert_triangles_and_uv cannot recompute), triangle index and barycentric blend on every
    triangle hit.  A best_prim that forgot an earlier mesh's triangle count names another mesh's triangle: the emulator's test on that triangle
    misses or hits elsewhere, and on a textured mesh (seed 13's third mesh holds an image, seed 15's fourth and eleventh objects a gradient)
    tri_uv + 6 * best_prim reads another triangle's coordinates and u, v differ from the oracle's."""
    q = ray_records(orc, models_dir, case)
    hits = rt.trace_rays(ctx, scene, q["o"], q["d"])
    assert_equal_to_oracle(hits, q["hit"], q["out"], case.id)
    h = q["hit"]
    assert np.array_equal(q["hit_uv"], h) and np.array_equal(u32(q["rec"][:, :8]), u32(q["out"]))           # the oracle's two queries agree
    bad = (u32(hits["u"][h]) != u32(q["rec"][h, 8])) | (u32(hits["v"][h]) != u32(q["rec"][h, 9]))
    assert not bad.any(), (case.id, "u, v", int(bad.sum()), np.flatnonzero(h)[bad][:5].tolist())
    checked = assert_triangles_and_uv(rt, case.objs, models_dir, q["o"], q["d"], hits, case.id, sample=len(h))
    spheres = np.array([o[0] == "sphere" for o in case.objs])
    assert checked == int((~spheres[q["out"][h, 7].astype(np.int32)]).sum()), (case.id, checked)                # every hit that is no sphere's


def check_render_aov(rt, orc, ctx, models_dir, case, scene):
    """rt_render_aov: (a) the ray plane is the primary-ray expression; (b) depth, normal, object against the oracle on those rays, as
    tests/test_gpu_query.py::test_aov_planes; the albedo plane on EVERY pixel against expected_albedo - a wrong texel on a textured triangle
    in a cluttered scene, a mesh triangle shaded with another triangle's uv, a cuboid face with the quad corners in another order all
    change the colour tests/texture_ref.py gives for the oracle's (u, v); and sky and emissive pixels against the oracle's one-bounce frame
    as test_albedo_is_the_one_bounce_render compares them."""
    cam = rt.Camera(W, H)
    p = plane_records(rt, orc, models_dir, case)
    hit, rec = p["hit"], p["rec"]
    aov = rt.render_aov(ctx, scene, cam, AOV_SKY)
    assert sorted(aov) == sorted(rt.AOV_PLANES)
    assert np.array_equal(u32(aov["ray"]), u32(primaries(cam.floats(), W, H))), case.id
    obj, depth, normal, albedo = aov["object"].reshape(-1), aov["depth"].reshape(-1), aov["normal"].reshape(-1, 3), aov["albedo"].reshape(-1, 3)
    assert np.array_equal(obj >= 0, hit) and np.array_equal(obj[hit], rec[hit, 7].astype(np.int32)) and np.all(obj[~hit] == -1), case.id
    assert np.array_equal(u32(depth[hit]), u32(rec[hit, 0])) and np.all(u32(depth[~hit]) == u32(MISS_T)), case.id
    assert np.array_equal(u32(normal[hit]), u32(rec[hit, 4:7])) and not u32(normal[~hit]).any(), case.id
    want = expected_albedo(case, hit, rec, AOV_SKY)
    bad = (u32(albedo) != u32(want)).any(axis=1)
    assert not bad.any(), (case.id, "albedo", int(bad.sum()), [(int(i), int(obj[i])) for i in np.flatnonzero(bad)[:5]])
    # sky (1,1,1), 1 spp, reflection limit 1, antialias off: the oracle's frame is the albedo where the first hit is lit, 0 elsewhere
    one = (1.0, 1.0, 1.0)
    frame = ref(case, "one bounce", lambda: oracle_of(orc, models_dir, case).render(cam.floats(), W, H, 1, 1, one, time_ms=4242, antialias=False)).reshape(-1, 3)
    lit = ~hit | np.array([o[-1][0] == "emissive" for o in case.objs] + [False])[rec[:, 7].astype(np.int32)]
    assert not u32(frame[~lit]).any()
    part = rt.render_aov(ctx, scene, cam, one, planes=("albedo", "object"))
    assert part["object"].tobytes() == aov["object"].tobytes()
    assert np.array_equal(u32(part["albedo"].reshape(-1, 3)[lit]), u32(frame[lit])), case.id
    assert np.array_equal(u32(part["albedo"].reshape(-1, 3)[~lit]), u32(want[~lit])), case.id
    data = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, cam, rt.RenderData(1, 1, False, one), data, 4242)
    assert np.array_equal(u32(data.previous_render.reshape(-1, 3)), u32(frame)), case.id
    # the query entry point on the plane's rays gives the planes, and the oracle's texture coordinates
    hits = rt.trace_rays(ctx, scene, p["o"], aov["ray"].reshape(-1, 3))
    assert np.array_equal(u32(hits["t"]), u32(depth)) and np.array_equal(hits["object"], obj) and np.array_equal(u32(hits["normal"]), u32(normal))
    assert np.array_equal(u32(hits["u"][hit]), u32(rec[hit, 8])) and np.array_equal(u32(hits["v"][hit]), u32(rec[hit, 9])), case.id


def check_occluded_rays(rt, orc, ctx, models_dir, case, scene):
    """rt_occluded_rays on the scene's rays with no limit and with per-ray limits on both sides of the oracle's own distance
    (tests/test_gpu_occlusion.py::check_batch: t, the floats below and above it, t / 2, MISS_T, +inf, NaN, 0, negative), on batches of 1, 63,
    64, 65 rays too.  An any-hit walk that stops after the first mesh, or that carries the stack pointer from one mesh's tree into the
    next, misses blockers that only a later mesh provides: every seed but one has two to six meshes."""
    q = ray_records(orc, models_dir, case)
    t = q["out"][:, 0].copy()
    compared = check_batch(rt, ctx, scene, q["o"], q["d"], q["hit"], t, case.id)
    for k in (1, 63, 64, 65):
        compared += check_batch(rt, ctx, scene, q["o"][:k], q["d"][:k], q["hit"][:k], t[:k], "%s n=%d" % (case.id, k))
    return compared


def check_render_visibility(rt, orc, ctx, models_dir, case, scene):
    """rt_render_visibility for a light in the open and one among the objects, with and without a bias, against two oracle calls per pixel
    (tests/test_gpu_occlusion.py::oracle_visibility).  The shadow ray starts ON a surface of a cluttered scene: one-way quads seen from
    behind, refractive and emissive blockers and a second mesh between a first mesh and the light all decide pixels here."""
    cam = rt.Camera(W, H)
    oracle = oracle_of(orc, models_dir, case)
    for light, bias in LIGHTS:
        want = ref(case, ("visibility", light, bias), lambda: oracle_visibility(oracle, cam.floats(), W, H, light, bias))
        got = rt.render_visibility(ctx, scene, cam, light, bias)
        assert got.shape == (H, W) and got.dtype == np.uint8
        assert got.tobytes() == want.tobytes(), (case.id, light, bias, int((got != want).sum()))


def check_render_ao(rt, orc, ctx, models_dir, case, scene):
    """rt_render_ao with 4 samples, radius 0.5 and an unlimited radius, against tests/ao_ref.py on every pixel (counts as bytes, ao as
    uint32).  The fused kernel chains a closest-hit walk and four any-hit walks per pixel over several trees; its samples start on textured
    and refractive surfaces whose normals the first walk flipped."""
    cam = rt.Camera(W, H)
    for radius in AO_RADII:
        r = ao_ref.scene_reference(rt, orc, models_dir, case.name, W, H, AO["samples"], radius, AO["bias"], case.time_ms, objs=case.objs)
        got = rt.render_ao(ctx, scene, cam, planes=BOTH, radius=radius, time_ms=case.time_ms, **AO)
        assert_planes(got, r["count"], r["ao"], (case.id, radius))


def budget_planes(case):
    """two random uint16 budget planes with values 0-5: the first renders over garbage from zero counts, the second folds into it, so that
    the second call's prior counts are the first plane - 0 to 5 and unequal to its own budgets on most pixels (tests/test_random_scenes.py)"""
    rng = np.random.default_rng(5000 + case.seed)
    b1, b2 = (rng.integers(0, 6, (H, W)).astype(np.uint16) for _ in range(2))
    return b1, b2


def check_render_budget(rt, orc, ctx, models_dir, case, scene):
    """rt_render_budget against tests/adaptive_ref.py: a random budget plane over garbage, then a second plane and seed folded into the
    first call's frame and counts.  The budget kernel compiles rt_render_loop.inc with other parameters and, on 1024 threads, walks with
    rt_descend_pop: lanes of one wave hold pixels of 0 to 5 samples, so they enter and leave the meshes' trees out of step."""
    cam, rd = rt.Camera(W, H), rt.RenderData(999, case.limit, True, case.sky)          # (rays_per_pixel is not read)
    oracle = oracle_of(orc, models_dir, case)
    b1, b2 = budget_planes(case)
    garbage, zero = np.full((H, W, 3), GARBAGE, F), np.zeros((H, W), np.uint32)
    want1, count1 = ref(case, "budget 1", lambda: adaptive_ref.budget_render(oracle, cam.floats(), W, H, b1, case.limit, case.sky, case.time_ms, garbage, zero))
    want2, count2 = ref(case, "budget 2", lambda: adaptive_ref.budget_render(oracle, cam.floats(), W, H, b2, case.limit, case.sky, -case.time_ms, want1, count1))
    got1, got_count1 = rt.render_budget(ctx, scene, cam, rd, case.time_ms, b1, garbage, zero)
    assert_frame(got1, want1, (case.id, "over garbage"))
    assert got_count1.tobytes() == count1.tobytes() == b1.astype(np.uint32).tobytes() and np.all(got1[b1 == 0] == GARBAGE)
    got2, got_count2 = rt.render_budget(ctx, scene, cam, rd, -case.time_ms, b2, got1, got_count1)
    assert_frame(got2, want2, (case.id, "fold"))
    assert got_count2.tobytes() == count2.tobytes() == (b1.astype(np.uint32) + b2).tobytes()


def view_inputs(rt, case):
    """three cameras (the default, one translated, one rotated) and their seeds"""
    return cameras(rt, W, H)[:N_VIEWS], [case.time_ms, -case.time_ms, 31 * case.time_ms]


def view_frames(rt, orc, models_dir, case):
    """the oracle's answers for the views: the separate frames and the frame they fold into (tests/views_ref.py)"""
    cams, times = view_inputs(rt, case)
    oracle = oracle_of(orc, models_dir, case)
    fl = [c.floats() for c in cams]
    return (ref(case, "views", lambda: views_ref.separate(oracle, fl, W, H, SPP, case.limit, case.sky, times)),
            ref(case, "views folded", lambda: views_ref.accumulated(oracle, fl, W, H, SPP, case.limit, case.sky, times)))


def check_render_views(rt, orc, ctx, models_dir, case, scene):
    """rt_render_views with three cameras, as separate frames and folded into one, against the oracle's frames / chain and against rt_render
    of each camera.  The views kernel is the third compilation of rt_render_loop.inc; a wave holds pixels of several views, whose rays meet
    the meshes in different orders.  (The three frames differ from one another - tests/test_random_scenes.py - so a mixed-up camera or seed
    cannot pass.)"""
    (cams, times), rd = view_inputs(rt, case), rt.RenderData(SPP, case.limit, True, case.sky)
    want, chain = view_frames(rt, orc, models_dir, case)
    got = on_device(rt, ctx, scene, cams, rd, times)
    assert_frames(got, want, (case.id, "oracle"))
    assert_frames(got, single_launches(rt, ctx, scene, cams, rd, times), (case.id, "rt_render"))
    folded = on_device(rt, ctx, scene, cams, rd, times, accumulate=True)
    assert_frames(folded, chain, (case.id, "folded, oracle"))
    data = rt.VariableRenderData(W, H)
    assert_frames(folded, single_launches(rt, ctx, scene, cams, rd, times, data), (case.id, "folded, chained rt_render"))
    assert data.frame_num == N_VIEWS


FAMILIES = {"trace_rays": check_trace_rays, "render_aov": check_render_aov, "occluded_rays": check_occluded_rays, "render_visibility": check_render_visibility,
            "render_ao": check_render_ao, "render_budget": check_render_budget, "render_views": check_render_views}
SOUP_FAMILIES = ("trace_rays", "render_aov", "occluded_rays", "render_visibility", "render_ao")       # the query, occlusion and AO families

# every family on every seed on the shape the scene picks; the two multi-mesh seeds on the two forced placements as well; the soups
SCENE_CASES = [Case("random", s) for s in SEEDS] + [Case("random", s, p) for s in PLACED_SEEDS for p in ("threads1024", "global")]
SOUP_CASES = [Case("soup", s, p) for p, s in SOUPS.items()]
CASES = [(f, c) for c in SCENE_CASES for f in FAMILIES] + [(f, c) for c in SOUP_CASES for f in SOUP_FAMILIES]


@pytest.mark.parametrize("family,case", CASES, ids=["%s-%s" % (f, c.id) for f, c in CASES])
def test_family_equals_its_yardstick(rt, orc, ctx, models_dir, monkeypatch, family, case):
    scene = case.commit(rt, ctx, monkeypatch, models_dir)
    FAMILIES[family](rt, orc, ctx, models_dir, case, scene)


def test_every_family_runs_on_every_seed_and_placement():
    ran = {(f, c.kind, c.seed, c.placement) for f, c in CASES}
    assert all((f, "random", s, "own") in ran for f in FAMILIES for s in SEEDS)
    assert all((f, "random", s, p) in ran for f in FAMILIES for s in PLACED_SEEDS for p in ENVS)
    assert all((f, "soup", s, p) in ran for f in SOUP_FAMILIES for p, s in SOUPS.items())
