"""The ambient-occlusion plane (rt_render_ao) against its yardstick (tests/ao_ref.py: the definition restated over the CPU oracle), against
the product's own renderer and against the unfused occlusion query.  Counts are compared as uint16 bytes and ao as uint32, on every pixel,
never to a tolerance.  The yardstick's planes are computed once per parameter set and shared.  Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_ref
from test_gpu_query import SCENES, u32
from test_gpu_shapes import SHAPES, _id, commit_as, plan, scene_of

pytestmark = pytest.mark.gpu

F = np.float32
BIG = ("soup6k", "sphere50k", "spheres_beyond_lds")
BASE = dict(samples=8, radius=0.5, bias=1e-3, time_ms=12345)
BOTH = ("ao", "count")


def size_of(name):
    """ragged tiles on both edges; the scenes whose oracle is slow per ray take the smaller image"""
    return (29, 21) if name in BIG else (61, 45)


def reference(rt, orc, models_dir, name, W, H, objs=None, **p):
    return ao_ref.scene_reference(rt, orc, models_dir, name, W, H, p["samples"], p["radius"], p["bias"], p["time_ms"], objs=objs)


def assert_planes(got, want_count, want_ao, what):
    assert got["count"].dtype == np.uint16 and got["ao"].dtype == np.float32 and got["count"].shape == got["ao"].shape == want_count.shape
    assert got["count"].tobytes() == want_count.tobytes(), (what, "count", int((got["count"] != want_count).sum()))
    assert np.array_equal(u32(got["ao"]), u32(want_ao)), (what, "ao", int((u32(got["ao"]) != u32(want_ao)).sum()))


def partial_share(ref, samples):
    """of the surface pixels, the share with 0 < count < samples (from the yardstick alone)"""
    c = ref["count"][ref["surface"]]
    return float(((c > 0) & (c < samples)).mean())


def check_scene(rt, orc, ctx, models_dir, name, scene=None, objs=None, size=None, min_share=0.10, **over):
    p = dict(BASE, **over)
    W, H = size or size_of(name)
    if scene is None:
        scene = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name]()[0], models_dir))
    ref = reference(rt, orc, models_dir, name, W, H, objs=objs, **p)
    share = partial_share(ref, p["samples"])
    print("%s %dx%d %s: %d surface pixels, %.0f %% partly occluded, placement %d" % (name, W, H, p, ref["surface"].sum(), 100 * share, scene.info()["scene_in_lds"]))
    # condition on the inputs, from the yardstick alone: a plane that is nearly all free or all blocked would test little
    assert share >= min_share, (name, share)
    assert_planes(rt.render_ao(ctx, scene, rt.Camera(W, H), planes=BOTH, **p), ref["count"], ref["ao"], name)
    return scene.info()["scene_in_lds"]


@pytest.mark.parametrize("name", [s for s in SCENES if s not in BIG])
def test_ao_equals_the_yardstick(rt, orc, ctx, models_dir, name):
    assert check_scene(rt, orc, ctx, models_dir, name) == 1          # the whole scene in LDS


def test_ao_equals_the_yardstick_beyond_lds(rt, orc, ctx, models_dir):
    """soup6k and sphere50k: the placements beyond LDS.  HYBRID (2) and GLOBAL (0) must both run; a placement the committed shapes do not
    pick is forced with RT_AMD_SCENE_MODE in a fresh child process, as tests/test_gpu_occlusion.py does it."""
    modes = {name: check_scene(rt, orc, ctx, models_dir, name) for name in ("soup6k", "sphere50k")}
    assert all(m in (0, 2) for m in modes.values()), modes
    missing = {0, 2} - set(modes.values())
    assert 2 not in missing, ("no scene runs the hybrid placement", modes)
    if 0 in missing:
        env = dict(os.environ, RT_AMD_SCENE_MODE="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "soup6k"], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "placement 0" in r.stdout and "child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey"])
def test_unlimited_radius(rt, orc, ctx, models_dir, name):
    check_scene(rt, orc, ctx, models_dir, name, radius=np.inf)
    # RT_HIT_MISS_T and anything above it mean the same: any hit at all
    W, H = size_of(name)
    scene = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name]()[0], models_dir))
    ref = reference(rt, orc, models_dir, name, W, H, **dict(BASE, radius=np.inf))
    for radius in (float(rt.HIT_MISS_T), 3.0e38):
        assert_planes(rt.render_ao(ctx, scene, rt.Camera(W, H), planes=BOTH, **dict(BASE, radius=radius)), ref["count"], ref["ao"], (name, radius))


GREY = ("standard", (0.5, 0.5, 0.5), 0)
# what a 1x1 image's only pixel (the view's top left corner) looks at: a large sphere, and a second one beside the hit that covers part of
# its hemisphere without crossing the primary ray
CORNER_SPHERES = [("sphere", (-1.79, 1.79, 3.1), 1.5, GREY), ("sphere", (-0.2, 1.1, 1.75), 0.6, GREY)]


@pytest.mark.parametrize("name,W,H", [("corner_spheres", 1, 1), ("three_sphere", 1, 1), ("three_sphere", 7, 9), ("corner_spheres", 7, 9)])
def test_small_images(rt, orc, ctx, models_dir, name, W, H):
    objs = CORNER_SPHERES if name == "corner_spheres" else rt.scenes.three_sphere()[0]
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    ref = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, 8, 0.5, 1e-3, 12345, objs=objs)
    # the one pixel of the corner scene has a surface and is partly occluded; the config scene's looks past everything
    if (W, H) == (1, 1):
        assert (0 < ref["count"][0, 0] < 8) if name == "corner_spheres" else ref["count"][0, 0] == ao_ref.NO_SURFACE
    else:
        assert ref["surface"].any()
    assert_planes(rt.render_ao(ctx, scene, rt.Camera(W, H), planes=BOTH, **BASE), ref["count"], ref["ao"], (name, W, H))


@pytest.mark.parametrize("name,W,H,samples", [("three_sphere", 61, 45, 1), ("three_sphere", 8, 8, 4096), ("monkey", 13, 11, 100)],
                         ids=["one-sample", "4096-samples", "100-samples-ragged"])
def test_sample_counts(rt, orc, ctx, models_dir, name, W, H, samples):
    """1, the most, and more than a wave has lanes on an image of ragged tiles"""
    scene = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name]()[0], models_dir))
    p = dict(BASE, samples=samples)
    ref = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, samples, p["radius"], p["bias"], p["time_ms"])
    assert ref["surface"].sum() >= 16 and (samples == 1 or partial_share(ref, samples) >= 0.10)
    assert_planes(rt.render_ao(ctx, scene, rt.Camera(W, H), planes=BOTH, **p), ref["count"], ref["ao"], (name, samples))


def test_radius_at_a_blockers_distance(rt, orc, ctx, models_dir):
    """the oracle's own blocker distance t of one pixel's sample as the radius: blocked at t, free just below it.  A sample's direction does
    not depend on the radius, so the yardstick's per-sample distances of the unlimited run give the expected plane for any radius."""
    name = "monkey"
    W, H = size_of(name)
    scene = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name]()[0], models_dir))
    ref = reference(rt, orc, models_dir, name, W, H, **dict(BASE, radius=np.inf))
    # the chosen sample: a blocker at a distance no other sample of the plane shares, nearest to 0.5
    ts, n_each = np.unique(ref["t"][ref["hit"]], return_counts=True)
    ts = ts[n_each == 1]
    t = F(ts[np.argmin(np.abs(ts - F(0.5)))])
    (py,), (px,), (k,) = np.nonzero(ref["t"] == t)
    below = np.nextafter(t, F(0.0))
    planes = {}
    for radius in (t, below):
        with np.errstate(invalid="ignore"):
            free = ~(ref["hit"] & (ref["t"] <= radius))
        count = np.where(ref["surface"], free.sum(axis=2), ao_ref.NO_SURFACE).astype(np.uint16)
        ao = np.where(ref["surface"], count.astype(F) / F(BASE["samples"]), F(1.0)).astype(F)
        planes[float(radius)] = count
        assert_planes(rt.render_ao(ctx, scene, rt.Camera(W, H), planes=BOTH, **dict(BASE, radius=float(radius))), count, ao, (name, float(radius)))
    diff = planes[float(below)].astype(np.int32) - planes[float(t)].astype(np.int32)
    assert diff[py, px] == 1 and np.count_nonzero(diff) == 1, (py, px, k, float(t))


def test_no_bias_single_planes_streams_and_repeats(rt, orc, ctx, models_dir):
    import torch
    name = "three_sphere"
    W, H = size_of(name)
    cam = rt.Camera(W, H)
    scene = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name]()[0], models_dir))
    check_scene(rt, orc, ctx, models_dir, name, bias=0.0)
    ref = reference(rt, orc, models_dir, name, W, H, **BASE)
    biased = reference(rt, orc, models_dir, name, W, H, **dict(BASE, bias=0.0))
    assert not np.array_equal(u32(ref["origin"]), u32(biased["origin"]))
    # only count, only ao
    only = rt.render_ao(ctx, scene, cam, planes=("count",), **BASE)
    assert list(only) == ["count"] and only["count"].tobytes() == ref["count"].tobytes()
    only = rt.render_ao(ctx, scene, cam, **BASE)                        # the default: ao
    assert list(only) == ["ao"] and np.array_equal(u32(only["ao"]), u32(ref["ao"]))
    # two calls give equal bytes
    a, b = rt.render_ao(ctx, scene, cam, planes=BOTH, **BASE), rt.render_ao(ctx, scene, cam, planes=BOTH, **BASE)
    assert a["count"].tobytes() == b["count"].tobytes() and a["ao"].tobytes() == b["ao"].tobytes()
    # the device form: both planes, one plane with the other left alone, and a stream of the caller ordered against a following copy
    dev = torch.device("cuda:0")
    t_count = torch.full((H, W), 7, dtype=torch.int16, device=dev)
    t_ao = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rt.render_ao_device(ctx, scene, cam, d_count=t_count.data_ptr(), d_ao=t_ao.data_ptr(), **BASE)
    ctx.synchronize()
    assert t_count.cpu().numpy().view(np.uint16).tobytes() == ref["count"].tobytes() and np.array_equal(u32(t_ao.cpu().numpy()), u32(ref["ao"]))
    assert ctx.last_kernel_ms() > 0
    t_count.fill_(7)
    t_ao.fill_(7.0)
    torch.cuda.synchronize()
    rt.render_ao_device(ctx, scene, cam, d_count=t_count.data_ptr(), **BASE)
    ctx.synchronize()
    assert t_count.cpu().numpy().view(np.uint16).tobytes() == ref["count"].tobytes() and bool((t_ao == 7.0).all())
    s = torch.cuda.Stream(device=dev)
    t_copy = torch.zeros_like(t_ao)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rt.render_ao_device(ctx, scene, cam, d_ao=t_ao.data_ptr(), stream=s.cuda_stream, **BASE)
        t_copy.copy_(t_ao, non_blocking=True)
    s.synchronize()
    assert np.array_equal(u32(t_copy.cpu().numpy()), u32(ref["ao"]))
    # another seed, a negative one included, is another plane: the yardstick's
    for tm in (12346, -7):
        other = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, 8, 0.5, 1e-3, tm)
        assert other["count"].tobytes() != ref["count"].tobytes()
        assert_planes(rt.render_ao(ctx, scene, cam, planes=BOTH, **dict(BASE, time_ms=tm)), other["count"], other["ao"], tm)


def test_invalid_arguments_leave_the_outputs_untouched(rt, ctx, models_dir):
    L = rt.lib()
    objs, _ = rt.scenes.three_sphere()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objs, models_dir))
    W, H = 16, 8
    cam = C.byref(rt.Camera(W, H).c)
    count = np.full((H, W), 0x1234, np.uint16)
    ao = np.full((H, W), 7.0, F)
    pc, pa = C.c_void_p(count.ctypes.data), ao.ctypes.data_as(C.POINTER(C.c_float))
    nan, inf = float("nan"), float("inf")
    good = (ctx._h, scene._h, cam, 8, 0.5, 1e-3, 0, pc, pa)

    def with_(i, v):
        return good[:i] + (v,) + good[i + 1:]

    bad = [(with_(3, 0), "sample count"), (with_(3, -1), "sample count"), (with_(3, rt.AO_MAX_SAMPLES + 1), "sample count"),
           (with_(4, nan), "radius"), (with_(4, 0.0), "radius"), (with_(4, -1.0), "radius"), (with_(4, -inf), "radius"),
           (with_(5, -1e-3), "bias"), (with_(5, inf), "bias"), (with_(5, nan), "bias"),
           (good[:7] + (None, None), "null"), (with_(1, None), "null"), (with_(2, None), "null"), (with_(1, foreign._h), "another context")]
    for args, msg in bad:
        assert L.rt_render_ao(*args) == rt.RT_ERR_INVALID, (msg, args[3:7])
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        assert L.rt_render_ao_device(*(args + (None,))) == rt.RT_ERR_INVALID, (msg, args[3:7])
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        assert np.all(count == 0x1234) and np.all(ao == 7.0), msg
    assert L.rt_render_ao(None, scene._h, cam, 8, 0.5, 1e-3, 0, pc, pa) == rt.RT_ERR_INVALID
    assert np.all(count == 0x1234) and np.all(ao == 7.0)
    # the limits themselves are accepted, and the context is as usable as before
    for args in (with_(3, 1), with_(4, inf), with_(5, 0.0), with_(6, -1), good[:7] + (pc, None), good[:7] + (None, pa)):
        assert L.rt_render_ao(*args) == rt.RT_OK, ctx.last_error()
    assert not np.any(count == 0x1234) and not np.any(ao == 7.0)


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey"])
def test_one_sample_is_the_renderers_first_bounce(rt, ctx, models_dir, name):
    """the product's own render kernel on the all-white scene, 1 spp, reflection limit 2, antialiasing off, sky 1: a pixel is 1 where the
    first bounce ray escapes (or there is no surface) and 0 where it does not - render_ao's count with one sample, no bias, any hit"""
    W, H = 61, 45
    cam = rt.Camera(W, H)
    scene = ctx.commit(rt.SceneObjects(ao_ref.whitened(rt.scenes.CONFIG_SCENES[name]()[0]), models_dir))
    for time_ms in (12345, -99):
        data = rt.VariableRenderData(W, H)
        rt.render(ctx, scene, cam, rt.RenderData(1, 2, False, (1.0, 1.0, 1.0)), data, time_ms)
        got = rt.render_ao(ctx, scene, cam, samples=1, radius=np.inf, bias=0.0, time_ms=time_ms, planes=BOTH)
        want = np.where(got["count"] == rt.AO_NO_SURFACE, 1, got["count"]).astype(F)
        assert (want == 0).any() and (want == 1).any() and (got["count"] == rt.AO_NO_SURFACE).any()
        for c in range(3):
            assert np.array_equal(u32(data.previous_render[..., c]), u32(want)), (name, time_ms, c)
        assert np.array_equal(u32(got["ao"]), u32(want))


def test_samples_equal_the_unfused_occlusion_query(rt, orc, ctx, models_dir):
    """rt_occluded_rays on the very segments the yardstick produced answers what the fused kernel counted: its per-sample bits"""
    name = "monkey"
    W, H = size_of(name)
    scene = ctx.commit(rt.SceneObjects(rt.scenes.CONFIG_SCENES[name]()[0], models_dir))
    ref = reference(rt, orc, models_dir, name, W, H, **BASE)
    s = ref["surface"]
    n = BASE["samples"]
    o = np.repeat(ref["origin"][s][:, None, :], n, axis=1).reshape(-1, 3)
    d = ref["direction"][s].reshape(-1, 3)
    occ = rt.occluded_rays(ctx, scene, o, d, BASE["radius"]).reshape(-1, n)
    assert occ.tobytes() == (1 - ref["free"][s]).astype(np.uint8).tobytes()
    got = rt.render_ao(ctx, scene, rt.Camera(W, H), planes=("count",), **BASE)["count"]
    assert np.array_equal(got[s], (n - occ.sum(axis=1)).astype(np.uint16)) and np.all(got[~s] == rt.AO_NO_SURFACE)


SHAPE_CASES = [(s, (plan(s)[1] or ["unreachable"])[0]) for s in SHAPES]
# The scene that leaves LDS without a mesh is a thin cloud of small spheres: within 0.5 next to nothing is in the way.  It takes the larger
# image, 16 samples and no limit, and of its ~1,300 surface pixels 2 % are asked to be partly occluded (the yardstick has 42 such pixels).
SHAPE_PARAMS = {"spheres_beyond_lds": dict(size=(61, 45), samples=16, radius=np.inf, min_share=0.02)}


@pytest.mark.parametrize("shape,name", SHAPE_CASES, ids=["%s-%s" % (_id(s), n) for s, n in SHAPE_CASES])
def test_every_shape_equals_the_yardstick(rt, orc, ctx, models_dir, monkeypatch, shape, name):
    """tests/test_gpu_shapes.py's forcing of every entry of RT_SHAPES, for the AO kernel: the first scene that reaches the shape"""
    env, scenes = plan(shape)
    assert scenes, "RT_SHAPES has the shape %s and tests/test_gpu_shapes.py has no scene that reaches it" % (shape,)
    objs, _ = scene_of(rt, name)
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    check_scene(rt, orc, ctx, models_dir, name, scene=scene, objs=objs, **SHAPE_PARAMS.get(name, {}))


if __name__ == "__main__":
    # child of test_ao_equals_the_yardstick_beyond_lds: one scene under the environment's placement knob
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    _rt = importlib.import_module("ray-tracer_amd")
    from oracle import binding as _orc
    _orc.build()
    check_scene(_rt, _orc, _rt.Context(0), _rt.scenes.models_dir(), sys.argv[1])
    print("child ok")
