"""The cube-map sky on the device (rt_sky_create, rt_render_sky[_device]) against its yardstick (tests/sky_ref.py: the oracle's bounce loop
restated over the oracle's exported pieces, with the lookup at the miss) and against the product's own camera sequences.  Every frame is
compared as uint32 on every pixel, never to a tolerance.  A scene's paths are traced once by the yardstick and shaded under every map a
test needs.  Run with -m gpu on an MI355X."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import sky_ref as S
from test_gpu_query import u32
from test_gpu_shapes import KNOB_ROWS, SHAPES, _id, commit_as, plan, scene_of
from test_gpu_views import GARBAGE, H, LIMIT, SCENES, SPP, W, assert_frames
from test_gpu_views import on_device as views_on_device

pytestmark = pytest.mark.gpu

F = np.float32
FACE_SIZES = [1, 2, 3, 7, 16, 64]
TIMES = [12345, -99, 777]
TINT = (0.9, 0.5, 1.5)
_CACHE = {}


def cameras(rt, w=W, h=H):
    """the default; one moved and rotated; one turned away from the scene (about the y axis by pi): it sees little but sky"""
    return [rt.Camera(w, h), rt.Camera(w, h, pos=(0.2, 0.0, 0.1), rot=(0.05, -0.2, 0.1)), rt.Camera(w, h, rot=(0.0, math.pi, 0.0))]


def hdr_map(n, seed=5):
    """texels in [0, 50], a few of them 0, a few 1e4, one Inf"""
    rng = np.random.default_rng(seed + n)
    faces = rng.uniform(0.0, 50.0, (6, n, n, 3)).astype(F)
    flat = faces.reshape(-1, 3)
    pick = rng.permutation(len(flat))
    k = max(1, len(flat) // 16)
    flat[pick[:k]] = 0.0
    if len(flat) > 2 * k:
        flat[pick[k:2 * k], rng.integers(0, 3)] = 1e4
        flat[pick[2 * k], 1] = np.inf
    return faces


def paths_of(rt, orc, models_dir, name, cams, times, tag="views", objs=None, w=W, h=H, spp=SPP, limit=LIMIT, antialias=True):
    """the yardstick's paths of every view, once per (scene, tag); callers leave them unchanged"""
    key = (name, tag)
    if key not in _CACHE:
        if objs is None:
            objs, _ = scene_of(rt, name)
        oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
        _CACHE[key] = [S.view_paths(orc, oracle, objs, c.floats(), w, h, spp, limit, t, antialias) for c, t in zip(cams, times)]
    return _CACHE[key]


def shaded(paths, faces, tint):
    """-> the views' means and, per view, what its samples read"""
    means, reads = zip(*[S.view_mean(p, faces, tint) for p in paths])
    return list(means), list(reads)


def on_device(rt, ctx, scene, sky, cams, rd, times, accumulate=False, frame_num=0, start=None, stream=None):
    """rt_render_sky_device over a buffer of garbage (or `start`); -> the frames"""
    import torch
    h, w = cams[0].height, cams[0].width
    shape = (h, w, 3) if accumulate else (len(cams), h, w, 3)
    t = torch.from_numpy(np.full(shape, GARBAGE, F) if start is None else np.ascontiguousarray(start, F)).to("cuda:0")
    torch.cuda.synchronize()
    rt.render_sky_device(ctx, scene, sky, cams, rd, times, t.data_ptr(), accumulate=accumulate, frame_num=frame_num, stream=stream)
    ctx.synchronize()
    return t.cpu().numpy()


def check_both_modes(rt, ctx, scene, faces, tint, cams, times, paths, what, spp=SPP, limit=LIMIT, antialias=True):
    sky = rt.Sky(ctx, faces)
    rd = rt.RenderData(spp, limit, antialias, tint)
    means, reads = shaded(paths, faces, tint)
    assert_frames(on_device(rt, ctx, scene, sky, cams, rd, times), S.separate(means), (what, "separate"))
    assert_frames(on_device(rt, ctx, scene, sky, cams, rd, times, accumulate=True), S.accumulated(means), (what, "accumulated"))
    return reads


# ---- 1. the two identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_a_constant_map_is_the_constant_sky(rt, ctx, models_dir, name):
    objs, _ = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams = cameras(rt)
    ones = rt.Sky(ctx, np.ones((6, 3, 3, 3), F))
    c = np.asarray((0.7, 1.3, 0.05), F)
    const = rt.Sky(ctx, np.broadcast_to(c, (6, 2, 2, 3)))
    product = tuple(float(v) for v in c * np.asarray(TINT, F))                    # fl(c * s), one rounding per channel
    for accumulate in (False, True):
        rd = rt.RenderData(SPP, LIMIT, True, TINT)
        want = views_on_device(rt, ctx, scene, cams, rd, TIMES, accumulate=accumulate)
        assert_frames(on_device(rt, ctx, scene, ones, cams, rd, TIMES, accumulate=accumulate), want, (name, "a map of ones", accumulate))
        assert ctx.last_kernel_ms() > 0
        want = views_on_device(rt, ctx, scene, cams, rt.RenderData(SPP, LIMIT, True, product), TIMES, accumulate=accumulate)
        assert_frames(on_device(rt, ctx, scene, const, cams, rd, TIMES, accumulate=accumulate), want, (name, "a constant map, tinted", accumulate))
        assert (u32(want) != u32(np.full_like(want, GARBAGE))).any()


# ---- 2. a random HDR map against the yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_an_hdr_map_equals_the_yardstick(rt, orc, ctx, models_dir, name):
    objs, _ = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams = cameras(rt)
    paths = paths_of(rt, orc, models_dir, name, cams, TIMES)
    reads = np.concatenate([r.reshape(-1, 3) for r in check_both_modes(rt, ctx, scene, hdr_map(16), TINT, cams, TIMES, paths, name)])
    # the map matters: its samples read many texels, and the frames differ from the constant sky's
    assert len({tuple(r) for r in reads[reads[:, 0] >= 0]}) > 20, name
    assert_frames(rt.render_sky(ctx, scene, rt.Sky(ctx, hdr_map(16)), cams, rt.RenderData(SPP, LIMIT, True, TINT), TIMES),
                  S.separate(shaded(paths, hdr_map(16), TINT)[0]), (name, "host form"))


@pytest.mark.parametrize("n", FACE_SIZES)
def test_every_face_size(rt, orc, ctx, models_dir, n):
    name = "three_sphere"
    objs, _ = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams = cameras(rt)
    check_both_modes(rt, ctx, scene, hdr_map(n), TINT, cams, TIMES, paths_of(rt, orc, models_dir, name, cams, TIMES), (name, n))


SHAPE_CASES = [(s, (plan(s)[1] or ["unreachable"])[0]) for s in SHAPES]


@pytest.mark.parametrize("shape,name", SHAPE_CASES, ids=["%s-%s" % (_id(s), n) for s, n in SHAPE_CASES])
def test_every_shape(rt, orc, ctx, models_dir, monkeypatch, shape, name):
    env, scenes = plan(shape)
    assert scenes, "RT_SHAPES has the shape %s and tests/test_gpu_shapes.py has no scene that reaches it" % (shape,)
    objs, _ = scene_of(rt, name)
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    cams = cameras(rt)
    check_both_modes(rt, ctx, scene, hdr_map(7), TINT, cams, TIMES, paths_of(rt, orc, models_dir, name, cams, TIMES), (name, shape))


@pytest.mark.parametrize("row", list(KNOB_ROWS))
def test_knobs_do_not_change_a_frame(rt, orc, models_dir, monkeypatch, row):
    objs, _ = scene_of(rt, "monkey")
    with monkeypatch.context() as m:
        for k in [k for k in os.environ if k.startswith("RT_AMD_") and k not in ("RT_AMD_LIB", "RT_AMD_NO_TORCH")]:
            m.delenv(k)
        for k, v in KNOB_ROWS[row].items():
            m.setenv(k, v)
        own = rt.Context(0)                                           # the knobs are read here
    scene = commit_as(rt, own, monkeypatch, objs, models_dir, {})
    cams = cameras(rt)
    check_both_modes(rt, own, scene, hdr_map(7), TINT, cams, TIMES, paths_of(rt, orc, models_dir, "monkey", cams, TIMES), row)
    del scene, own


# ---- 3. the lookup alone ------------------------------------------------------------------------------------------------------------------------
LONE = [("sphere", (0.0, 0.0, 2.0), 0.3, ("standard", (0.5, 0.5, 0.5), 0.0))]
AXES = [(0.0, 0.0, 0.0), (0.0, math.pi / 2, 0.0), (0.0, math.pi, 0.0), (0.0, -math.pi / 2, 0.0), (math.pi / 2, 0.0, 0.0), (-math.pi / 2, 0.0, 0.0)]


@pytest.mark.parametrize("n", FACE_SIZES)
def test_a_primary_ray_that_misses_reads_its_texel(rt, orc, ctx, models_dir, n):
    """antialias off, one sample, one bounce: a pixel whose primary ray misses is texel * tint of the lookup of that ray, the ray taken from
    the AOV plane of primary directions"""
    scene = ctx.commit(rt.SceneObjects(LONE, models_dir))
    cams = [rt.Camera(W, H, fov=2.4, rot=r) for r in AXES]                       # 137 degrees across, 111 up and down
    times = list(range(6))
    faces = hdr_map(n)
    tint = np.asarray(TINT, F)
    got = on_device(rt, ctx, scene, rt.Sky(ctx, faces), cams, rt.RenderData(1, 1, False, TINT), times)
    seen = set()
    for i, cam in enumerate(cams):
        aov = rt.render_aov(ctx, scene, cam, planes=("object", "ray"))
        miss = aov["object"] < 0
        assert miss.sum() > W * H // 2, i
        face, row, col = S.lookup(aov["ray"], n)
        want = S.fold(None, (faces[face, row, col] * tint) * F(1.0), 0)
        assert np.array_equal(u32(got[i])[miss], u32(want)[miss]), (n, i, int((u32(got[i]) != u32(want))[miss].any(axis=-1).sum()))
        seen |= set(zip(face[miss].tolist(), row[miss].tolist(), col[miss].tolist()))
    # ... and the yardstick reads the same texels: all six faces, and of a small map every texel
    paths = paths_of(rt, orc, models_dir, "lone", cams, times, tag="axes", objs=LONE, spp=1, limit=1, antialias=False)
    means, reads = shaded(paths, faces, TINT)
    assert_frames(got, S.separate(means), ("yardstick", n))
    read = {tuple(r) for r in np.concatenate([r.reshape(-1, 3) for r in reads]).tolist() if r[0] >= 0}
    assert read == seen and {r[0] for r in read} == set(range(6)), n
    if n <= 3:
        assert len(read) == 6 * n * n, (n, len(read))


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_sphere", "monkey"])
def test_edges(rt, orc, ctx, models_dir, name):
    objs, _ = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams = cameras(rt)
    faces = hdr_map(16)
    sky = rt.Sky(ctx, faces)
    rd = rt.RenderData(SPP, LIMIT, True, TINT)
    means, _ = shaded(paths_of(rt, orc, models_dir, name, cams, TIMES), faces, TINT)
    # one view, in both modes; a frame number above 0 over a previous frame
    assert_frames(on_device(rt, ctx, scene, sky, cams[1:2], rd, TIMES[1:2]), S.separate(means[1:2]), (name, "one view"))
    assert_frames(on_device(rt, ctx, scene, sky, cams[1:2], rd, TIMES[1:2], accumulate=True), S.accumulated(means[1:2]), (name, "one view, accumulated"))
    first = S.accumulated(means[:1])
    assert_frames(on_device(rt, ctx, scene, sky, cams[1:], rd, TIMES[1:], accumulate=True, frame_num=1, start=first), S.accumulated(means), (name, "from frame 1"))
    assert_frames(rt.render_sky(ctx, scene, sky, cams[1:], rd, TIMES[1:], accumulate=True, frame_num=1, frame=first), S.accumulated(means), (name, "host form from frame 1"))
    again = S.accumulated(means[1:], frame_num=7, prev=first)
    assert_frames(on_device(rt, ctx, scene, sky, cams[1:], rd, TIMES[1:], accumulate=True, frame_num=7, start=first), again, (name, "from frame 7"))
    # RT_VIEWS_MAX views of a 16 x 8 image at one sample: every frame index, a two-tile schedule; one camera repeated is a progressive batch
    assert rt.VIEWS_MAX == 32 and ctx.max_batch_frames(16, 8) >= 32
    orbit = [rt.Camera(16, 8, pos=(0.02 * i, 0.0, -0.01 * i), rot=(0.0, 0.01 * i, 0.0)) for i in range(16)] + [rt.Camera(16, 8)] * 16
    times = [1000 + 17 * i for i in range(32)]
    one = rt.RenderData(1, LIMIT, True, TINT)
    m32, _ = shaded(paths_of(rt, orc, models_dir, name, orbit, times, tag="orbit32", w=16, h=8, spp=1), faces, TINT)
    assert_frames(on_device(rt, ctx, scene, sky, orbit, one, times), S.separate(m32), (name, "32 views"))
    assert_frames(on_device(rt, ctx, scene, sky, orbit, one, times, accumulate=True), S.accumulated(m32), (name, "32 views, accumulated"))
    # a 1 x 1 image; a face size of 1
    tiny = [rt.Camera(1, 1), rt.Camera(1, 1, rot=(0.0, math.pi, 0.0))]
    check_both_modes(rt, ctx, scene, faces, TINT, tiny, TIMES[:2], paths_of(rt, orc, models_dir, name, tiny, TIMES[:2], tag="1x1", w=1, h=1), (name, "1 x 1"))
    check_both_modes(rt, ctx, scene, hdr_map(1), TINT, cams, TIMES, paths_of(rt, orc, models_dir, name, cams, TIMES), (name, "a face of one texel"))


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_frames_untouched(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    objs, sky_colour = scene_of(rt, "three_sphere")
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    other = rt.Context(0)
    foreign_scene = other.commit(rt.SceneObjects(objs, models_dir))
    sky, foreign_sky = rt.Sky(ctx, hdr_map(2)), rt.Sky(other, hdr_map(2))
    n = 3
    arr = (rt.rt_camera * 40)(*[rt.Camera(W, H).c for _ in range(40)])
    times = (C.c_int32 * 40)(*range(40))
    rd, neg = rt.RenderData(SPP, LIMIT, True, sky_colour), rt.RenderData(SPP, -1, True, sky_colour)
    t = torch.full((n, H, W, 3), float(GARBAGE), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    host = np.full((n, H, W, 3), GARBAGE, F)
    fn = C.c_int32(0)
    good_d = (ctx._h, scene._h, sky._h, arr, times, n, C.byref(rd.c), 0, 0, C.c_void_p(t.data_ptr()), None)
    good_h = (ctx._h, scene._h, sky._h, arr, times, n, C.byref(rd.c), 0, C.byref(fn), host.ctypes.data_as(C.POINTER(C.c_float)))

    def with_(good, i, v, j=None, w=None):
        a = good[:i] + (v,) + good[i + 1:]
        return a if j is None else a[:j] + (w,) + a[j + 1:]

    def odd(i, **kw):
        a = (rt.rt_camera * 40)(*[rt.Camera(W, H).c for _ in range(40)])
        for k, v in kw.items():
            setattr(a[i], k, v)
        return a

    bad = [(1, None, "null"), (2, None, "null"), (3, None, "null"), (4, None, "null"), (6, None, "null"), (9, None, "null"), (1, foreign_scene._h, "another context"),
           (2, foreign_sky._h, "sky belongs to another context"), (5, 0, "number of views"), (5, -1, "number of views"), (6, C.byref(neg.c), "render settings"),
           (3, odd(0, width=0), "image size"), (3, odd(0, width=40000), "image size"), (3, odd(2, width=W + 1), "share one image size")]
    for i, v, msg in bad:
        assert L.rt_render_sky_device(*with_(good_d, i, v)) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        assert L.rt_render_sky(*with_(good_h, i, v)) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
    assert L.rt_render_sky_device(*with_(good_d, 5, 33)) == rt.RT_ERR_INVALID and "number of views" in ctx.last_error()
    assert L.rt_render_sky_device(*with_(good_d, 8, -1)) == rt.RT_ERR_INVALID and "frame number" in ctx.last_error()
    assert L.rt_render_sky_device(*with_(good_d, 8, 2)) == rt.RT_ERR_INVALID and "frame number" in ctx.last_error()
    assert L.rt_render_sky(*with_(good_h, 8, None)) == rt.RT_ERR_INVALID and "null" in ctx.last_error()
    assert L.rt_render_sky_device(None, scene._h, sky._h, arr, times, n, C.byref(rd.c), 0, 0, C.c_void_p(t.data_ptr()), None) == rt.RT_ERR_INVALID
    # the sky's own constructor
    faces = hdr_map(2)
    fp, out = faces.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p()
    for args in ((None, 2, fp, C.byref(out)), (ctx._h, 2, None, C.byref(out)), (ctx._h, 2, fp, None), (ctx._h, 0, fp, C.byref(out)), (ctx._h, -3, fp, C.byref(out)),
                 (ctx._h, rt.SKY_MAX_FACE + 1, fp, C.byref(out))):
        assert L.rt_sky_create(*args) == rt.RT_ERR_INVALID and not out.value, args[1]
    with pytest.raises(ValueError, match=r"\[6, n, n, 3\]"):
        rt.Sky(ctx, np.zeros((6, 2, 3, 3), F))
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((t == float(GARBAGE)).all()) and np.all(host == GARBAGE) and fn.value == 0
    # ... and the good call goes through
    assert L.rt_render_sky_device(*good_d) == rt.RT_OK
    ctx.synchronize()
    assert not bool((t == float(GARBAGE)).all())
    del sky, foreign_sky, foreign_scene, other


# ---- 6. the launch order ------------------------------------------------------------------------------------------------------------------------
def test_a_consumer_queued_behind_the_call_sees_the_frames(rt, orc, ctx, models_dir):
    """the call on a caller's stream, a copy queued behind it on that stream, no host wait in between: the copy holds what the synchronised
    call gives"""
    import torch
    name = "monkey"
    objs, _ = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams, rd = cameras(rt), rt.RenderData(SPP, LIMIT, True, TINT)
    sky = rt.Sky(ctx, hdr_map(16))
    want = on_device(rt, ctx, scene, sky, cams, rd, TIMES)
    s = torch.cuda.Stream(device="cuda:0")
    t = torch.full((len(cams), H, W, 3), float(GARBAGE), dtype=torch.float32, device="cuda:0")
    t_copy = torch.zeros_like(t)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rt.render_sky_device(ctx, scene, sky, cams, rd, TIMES, t.data_ptr(), stream=s.cuda_stream)
        t_copy.copy_(t, non_blocking=True)
    s.synchronize()
    assert_frames(t_copy.cpu().numpy(), want, "caller's stream")
    assert_frames(want, S.separate(shaded(paths_of(rt, orc, models_dir, name, cams, TIMES), hdr_map(16), TINT)[0]), "the synchronised call")


# ---- 7. the C++ mirror --------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_example(rt, ctx, models_dir, tmp_path):
    """host/example_sky.cpp (Sky, Renderer::create_sky, Renderer::render_sky of host/raytracer.hpp): it builds, checks a white map against the
    constant sky itself, and its frame is the Python call's under the map it wrote"""
    import subprocess
    exe = rt.build.build_sky_example()
    w, h, n = 72, 56, 16
    r = subprocess.run([exe, models_dir, str(w), str(h), str(n), str(tmp_path / "sky")], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "sky ok: %d x %d under a %d-texel cube map" % (w, h, n) in r.stdout, r.stdout[-3000:]
    assert os.path.getsize(str(tmp_path / "sky.png")) > 1000
    faces = np.fromfile(str(tmp_path / "sky_sky.f32"), F).reshape(6, n, n, 3)
    frame = np.fromfile(str(tmp_path / "sky_frame.f32"), F).reshape(1, h, w, 3)
    assert len(np.unique(u32(faces).reshape(-1, 3), axis=0)) > n                                                   # a gradient, not a flat map
    objs = [("obj", "low_poly_monkey.obj", [("enlarge", 0.3), ("rotate", 0, 2.3, 0), ("translate", 0.1, -0.1, 1.6)], ("standard", (0.9, 0.9, 0.9), 0.2)),
            ("sphere", (0, -100.5, 1.5), 100, ("standard", (0.5, 0.5, 0.5), 0.3))]
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    got = rt.render_sky(ctx, scene, rt.Sky(ctx, faces), [rt.Camera(w, h)], rt.RenderData(32, 5, True, (1, 1, 1)), [12345])
    assert_frames(got, frame, "the example's frame")
    assert np.isfinite(frame).all() and frame.any()
