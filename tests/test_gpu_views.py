"""Camera sequences on the device (rt_render_views[_device]): many views of a scene in one launch against their yardstick (tests/views_ref.py:
one oracle render per view with that view's camera, chained for the accumulate mode) and against the product's own one-view renderer.
Every frame is compared as uint32 on every pixel, never to a tolerance.  The oracle's answers are computed once per case and shared.
Run with -m gpu on an MI355X."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import views_ref as R
from test_gpu_query import u32
from test_gpu_shapes import KNOB_ROWS, MESH_SCENES, NO_MESH_SCENES, SHAPES, _id, commit_as, plan, scene_of

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 37, 21                       # 5 x 3 tiles, ragged on both axes
SPP, LIMIT = 3, 5
TIMES = [12345, -99, 777, 31337, 4242]
MORE_TIMES = [5150, -7, 2024]
GARBAGE = F(7.0)
SCENES = NO_MESH_SCENES + MESH_SCENES + ["reference_scene1"]
_CACHE = {}


def cameras(rt, w=W, h=H):
    """the default; one translated; one rotated; one turned away from the scene (about the y axis by pi); the first again (another seed)"""
    return [rt.Camera(w, h), rt.Camera(w, h, pos=(0.3, 0.1, -0.2)), rt.Camera(w, h, pos=(0.2, 0.0, 0.1), rot=(0.05, -0.2, 0.1)),
            rt.Camera(w, h, rot=(0.0, math.pi, 0.0)), rt.Camera(w, h)]


def more_cameras(rt, w=W, h=H):
    return [rt.Camera(w, h, pos=(-0.2, 0.05, 0.0)), rt.Camera(w, h, rot=(0.0, 0.15, 0.0)), rt.Camera(w, h, pos=(0.0, 0.2, -0.3), rot=(0.1, 0.0, 0.0))]


def oracle_of(rt, orc, models_dir, name):
    key = ("oracle", name)
    if key not in _CACHE:
        objs, sky = scene_of(rt, name)
        _CACHE[key] = (orc.Scene(objs, orc.MATH_DET, models_dir), sky)
    return _CACHE[key]


def ref(rt, orc, models_dir, name, tag, make):
    """make(oracle, sky) once per (scene, tag)"""
    key = ("ref", name, tag)
    if key not in _CACHE:
        _CACHE[key] = make(*oracle_of(rt, orc, models_dir, name))
    return _CACHE[key]


def ref_separate(rt, orc, models_dir, name, cams, times, w=W, h=H, spp=SPP, limit=LIMIT, antialias=True, tag="separate"):
    fl = [c.floats() for c in cams]
    return ref(rt, orc, models_dir, name, tag, lambda o, sky: R.separate(o, fl, w, h, spp, limit, sky, times, antialias))


def ref_accumulated(rt, orc, models_dir, name, cams, times, frame_num=0, prev=None, w=W, h=H, spp=SPP, limit=LIMIT, antialias=True, tag="accumulated"):
    fl = [c.floats() for c in cams]
    return ref(rt, orc, models_dir, name, tag, lambda o, sky: R.accumulated(o, fl, w, h, spp, limit, sky, times, frame_num, prev, antialias))


def assert_frames(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    diff = u32(got) != u32(want)
    assert not diff.any(), (what, "pixels that differ per frame", diff.reshape(-1, got.shape[-3] * got.shape[-2], 3).any(axis=2).sum(axis=1).tolist())


def on_device(rt, ctx, scene, cams, rd, times, accumulate=False, frame_num=0, start=None, stream=None):
    """rt_render_views_device over a buffer of garbage (or `start`); -> the frames"""
    import torch
    h, w = cams[0].height, cams[0].width
    shape = (h, w, 3) if accumulate else (len(cams), h, w, 3)
    t = torch.from_numpy(np.full(shape, GARBAGE, F) if start is None else np.ascontiguousarray(start, F)).to("cuda:0")
    torch.cuda.synchronize()
    rt.render_views_device(ctx, scene, cams, rd, times, t.data_ptr(), accumulate=accumulate, frame_num=frame_num, stream=stream)
    ctx.synchronize()
    return t.cpu().numpy()


def single_launches(rt, ctx, scene, cams, rd, times, data=None):
    """the product's own one-view renderer: rt_render per camera; data None: each a frame 0 (-> [n, H, W, 3]), else chained in `data`"""
    if data is not None:
        for c, t in zip(cams, times):
            rt.render(ctx, scene, c, rd, data, t)
        return data.previous_render
    out = []
    for c, t in zip(cams, times):
        one = rt.VariableRenderData(c.width, c.height)
        rt.render(ctx, scene, c, rd, one, t)
        out.append(one.previous_render.copy())
    return np.stack(out)


# ---- 1. separate frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_separate_frames_equal_the_oracle_and_the_one_view_renderer(rt, orc, ctx, models_dir, name):
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams, rd = cameras(rt), rt.RenderData(SPP, LIMIT, True, sky)
    want = ref_separate(rt, orc, models_dir, name, cams, TIMES)
    got = on_device(rt, ctx, scene, cams, rd, TIMES)
    assert ctx.last_kernel_ms() > 0
    assert_frames(got, want, (name, "oracle"))
    assert_frames(got, single_launches(rt, ctx, scene, cams, rd, TIMES), (name, "rt_render_device"))
    # the views differ from one another (the last is the first with another seed), so a mixed-up camera or seed cannot pass
    assert len({want[i].tobytes() for i in range(len(cams))}) == len(cams), name
    assert_frames(rt.render_views(ctx, scene, cams, rd, TIMES), want, (name, "host form"))


# ---- 2. one accumulated frame -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey", "reference_scene0"])
def test_accumulated_frame_equals_the_oracles_chain(rt, orc, ctx, models_dir, name):
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams, more, rd = cameras(rt), more_cameras(rt), rt.RenderData(SPP, LIMIT, True, sky)
    want5 = ref_accumulated(rt, orc, models_dir, name, cams, TIMES, tag="acc5")
    want8 = ref_accumulated(rt, orc, models_dir, name, more, MORE_TIMES, frame_num=5, prev=want5, tag="acc8")
    got5 = on_device(rt, ctx, scene, cams, rd, TIMES, accumulate=True)                                   # from frame 0 over garbage
    assert_frames(got5, want5, (name, "five views from frame 0"))
    got8 = on_device(rt, ctx, scene, more, rd, MORE_TIMES, accumulate=True, frame_num=5, start=got5)     # a second call goes on
    assert_frames(got8, want8, (name, "three more from frame 5"))
    data = rt.VariableRenderData(W, H)
    assert_frames(single_launches(rt, ctx, scene, cams + more, rd, TIMES + MORE_TIMES, data), want8, (name, "chained rt_render_device"))
    assert data.frame_num == 8
    assert_frames(rt.render_views(ctx, scene, more, rd, MORE_TIMES, accumulate=True, frame_num=5, frame=want5), want8, (name, "host form"))
    # identical cameras: the multi-frame launch of one view
    same = [rt.Camera(W, H, pos=(0.3, 0.1, -0.2)) for _ in TIMES]
    batch = rt.VariableRenderData(W, H)
    rt.render_frames(ctx, scene, same[0], rd, batch, TIMES)
    assert_frames(on_device(rt, ctx, scene, same, rd, TIMES, accumulate=True), batch.previous_render, (name, "rt_render_device_batch"))


# ---- 3. every kernel shape ----------------------------------------------------------------------------------------------------------------
SHAPE_CASES = [(s, (plan(s)[1] or ["unreachable"])[0]) for s in SHAPES]


@pytest.mark.parametrize("shape,name", SHAPE_CASES, ids=["%s-%s" % (_id(s), n) for s, n in SHAPE_CASES])
def test_every_shape_equals_the_oracle(rt, orc, ctx, models_dir, monkeypatch, shape, name):
    env, scenes = plan(shape)
    assert scenes, "RT_SHAPES has the shape %s and tests/test_gpu_shapes.py has no scene that reaches it" % (shape,)
    objs, sky = scene_of(rt, name)
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    cams, times, rd = cameras(rt)[:3], TIMES[:3], rt.RenderData(SPP, LIMIT, True, sky)
    assert_frames(on_device(rt, ctx, scene, cams, rd, times), ref_separate(rt, orc, models_dir, name, cams, times, tag="separate3"), (name, shape))
    assert_frames(on_device(rt, ctx, scene, cams, rd, times, accumulate=True), ref_accumulated(rt, orc, models_dir, name, cams, times, tag="acc3"),
                  (name, shape, "accumulated"))


# ---- 4. the scheduling knobs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(KNOB_ROWS))
def test_knobs_do_not_change_a_view(rt, orc, models_dir, monkeypatch, row):
    objs, sky = scene_of(rt, "monkey")
    with monkeypatch.context() as m:
        for k in [k for k in os.environ if k.startswith("RT_AMD_") and k not in ("RT_AMD_LIB", "RT_AMD_NO_TORCH")]:
            m.delenv(k)
        for k, v in KNOB_ROWS[row].items():
            m.setenv(k, v)
        ctx = rt.Context(0)                                           # the knobs are read here
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {})
    cams, times, rd = cameras(rt)[:3], TIMES[:3], rt.RenderData(SPP, LIMIT, True, sky)
    assert_frames(on_device(rt, ctx, scene, cams, rd, times), ref_separate(rt, orc, models_dir, "monkey", cams, times, tag="separate3"), row)
    assert_frames(on_device(rt, ctx, scene, cams, rd, times, accumulate=True), ref_accumulated(rt, orc, models_dir, "monkey", cams, times, tag="acc3"),
                  (row, "accumulated"))
    del scene, ctx


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_sphere", "monkey"])
def test_edges(rt, orc, ctx, models_dir, name):
    import torch
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams, rd = cameras(rt), rt.RenderData(SPP, LIMIT, True, sky)
    want = ref_separate(rt, orc, models_dir, name, cams, TIMES)
    # one view
    assert_frames(on_device(rt, ctx, scene, cams[1:2], rd, TIMES[1:2]), want[1:2], (name, "one view"))
    assert_frames(on_device(rt, ctx, scene, cams[1:2], rd, TIMES[1:2], accumulate=True), want[1], (name, "one view, accumulated"))
    # 32 views of a 16 x 8 image at one sample: every frame index, a two-tile schedule
    orbit = [rt.Camera(16, 8, pos=(0.02 * i, 0.0, -0.01 * i), rot=(0.0, 0.01 * i, 0.0)) for i in range(40)]
    times = [1000 + 17 * i for i in range(40)]
    one = rt.RenderData(1, LIMIT, True, sky)
    want40 = ref_separate(rt, orc, models_dir, name, orbit, times, w=16, h=8, spp=1, tag="orbit40")
    acc40 = ref_accumulated(rt, orc, models_dir, name, orbit, times, w=16, h=8, spp=1, tag="orbit40acc")
    acc32 = ref_accumulated(rt, orc, models_dir, name, orbit[:32], times[:32], w=16, h=8, spp=1, tag="orbit32acc")
    assert rt.VIEWS_MAX == 32 and ctx.max_batch_frames(16, 8) >= 32
    assert_frames(on_device(rt, ctx, scene, orbit[:32], one, times[:32]), want40[:32], (name, "32 views"))
    assert_frames(on_device(rt, ctx, scene, orbit[:32], one, times[:32], accumulate=True), acc32, (name, "32 views, accumulated"))
    # the host form with 40 views: two launches, in both modes
    assert_frames(rt.render_views(ctx, scene, orbit, one, times), want40, (name, "40 views, host form"))
    assert_frames(rt.render_views(ctx, scene, orbit, one, times, accumulate=True), acc40, (name, "40 views, host form, accumulated"))
    # a 1 x 1 image
    tiny = [rt.Camera(1, 1), rt.Camera(1, 1, pos=(0.1, 0.0, 0.0))]
    assert_frames(on_device(rt, ctx, scene, tiny, rd, TIMES[:2]), ref_separate(rt, orc, models_dir, name, tiny, TIMES[:2], w=1, h=1, tag="1x1"), (name, "1 x 1"))
    # antialias off; a bounce limit of 0; one sample per pixel
    for tag, data, kw in (("no-aa", rt.RenderData(SPP, LIMIT, False, sky), dict(antialias=False)), ("limit0", rt.RenderData(SPP, 0, True, sky), dict(limit=0)),
                          ("spp1", rt.RenderData(1, LIMIT, True, sky), dict(spp=1))):
        w3 = ref_separate(rt, orc, models_dir, name, cams[:3], TIMES[:3], tag=tag, **kw)
        assert_frames(on_device(rt, ctx, scene, cams[:3], data, TIMES[:3]), w3, (name, tag))
        assert_frames(on_device(rt, ctx, scene, cams[:3], data, TIMES[:3], accumulate=True),
                      ref_accumulated(rt, orc, models_dir, name, cams[:3], TIMES[:3], tag=tag + "-acc", **kw), (name, tag, "accumulated"))
        assert tag != "limit0" or not w3.any()
    # a caller's stream, ordered against a copy behind it
    s = torch.cuda.Stream(device="cuda:0")
    t = torch.full((len(cams), H, W, 3), float(GARBAGE), dtype=torch.float32, device="cuda:0")
    t_copy = torch.zeros_like(t)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rt.render_views_device(ctx, scene, cams, rd, TIMES, t.data_ptr(), stream=s.cuda_stream)
        t_copy.copy_(t, non_blocking=True)
    s.synchronize()
    assert_frames(t_copy.cpu().numpy(), want, (name, "caller's stream"))


# ---- 6. the context's state ---------------------------------------------------------------------------------------------------------------
def test_the_cached_view_and_the_frames_in_flight_are_left_alone(rt, orc, models_dir):
    import torch
    ctx = rt.Context(0)
    name = "monkey"
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cams, rd = cameras(rt), rt.RenderData(SPP, LIMIT, True, sky)
    want = ref_separate(rt, orc, models_dir, name, cams, TIMES)
    old = cams[1]
    # a warm view: rendered twice, its measured costs read
    for _ in range(2):
        one = rt.VariableRenderData(W, H)
        rt.render(ctx, scene, old, rd, one, TIMES[1])
    assert_frames(one.previous_render, want[1], "warm view")
    before = ctx.tile_costs(with_peaks=True)
    assert len(before[0]) == 15 and before[1].any()
    assert_frames(on_device(rt, ctx, scene, cams, rd, TIMES), want, "views launch")
    assert_frames(on_device(rt, ctx, scene, cams, rd, TIMES, accumulate=True), ref_accumulated(rt, orc, models_dir, name, cams, TIMES, tag="acc5"), "views launch")
    after = ctx.tile_costs(with_peaks=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    again = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, old, rd, again, TIMES[1])
    assert_frames(again.previous_render, want[1], "the old view after the views launch")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, ctx.tile_costs(with_peaks=True)))
    # two frames in flight, a views launch queued behind them, then the frames collected
    chain = ref_accumulated(rt, orc, models_dir, name, [old, old], [TIMES[1], 555], tag="pipelined2")
    rt.frame_depth(ctx, 2)
    rt.frame_submit(ctx, scene, old, rd, TIMES[1])
    rt.frame_submit(ctx, scene, old, rd, 555)
    got = on_device(rt, ctx, scene, cams, rd, TIMES)
    fr = torch.full((H, W, 3), float(GARBAGE), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rt.frame_collect(ctx, 0, fr.data_ptr())
    rt.frame_collect(ctx, 1, fr.data_ptr())
    rt.frame_wait(ctx)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert rt.frames_pending(ctx) == 0
    assert_frames(got, want, "views launch behind two frames in flight")
    assert_frames(fr.cpu().numpy(), chain, "the two pipelined frames")


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_frames_untouched(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    objs, sky = scene_of(rt, "three_sphere")
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objs, models_dir))
    n = 3
    arr = (rt.rt_camera * 40)(*[rt.Camera(W, H).c for _ in range(40)])
    times = (C.c_int32 * 40)(*range(40))
    rd, neg = rt.RenderData(SPP, LIMIT, True, sky), rt.RenderData(SPP, -1, True, sky)
    t = torch.full((n, H, W, 3), float(GARBAGE), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    host = np.full((n, H, W, 3), GARBAGE, F)
    fn = C.c_int32(0)
    good_d = (ctx._h, scene._h, arr, times, n, C.byref(rd.c), 0, 0, C.c_void_p(t.data_ptr()), None)
    good_h = (ctx._h, scene._h, arr, times, n, C.byref(rd.c), 0, C.byref(fn), host.ctypes.data_as(C.POINTER(C.c_float)))

    def with_(good, i, v, j=None, w=None):
        a = good[:i] + (v,) + good[i + 1:]
        return a if j is None else a[:j] + (w,) + a[j + 1:]

    def odd(i, **kw):
        a = (rt.rt_camera * 40)(*[rt.Camera(W, H).c for _ in range(40)])
        for k, v in kw.items():
            setattr(a[i], k, v)
        return a

    bad = [(1, None, "null"), (2, None, "null"), (3, None, "null"), (5, None, "null"), (8, None, "null"), (1, foreign._h, "another context"),
           (4, 0, "number of views"), (4, -1, "number of views"), (5, C.byref(neg.c), "render settings"),
           (2, odd(0, width=0), "image size"), (2, odd(0, height=-3), "image size"), (2, odd(0, width=40000), "image size"),
           (2, odd(2, width=W + 1), "share one image size"), (2, odd(1, height=H - 1), "share one image size")]
    for i, v, msg in bad:
        assert L.rt_render_views_device(*with_(good_d, i, v)) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        assert L.rt_render_views(*with_(good_h, i, v)) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
    # the device form alone: more than one launch's views; frame numbers
    assert L.rt_render_views_device(*with_(good_d, 4, 33)) == rt.RT_ERR_INVALID and "number of views" in ctx.last_error()
    assert L.rt_render_views_device(*with_(good_d, 7, -1)) == rt.RT_ERR_INVALID and "frame number" in ctx.last_error()
    assert L.rt_render_views_device(*with_(good_d, 7, 2)) == rt.RT_ERR_INVALID and "frame number" in ctx.last_error()
    assert L.rt_render_views_device(*with_(good_d, 6, 1, 7, -1)) == rt.RT_ERR_INVALID and "frame number" in ctx.last_error()
    for value in (-1, 2):
        fnb = C.c_int32(value)
        assert L.rt_render_views(*with_(good_h, 7, C.byref(fnb))) == rt.RT_ERR_INVALID and "frame number" in ctx.last_error() and fnb.value == value
    fnb = C.c_int32(-4)
    assert L.rt_render_views(*with_(good_h, 6, 1, 7, C.byref(fnb))) == rt.RT_ERR_INVALID and "frame number" in ctx.last_error() and fnb.value == -4
    assert L.rt_render_views(*with_(good_h, 7, None)) == rt.RT_ERR_INVALID and "null" in ctx.last_error()
    assert L.rt_render_views_device(None, scene._h, arr, times, n, C.byref(rd.c), 0, 0, C.c_void_p(t.data_ptr()), None) == rt.RT_ERR_INVALID
    assert L.rt_render_views(None, scene._h, arr, times, n, C.byref(rd.c), 0, C.byref(fn), host.ctypes.data_as(C.POINTER(C.c_float))) == rt.RT_ERR_INVALID
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((t == float(GARBAGE)).all()) and np.all(host == GARBAGE) and fn.value == 0
    # ... and the good call goes through
    assert L.rt_render_views_device(*good_d) == rt.RT_OK
    ctx.synchronize()
    assert not bool((t == float(GARBAGE)).all())
    with pytest.raises(ValueError, match="one time_ms per camera"):
        rt.render_views(ctx, scene, cameras(rt), rd, TIMES[:2])


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_example(rt, models_dir, tmp_path):
    """host/example_views.cpp (Renderer::render_views, Camera::lens, lens_cameras of host/raytracer.hpp), like the other C++ mirror tests: it
    checks every view of an orbit and a depth-of-field frame against Renderer::render itself and writes the pictures"""
    import subprocess
    exe = rt.build.build_views_example()
    r = subprocess.run([exe, models_dir, "72", "56", "5", str(tmp_path / "views")], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "views ok: 5 views of 72 x 56" in r.stdout, r.stdout[-3000:]
    for name in ("views_000.png", "views_004.png", "views_dof.png"):
        assert os.path.getsize(str(tmp_path / name)) > 1000, name
