"""Per-pixel sample budgets and the adaptive sampling loop on the device (rt_render_budget[_device], rt_adaptive_plan_device,
rt_render_adaptive) against their yardstick (tests/adaptive_ref.py: the definitions in NumPy float32 over the CPU oracle's renderer) and
against the product's own renderer.  Frames are compared as uint32, counts and budgets as bytes, on every pixel, never to a tolerance.  The
yardstick's answers are computed once per case and shared.  Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as R
from test_gpu_query import u32
from test_gpu_shapes import SHAPES, _id, commit_as, plan, scene_of

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 37, 21                       # 5 x 3 tiles, ragged on both axes
TILES_X = 5
LIMIT = 5
SEED, SEED2 = 12345, -99
GARBAGE = F(7.0)
_CACHE = {}


def budget_plane(big=False):
    """a fixed draw from {0, 0, 1, 2, 5, 17}; tile 6 all zero, tile 7 with one pixel at slot 0, tile 2 with one at slot 63; big: one
    pixel of 4096 samples"""
    b = np.random.default_rng(2024).choice(np.array([0, 0, 1, 2, 5, 17], np.uint16), size=(H, W))
    b[8:16, 8:16] = 0               # tile 6 = (ty 1, tx 1)
    b[8:16, 16:24] = 0              # tile 7
    b[8, 16] = 3                    # ... slot 0
    b[0:8, 16:24] = 0               # tile 2
    b[7, 23] = 2                    # ... slot 63
    if big:
        b[12, 2] = 4096
    assert (b[16:, 32:] > 0).any() and (b == 0).sum() > W * H // 4 and sorted(set(b.ravel()) - {3, 4096}) == [0, 1, 2, 5, 17]
    return b


def oracle_of(rt, orc, models_dir, name):
    key = ("oracle", name)
    if key not in _CACHE:
        objs, sky = scene_of(rt, name)
        _CACHE[key] = (orc.Scene(objs, orc.MATH_DET, models_dir), sky)
    return _CACHE[key]


def ref_budget(rt, orc, models_dir, name, budget, limit, seed, frame=None, count=None, antialias=True, tile_list=None, tag=None):
    """the yardstick's (frame, count) after one call, cached under `tag`"""
    key = ("budget", name, tag)
    if tag is None or key not in _CACHE:
        oracle, sky = oracle_of(rt, orc, models_dir, name)
        out = R.budget_render(oracle, rt.Camera(W, H).floats(), W, H, budget, limit, sky, seed, frame, count, antialias, tile_list)
        if tag is None:
            return out
        _CACHE[key] = out
    return _CACHE[key]


def assert_frame(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(u32(got), u32(want)), (what, "frame", int((u32(got) != u32(want)).any(axis=-1).sum()))


def check_scene(rt, orc, ctx, models_dir, name, scene, sky, big=False):
    """every case of the budget render on one committed scene"""
    import torch
    cam, rd = rt.Camera(W, H), rt.RenderData(999, LIMIT, True, sky)          # (rays_per_pixel is not read)
    budget = budget_plane(big)
    dev = torch.device("cuda:0")
    t_budget = torch.from_numpy(budget.view(np.int16)).to(dev)
    garbage = np.full((H, W, 3), GARBAGE, F)
    # (a) counts zero, over a frame of garbage: pixels of budget 0 keep the garbage and a count of 0
    want, want_count = ref_budget(rt, orc, models_dir, name, budget, LIMIT, SEED, garbage, np.zeros((H, W), np.uint32), tag=("a", big))
    t_frame = torch.from_numpy(garbage).to(dev)
    t_count = torch.zeros((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rt.render_budget_device(ctx, scene, cam, rd, SEED, t_budget.data_ptr(), t_frame.data_ptr(), d_count=t_count.data_ptr())
    ctx.synchronize()
    assert ctx.last_kernel_ms() > 0
    assert_frame(t_frame.cpu().numpy(), want, (name, "zero counts"))
    assert t_count.cpu().numpy().view(np.uint32).tobytes() == want_count.tobytes() == budget.astype(np.uint32).tobytes()
    assert np.all(want[budget == 0] == GARBAGE)
    # (b) counts non-zero, from that call: another seed folds into it (pixels of budget 0 had count 0 and keep it)
    want2, want_count2 = ref_budget(rt, orc, models_dir, name, budget, LIMIT, SEED2, want, want_count, tag=("b", big))
    rt.render_budget_device(ctx, scene, cam, rd, SEED2, t_budget.data_ptr(), t_frame.data_ptr(), d_count=t_count.data_ptr())
    ctx.synchronize()
    assert_frame(t_frame.cpu().numpy(), want2, (name, "fold"))
    assert t_count.cpu().numpy().view(np.uint32).tobytes() == want_count2.tobytes() == (2 * budget.astype(np.uint32)).tobytes()
    assert not np.array_equal(u32(want2[budget > 0]), u32(want[budget > 0]))
    # ... with counts that differ from the budgets: the first call's budgets permuted, so that n != m for most pixels (host form)
    other = np.ascontiguousarray(budget[::-1, ::-1])
    want3, want_count3 = ref_budget(rt, orc, models_dir, name, other, LIMIT, SEED2, want, want_count, tag=("b2", big)) if not big else (None, None)
    if not big:
        got3, got_count3 = rt.render_budget(ctx, scene, cam, rd, SEED2, other, want, want_count)
        assert_frame(got3, want3, (name, "fold, n != m"))
        assert got_count3.tobytes() == want_count3.tobytes() and ((other > 0) & (budget > 0) & (other != budget)).sum() > 50
    # (c) d_count == NULL: every pixel starts from nothing, whatever the frame holds; a caller's stream, ordered against a copy behind it
    t_frame.copy_(torch.from_numpy(garbage))
    t_copy = torch.zeros_like(t_frame)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rt.render_budget_device(ctx, scene, cam, rd, SEED, t_budget.data_ptr(), t_frame.data_ptr(), stream=s.cuda_stream)
        t_copy.copy_(t_frame, non_blocking=True)
    s.synchronize()
    assert_frame(t_copy.cpu().numpy(), want, (name, "no count plane, caller's stream"))
    if big:
        return
    # (d) a tile list that omits tiles, in reverse order: only its tiles' pixels are considered
    tl = [t for t in range(15) if t not in (0, 4, 9)][::-1]
    want_t, want_count_t = ref_budget(rt, orc, models_dir, name, budget, LIMIT, SEED, garbage, np.zeros((H, W), np.uint32), tile_list=tl, tag="tiles")
    got, got_count = rt.render_budget(ctx, scene, cam, rd, SEED, budget, garbage, np.zeros((H, W), np.uint32), tile_list=tl)
    assert_frame(got, want_t, (name, "tile list"))
    assert got_count.tobytes() == want_count_t.tobytes() and not got_count[0:8, 0:8].any() and not got_count[8:16, 32:].any() and got_count[16:, 32:].any()
    assert_frame(rt.render_budget(ctx, scene, cam, rd, SEED, budget, garbage, None, tile_list=[])[0], garbage, (name, "empty list"))
    # (e) reflection_limit 0: (0, 0, 0) where the budget is not 0
    got, got_count = rt.render_budget(ctx, scene, cam, rt.RenderData(999, 0, True, sky), SEED, budget, garbage, None)
    assert np.all(got[budget > 0] == 0) and np.all(got[budget == 0] == GARBAGE) and got_count.tobytes() == want_count.tobytes()
    assert_frame(got, ref_budget(rt, orc, models_dir, name, budget, 0, SEED, garbage, None)[0], (name, "limit 0"))
    # (f) antialias off
    want_f, _ = ref_budget(rt, orc, models_dir, name, budget, LIMIT, SEED, garbage, None, antialias=False, tag="no-aa")
    got, _ = rt.render_budget(ctx, scene, cam, rt.RenderData(999, LIMIT, False, sky), SEED, budget, garbage, None)
    assert_frame(got, want_f, (name, "antialias off"))
    assert not np.array_equal(u32(want_f), u32(want))


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey"])
def test_budget_render_equals_the_yardstick(rt, orc, ctx, models_dir, name):
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    assert scene.info()["scene_in_lds"] == 1
    check_scene(rt, orc, ctx, models_dir, name, scene, sky)


PLACED = [(1, 2, 1024), (1, 0, 1024), (0, 0, 256)]                 # hybrid, global with a mesh, global without: shapes of RT_SHAPES


@pytest.mark.parametrize("shape", PLACED, ids=[_id(s) for s in PLACED])
def test_budget_render_equals_the_yardstick_beyond_lds(rt, orc, ctx, models_dir, monkeypatch, shape):
    """every case of check_scene on the placements tests/test_gpu_shapes.py forces: the hybrid (BVH in LDS, triangles from global memory) and
    the two global ones, each asserted from scene.info()"""
    assert shape in SHAPES
    env, scenes = plan(shape)
    name = scenes[0]
    objs, sky = scene_of(rt, name)
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    check_scene(rt, orc, ctx, models_dir, name, scene, sky)


def test_one_pixel_of_4096_samples(rt, orc, ctx, models_dir):
    objs, sky = scene_of(rt, "three_sphere")
    check_scene(rt, orc, ctx, models_dir, "three_sphere", ctx.commit(rt.SceneObjects(objs, models_dir)), sky, big=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["three_sphere", "monkey"])
def test_a_uniform_budget_is_the_render_kernels_frame(rt, ctx, models_dir, name, n):
    """the product against itself: rt_render_device at rays_per_pixel = n, frame_num = 0"""
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cam = rt.Camera(W, H)
    data = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, cam, rt.RenderData(n, LIMIT, True, sky), data, SEED)
    got, count = rt.render_budget(ctx, scene, cam, rt.RenderData(0, LIMIT, True, sky), SEED, np.full((H, W), n, np.uint16))
    assert_frame(got, data.previous_render, (name, n))
    assert np.all(count == n)


SHAPE_CASES = [(s, (plan(s)[1] or ["unreachable"])[0]) for s in SHAPES]


@pytest.mark.parametrize("shape,name", SHAPE_CASES, ids=["%s-%s" % (_id(s), n) for s, n in SHAPE_CASES])
def test_every_shape_equals_the_yardstick(rt, orc, ctx, models_dir, monkeypatch, shape, name):
    """tests/test_gpu_shapes.py's forcing of every entry of RT_SHAPES, for the budget kernel: the first scene that reaches the shape (the
    hybrid and global placements among them), one 37 x 21 case each: zero counts, then the fold"""
    import torch
    env, scenes = plan(shape)
    assert scenes, "RT_SHAPES has the shape %s and tests/test_gpu_shapes.py has no scene that reaches it" % (shape,)
    objs, sky = scene_of(rt, name)
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    cam, rd = rt.Camera(W, H), rt.RenderData(999, LIMIT, True, sky)
    budget = budget_plane()
    garbage = np.full((H, W, 3), GARBAGE, F)
    want, want_count = ref_budget(rt, orc, models_dir, name, budget, LIMIT, SEED, garbage, np.zeros((H, W), np.uint32), tag=("a", False))
    want2, want_count2 = ref_budget(rt, orc, models_dir, name, budget, LIMIT, SEED2, want, want_count, tag=("b", False))
    got, count = rt.render_budget(ctx, scene, cam, rd, SEED, budget, garbage, np.zeros((H, W), np.uint32))
    assert_frame(got, want, (name, shape))
    assert count.tobytes() == want_count.tobytes()
    got, count = rt.render_budget(ctx, scene, cam, rd, SEED2, budget, got, count)
    assert_frame(got, want2, (name, shape, "fold"))
    assert count.tobytes() == want_count2.tobytes()
    del torch


def test_invalid_arguments_leave_the_outputs_untouched(rt, ctx, models_dir):
    L = rt.lib()
    objs, sky = scene_of(rt, "three_sphere")
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objs, models_dir))
    cam, rd = rt.Camera(W, H), rt.RenderData(4, LIMIT, True, sky)
    budget = np.full((H, W), 2, np.uint16)
    count = np.full((H, W), 0x1234, np.uint32)
    frame = np.full((H, W, 3), GARBAGE, F)
    pb, pc, pf = C.c_void_p(budget.ctypes.data), count.ctypes.data_as(C.POINTER(C.c_uint32)), frame.ctypes.data_as(C.POINTER(C.c_float))
    ids = (C.c_uint32 * 4)(0, 1, 2, 2)
    good = (ctx._h, scene._h, C.byref(cam.c), C.byref(rd.c), 0, None, pb, pc, pf)

    def with_(i, v):
        return good[:i] + (v,) + good[i + 1:]

    def spec(**kw):
        ts = rt.rt_tile_spec(8, 0, 1, 0)
        ts.tile_list, ts.num_tiles = C.cast(ids, C.POINTER(C.c_uint32)), 3
        for k, v in kw.items():
            setattr(ts, k, v)
        return C.byref(ts)

    neg = rt.RenderData(4, -1, True, sky)
    bad = [(with_(1, None), "null"), (with_(2, None), "null"), (with_(3, None), "null"), (with_(6, None), "null"), (with_(8, None), "null"),
           (with_(1, foreign._h), "another context"), (with_(3, C.byref(neg.c)), "render settings"),
           (with_(5, C.byref(rt.rt_tile_spec(8, 0, 1, 0))), "not bands"), (with_(5, spec(compact=1)), "compact"),
           (with_(5, spec(tile_cost=C.cast(ids, C.POINTER(C.c_uint32)))), "tile_cost"), (with_(5, spec(num_tiles=16)), "num_tiles"),
           (with_(5, spec(num_tiles=4)), "listed twice")]
    for args, msg in bad:
        assert L.rt_render_budget(*args) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        assert np.all(count == 0x1234) and np.all(frame == GARBAGE), msg
    p = rt.AdaptiveParams()
    st = rt.rt_adaptive_stats()
    for field, value in (("pilot_spp", 0), ("step_spp", 65536), ("max_spp", p.c.pilot_spp - 1), ("max_passes", 65), ("threshold", float("inf")),
                         ("pixel_threshold", 0.0), ("floor", float("nan"))):
        q = rt.AdaptiveParams(**{field: value})
        assert L.rt_render_adaptive_host(ctx._h, scene._h, C.byref(cam.c), C.byref(rd.c), 0, C.byref(q.c), pf, pc, C.byref(st)) == rt.RT_ERR_INVALID, field
        assert "adaptive parameters" in ctx.last_error() and field in ctx.last_error(), (field, ctx.last_error())
        assert np.all(count == 0x1234) and np.all(frame == GARBAGE) and st.passes == 0
    # the context is as usable as before
    assert L.rt_render_budget(*good) == rt.RT_OK, ctx.last_error()
    assert np.all(count == 0x1234 + 2) and not np.any(frame == GARBAGE)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
PLAN = dict(step_spp=3, max_spp=11, threshold=0.25, pixel_threshold=np.inf, floor=0.01)


def plan_inputs(rt, orc, models_dir, w, h):
    """A / B: two oracle frames of the three-sphere scene at 2 spp, with a NaN and two infinite pixels where the image has room; counts on
    both sides of max_spp"""
    key = ("plan", w, h)
    if key not in _CACHE:
        oracle, sky = oracle_of(rt, orc, models_dir, "three_sphere")
        cam = rt.Camera(w, h).floats()
        A = oracle.render(cam, w, h, 2, LIMIT, sky, time_ms=1)
        B = oracle.render(cam, w, h, 2, LIMIT, sky, time_ms=2)
        count = np.random.default_rng(w * 1000 + h).choice(np.array([2, 5, 9, 10, 11, 12, 400], np.uint32), size=(h, w))
        if w * h >= 64:
            A[h // 2, w // 2, 1] = np.nan
            A[1, 2] = np.inf                                        # A - B = inf, I = inf: e = inf / inf = NaN -> 0
            B[h - 1, w - 1, 0] = -np.inf                            # num = inf, s = -inf -> floor: e = +inf, and so is the tile's E
        _CACHE[key] = (A, B, count)
    return _CACHE[key]


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (37, 21), (64, 40)])
@pytest.mark.parametrize("pixel_threshold", [np.inf, 0.7])
def test_plan_equals_the_yardstick(rt, orc, ctx, models_dir, w, h, pixel_threshold):
    import torch
    A, B, count = plan_inputs(rt, orc, models_dir, w, h)
    p = dict(PLAN, pixel_threshold=pixel_threshold)
    budget, E, active, e = R.plan(A, B, count, **p)
    if w * h >= 64:
        # conditions on the inputs, from the yardstick alone: both rules decide somewhere, and the special values are where they were put
        assert np.isinf(E[-1]) and e[1, 2] == 0 and e[h // 2, w // 2] == 0
        assert (budget == 0).any() and (budget == 3).any() and ((budget > 0) & (budget < 3)).any()
        assert 0 < np.count_nonzero(active) and (w * h == 64 or np.count_nonzero(active) < len(active))
        if np.isfinite(pixel_threshold) and len(E) > 1:
            assert not np.array_equal(budget, R.plan(A, B, count, **PLAN)[0])
    n_tiles = len(E)
    dev = torch.device("cuda:0")
    t_a, t_b = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    t_count = torch.from_numpy(count.view(np.int32)).to(dev)
    t_budget = torch.full((h, w), 0x7777, dtype=torch.int16, device=dev)
    t_err = torch.full((n_tiles,), 7.0, dtype=torch.float32, device=dev)
    t_act = torch.full((n_tiles,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rt.adaptive_plan_device(ctx, w, h, t_a.data_ptr(), t_b.data_ptr(), t_count.data_ptr(), t_budget.data_ptr(), t_err.data_ptr(), t_act.data_ptr(),
                            rt.AdaptiveParams(pilot_spp=2, max_passes=4, **p))
    ctx.synchronize()
    assert t_budget.cpu().numpy().view(np.uint16).tobytes() == budget.tobytes(), int((t_budget.cpu().numpy().view(np.uint16) != budget).sum())
    assert np.array_equal(u32(t_err.cpu().numpy()), u32(E))
    assert t_act.cpu().numpy().view(np.uint32).tobytes() == active.tobytes()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
DW, DH = 40, 24
DRIVER = dict(pilot_spp=2, step_spp=3, max_spp=11, max_passes=4, threshold=0.15)


def ref_driver(rt, orc, models_dir, name, params):
    key = ("driver", name, tuple(sorted(params.items())))
    if key not in _CACHE:
        oracle, sky = oracle_of(rt, orc, models_dir, name)
        _CACHE[key] = R.render_adaptive(oracle, rt.Camera(DW, DH).floats(), DW, DH, LIMIT, sky, SEED, params)[:3]
    return _CACHE[key]


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey"])
def test_driver_equals_the_yardstick_loop(rt, orc, ctx, models_dir, name):
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cam, rd = rt.Camera(DW, DH), rt.RenderData(999, LIMIT, True, sky)
    want, want_count, want_stats = ref_driver(rt, orc, models_dir, name, DRIVER)
    print(name, want_stats)
    # conditions on the inputs, from the yardstick alone: passes were rendered, some tiles stopped at the pilot and some pixels reached
    # max_spp (2, 5, 8, 11: three passes; the fourth plan finds nothing left); on two of the scenes tiles drop out between passes
    assert want_stats["passes"] == 3 and want_stats["active_tiles"][0] < 15 and want_count.min() == 4 and want_count.max() == 22
    assert name == "monkey" or (want_stats["active_tiles"][-1] < want_stats["active_tiles"][0] and len(np.unique(want_count)) == 4)
    got, count, stats = rt.render_adaptive(ctx, scene, cam, rd, SEED, rt.AdaptiveParams(**DRIVER))
    assert stats == want_stats, (stats, want_stats)
    assert count.tobytes() == want_count.tobytes() and stats["total_samples"] == int(count.sum())
    assert_frame(got, want, name)
    # twice: identical bytes
    again, count2, stats2 = rt.render_adaptive(ctx, scene, cam, rd, SEED, rt.AdaptiveParams(**DRIVER))
    assert again.tobytes() == got.tobytes() and count2.tobytes() == count.tobytes() and stats2 == stats
    # max_passes 0: the pilot only
    want0, want_count0, want_stats0 = ref_driver(rt, orc, models_dir, name, dict(DRIVER, max_passes=0))
    got0, count0, stats0 = rt.render_adaptive(ctx, scene, cam, rd, SEED, rt.AdaptiveParams(**dict(DRIVER, max_passes=0)))
    assert stats0 == want_stats0 == {"passes": 0, "active_tiles": [], "total_samples": 4 * DW * DH}
    assert_frame(got0, want0, (name, "pilot only"))
    assert np.all(count0 == 4) and count0.tobytes() == want_count0.tobytes()


def test_driver_with_the_pixel_rule_and_device_outputs(rt, orc, ctx, models_dir):
    """a finite pixel_threshold, the device-buffer form, no count plane, no stats"""
    import torch
    name = "cube"
    objs, sky = scene_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cam, rd = rt.Camera(DW, DH), rt.RenderData(999, LIMIT, True, sky)
    params = dict(DRIVER, threshold=0.6, pixel_threshold=1.0)
    want, want_count, want_stats = ref_driver(rt, orc, models_dir, name, params)
    # (the pixel rule decided somewhere: a tile whose pixels did not all get the same number of samples)
    assert want_stats["passes"] >= 1 and any(len(set(t[t > 0])) > 1 for t in R.tiles_of(want_count, 0))
    t_frame = torch.full((DH, DW, 3), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p = rt.AdaptiveParams(**params)
    ctx._check(rt.lib().rt_render_adaptive(ctx._h, scene._h, C.byref(cam.c), C.byref(rd.c), SEED, C.byref(p.c), C.c_void_p(t_frame.data_ptr()), None, None, None))
    assert_frame(t_frame.cpu().numpy(), want, "device form")
    got, count, stats = rt.render_adaptive(ctx, scene, cam, rd, SEED, p)
    assert stats == want_stats and count.tobytes() == want_count.tobytes()


def test_the_cpp_example_runs_end_to_end(rt, models_dir, tmp_path):
    """host/example_adaptive.cpp (Renderer::render_adaptive, Renderer::render_budget of host/raytracer.hpp), like the other C++ mirror tests: it checks
    a uniform budget against Renderer::render itself, runs the loop and writes the frame and the sample map"""
    exe = rt.build.build_adaptive_example()
    r = subprocess.run([exe, models_dir, "72", "56", str(tmp_path / "adaptive")], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "adaptive ok" in r.stdout, r.stdout[-3000:]
    assert os.path.getsize(str(tmp_path / "adaptive.png")) > 1000 and os.path.getsize(str(tmp_path / "adaptive_samples.png")) > 100
