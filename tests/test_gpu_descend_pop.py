"""rt_descend_pop (ray-tracer_amd/csrc/rt_traverse.h) on the device, where the in-loop pop has the most to do or the least room: a scene
whose descents mostly dead-end, waves with a single traversing lane, a stack that restarts between two meshes, and nodes / triangles read
from global memory - each against the oracle in det mode, bit for bit (uint32), across RT_AMD_DESCEND_KEEP where the exit rule matters.
tests/test_descend_pop_model.py holds the loop's control to today's per-lane order on the CPU; the whole GPU suite runs the same kernels."""
import os

import numpy as np
import pytest

from test_gpu_parity import _random_scene, eq
from test_gpu_shapes import commit_as

pytestmark = pytest.mark.gpu

_WANT = {}


def context_with(rt, monkeypatch, env):
    """a context created under `env` alone (the RT_AMD_* knobs are read there)"""
    with monkeypatch.context() as m:
        for k in [k for k in os.environ if k.startswith("RT_AMD_") and k not in ("RT_AMD_LIB", "RT_AMD_NO_TORCH")]:
            m.delenv(k)
        for k, v in env.items():
            m.setenv(k, v)
        return rt.Context(0)


def on_1024_threads(rt, ctx, monkeypatch, objs, models_dir):
    """the scene on the 1024-thread shape, the one that walks with rt_descend_pop (rt_descend_pops, rt_traverse.h), whatever its size would choose"""
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": "1024"})
    assert scene.info()["threads_per_block"] == 1024 and scene.info()["scene_in_lds"] == 1, scene.info()
    return scene


def keep_env(keep):
    return {} if keep is None else {"RT_AMD_DESCEND_KEEP": str(keep)}


def oracle_once(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def mismatches(got, want):
    return int((np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)).sum())


def unrotated_cube():
    """the scene of test_gpu_multi::test_flat_box_drop_quirk_on_the_device: flat leaf boxes nobody enters, so most descents end empty"""
    mat = ("standard", (0.8, 0.4, 0.2), 0)
    ground = ("sphere", (0, -100.5, 1.5), 100, ("standard", (0.5, 0.5, 0.5), 0))
    return [("obj", "cube.obj", [("enlarge", 0.3), ("rotate", 0.0, 0.0, 0.0), ("translate", 0, 0, 1.8)], mat), ground], (0.8, 1.0, 1.0)


@pytest.mark.parametrize("keep", [0, 1, None, 63, 64], ids=lambda k: "keep-default" if k is None else "keep-%d" % k)
def test_dead_ends_everywhere(rt, orc, models_dir, monkeypatch, keep):
    W, H, spp, limit = 64, 48, 4, 8
    objs, sky = unrotated_cube()
    want = oracle_once("cube", lambda: orc.Scene(objs, orc.MATH_DET, models_dir).render(rt.Camera(W, H).floats(), W, H, spp, limit, sky, time_ms=4242))
    ctx = context_with(rt, monkeypatch, keep_env(keep))
    scene = on_1024_threads(rt, ctx, monkeypatch, objs, models_dir)
    data = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, rt.Camera(W, H), rt.RenderData(spp, limit, True, sky), data, 4242)
    assert eq(data.previous_render, want), (keep, mismatches(data.previous_render, want))


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2)])
def test_one_traversing_lane_per_wave(rt, orc, ctx, models_dir, monkeypatch, W, H):
    """a pixel or six: a wave's traversing lanes are so few that n_keep is 0 and the loop runs until nobody travels"""
    objs, sky = rt.scenes.CONFIG_SCENES["monkey"]()
    spp, limit = 16, 8
    want = orc.Scene(objs, orc.MATH_DET, models_dir).render(rt.Camera(W, H).floats(), W, H, spp, limit, sky, time_ms=987654321)
    scene = on_1024_threads(rt, ctx, monkeypatch, objs, models_dir)
    data = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, rt.Camera(W, H), rt.RenderData(spp, limit, True, sky), data, 987654321)
    assert eq(data.previous_render, want), mismatches(data.previous_render, want)


def test_two_meshes_restart_the_stack(rt, orc, ctx, models_dir, monkeypatch):
    """seed 13 of test_gpu_parity._random_scene: a lane goes from one mesh to the next with sp back at 0; three progressive frames in one launch"""
    W, H, spp, limit, times = 64, 48, 4, 8, [987654321, 987654358, 987654395]
    objs, sky = _random_scene(13)
    assert sum(o[0] in ("mesh", "obj") for o in objs) >= 2, [o[0] for o in objs]
    oracle, prev = orc.Scene(objs, orc.MATH_DET, models_dir), None
    for i, t in enumerate(times):
        prev = oracle.render(rt.Camera(W, H).floats(), W, H, spp, limit, sky, time_ms=t, frame_num=i, prev=prev)
    scene = on_1024_threads(rt, ctx, monkeypatch, objs, models_dir)
    data = rt.VariableRenderData(W, H)
    assert ctx.max_batch_frames(W, H) >= len(times)
    rt.render_frames(ctx, scene, rt.Camera(W, H), rt.RenderData(spp, limit, True, sky), data, times)
    assert data.frame_num == len(times)
    assert eq(data.previous_render, prev), mismatches(data.previous_render, prev)


@pytest.mark.parametrize("keep", [0, 64])
@pytest.mark.parametrize("mode", ["hybrid", "global"])
def test_nodes_and_triangles_outside_lds(rt, orc, models_dir, monkeypatch, mode, keep):
    """soup6k: the triangles from global memory (hybrid), then the nodes too (RT_AMD_SCENE_MODE=0): the loop's node fetch and its read of
    the top of the stack then go to different memories, and LDS holds the stacks alone"""
    W, H, spp, limit = 48, 32, 2, 8
    objs, sky = rt.scenes.CONFIG_SCENES["soup6k"]()
    want = oracle_once("soup6k", lambda: orc.Scene(objs, orc.MATH_DET, models_dir).render(rt.Camera(W, H).floats(), W, H, spp, limit, sky, time_ms=12345))
    ctx = context_with(rt, monkeypatch, keep_env(keep))
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_SCENE_MODE": "0"} if mode == "global" else {})
    assert scene.info()["scene_in_lds"] == (0 if mode == "global" else 2) and scene.info()["threads_per_block"] == 1024, scene.info()
    data = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, rt.Camera(W, H), rt.RenderData(spp, limit, True, sky), data, 12345)
    assert eq(data.previous_render, want), (mode, keep, mismatches(data.previous_render, want))
