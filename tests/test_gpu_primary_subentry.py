"""The sub-entry words on the device (ray-tracer_amd/csrc/rt_entry.h, "The sub-entry words"; px_gen and the mesh start of rt_render_loop.inc): a
primary ray of a pixel with a table starts on the one-triangle leaf of its sub-box's word, or does not enter the mesh where the word is `nothing`.
A wrong word changes a pixel silently, so every frame here is compared as uint32 across five renderings - sub-entries on with the refinement at
once (RT_AMD_SUBENTRY_SAMPLES=0), RT_AMD_PRIMARY_SUBENTRY=0 (no table: every table pixel's word stays 0), RT_AMD_PRIMARY_ENTRY=0, the generic
kernel and the CPU oracle (MATH_DET) -, through launch forms that read the plane and across the plane's lifetimes, and the tables the
refinement wrote are the host function's, pixel by pixel.  Nothing has a tolerance.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from test_gpu_descend_pop import context_with, mismatches
from test_gpu_primary_cull import eq
from test_gpu_primary_cull_views import BAND, GARBAGE, band_rows_owned, buffer, generic_scene, host, random_tile_list, tile_mask, traits_scene
from test_gpu_primary_entry import NOTHING, SPP, TIMES, objects, one_frame, oracle
from test_subtree_cull import INSIDE

pytestmark = pytest.mark.gpu

SWITCHES = {"sub": {"RT_AMD_SUBENTRY_SAMPLES": "0"}, "sub off": {"RT_AMD_PRIMARY_SUBENTRY": "0", "RT_AMD_SUBENTRY_SAMPLES": "0"},
            "entries off": {"RT_AMD_PRIMARY_ENTRY": "0", "RT_AMD_SUBENTRY_SAMPLES": "0"}, "deferred": {"RT_AMD_SUBENTRY_SAMPLES": "1000000"}}
_CTX, _SCENE = {}, {}


def ctx_of(rt, monkeypatch, switch):
    if switch not in _CTX:
        _CTX[switch] = context_with(rt, monkeypatch, SWITCHES[switch])
    return _CTX[switch]


def scene_of(rt, monkeypatch, models_dir, name, kind):
    if (name, kind) not in _SCENE:
        objs, _ = objects(rt, name)
        ctx = ctx_of(rt, monkeypatch, "sub" if kind == "generic" else kind)
        _SCENE[(name, kind)] = (ctx, (generic_scene if kind == "generic" else traits_scene)(rt, ctx, monkeypatch, objs, models_dir))
    return _SCENE[(name, kind)]


def device_tables(rt, ctx, scene, cam):
    """the tables the context's last launch was handed, asserted to be the host function's for `cam`, with at least one non-zero sub-word, and
    the table pixels' own words 0"""
    refined, pixels, words = rt.primary_subentry_tables(ctx)
    assert refined, "the launch was handed no refined plane"
    # (where more pixels want a table than the image's allocation holds the device hands its slots to whichever come first: any `cap` of them)
    hp, hw, st = rt.primary_subentry_host(scene, cam, True, cap=1 << 30)
    assert pixels.size == min(st["pixels_wanting_table"], 4 * rt.cull.plane_words(cam.c.width, cam.c.height)) and (np.diff(pixels.astype(np.int64)) > 0).all()
    at = np.searchsorted(hp, pixels)
    assert (at < hp.size).all() and np.array_equal(hp[np.minimum(at, hp.size - 1)], pixels), "the device gave a table to a pixel that wants none"
    assert np.array_equal(words, hw[at]), "%d sub-words of the device differ from the host's" % int((words != hw[at]).sum())
    assert (words != 0).any(), "no table pixel has a non-zero sub-word: the case decides nothing"
    used, own = rt.primary_entry_words(ctx)
    assert used and not own.reshape(-1)[pixels].any()
    return pixels, words


def camera_of(rt, which, w=96, h=64):
    if which == "inside the root box":
        return rt.Camera(w, h, pos=INSIDE)
    if which == "narrow field of view":
        return rt.Camera(w, h, fov=0.035)
    return rt.Camera(w, h)


def five_way(rt, orc, monkeypatch, models_dir, name, cam, limit):
    objs, sky = objects(rt, name)
    rd = rt.RenderData(SPP, limit, True, sky)
    got = {}
    for kind in ("sub off", "entries off", "generic", "sub"):
        ctx, scene = scene_of(rt, monkeypatch, models_dir, name, kind)
        got[kind] = one_frame(rt, ctx, scene, cam, rd)
        if kind == "sub off":
            assert not rt.primary_subentry_tables(ctx)[0], "RT_AMD_PRIMARY_SUBENTRY=0 refines nothing"
            used, own = rt.primary_entry_words(ctx)
            want, _ = rt.primary_entry_host(scene, cam, True)
            assert used and np.array_equal(own, want), "RT_AMD_PRIMARY_SUBENTRY=0 leaves every table pixel's word 0 and the others as they were"
    got["oracle"] = oracle(orc, models_dir, rt, name, cam, limit, True)
    for kind in ("sub off", "entries off", "generic", "oracle"):
        assert eq(got["sub"], got[kind]), (name, limit, "sub-entries on against " + kind, mismatches(got["sub"], got[kind]))
    ctx, scene = scene_of(rt, monkeypatch, models_dir, name, "sub")
    return device_tables(rt, ctx, scene, cam)


@pytest.mark.parametrize("limit", [8, 1])
@pytest.mark.parametrize("size", [(96, 64), (100, 67)], ids=lambda s: "%dx%d" % s)
def test_five_renderings_agree_on_the_monkey(rt, orc, models_dir, monkeypatch, size, limit):
    _pixels, words = five_way(rt, orc, monkeypatch, models_dir, "monkey", rt.Camera(*size), limit)
    assert (words & 1).any() and (words == NOTHING).any()


@pytest.mark.parametrize("which", ["narrow field of view", "inside the root box"])
def test_five_renderings_agree_from_other_cameras(rt, orc, models_dir, monkeypatch, which):
    """a two-degree field of view: cones span pixels, the tables are dense (and full); a camera inside the root box"""
    five_way(rt, orc, monkeypatch, models_dir, "monkey", camera_of(rt, which), 8)


@pytest.mark.parametrize("name", ["12 triangles", "mesh first", "mesh last", "mesh emissive"])
def test_five_renderings_agree_on_other_scenes(rt, orc, models_dir, monkeypatch, name):
    """a 12-triangle mesh; the mesh first, last and emissive in the object list, with a sphere in front"""
    five_way(rt, orc, monkeypatch, models_dir, name, rt.Camera(96, 64), 8)


def test_the_device_tables_are_the_host_functions(rt, models_dir, monkeypatch):
    """a ragged image (no multiple of 8, 32 or 64 pixels), pixel by pixel"""
    objs, sky = objects(rt, "monkey")
    ctx, scene = scene_of(rt, monkeypatch, models_dir, "monkey", "sub")
    cam = rt.Camera(100, 67)
    one_frame(rt, ctx, scene, cam, rt.RenderData(SPP, 8, True, sky))
    pixels, _words = device_tables(rt, ctx, scene, cam)
    assert pixels.size > 100


def test_batch_and_per_frame_launches_agree(rt, orc, models_dir, monkeypatch):
    """three progressive frames in one launch and one launch per frame, against the oracle's progressive loop"""
    objs, sky = objects(rt, "monkey")
    ctx, scene = scene_of(rt, monkeypatch, models_dir, "monkey", "sub")
    cam, rd = rt.Camera(96, 64), rt.RenderData(SPP, 8, True, sky)
    want = oracle(orc, models_dir, rt, "monkey", cam, 8, True, frames=3)
    batch = buffer(96, 64, GARBAGE)
    rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, batch.data_ptr())
    device_tables(rt, ctx, scene, cam)
    prev, out = None, None
    for i, t in enumerate(TIMES):
        out = buffer(96, 64, GARBAGE)
        rt.render_device(ctx, scene, cam, rd, t, i, out.data_ptr(), None if prev is None else prev.data_ptr())
        prev = out
    assert eq(host(batch), want) and eq(host(out), want)


def test_bands_compact_bands_and_a_shuffled_tile_list(rt, orc, models_dir, monkeypatch):
    """the launch forms that render part of the image: the rows or tiles they own are the full frame's"""
    objs, sky = objects(rt, "monkey")
    ctx, scene = scene_of(rt, monkeypatch, models_dir, "monkey", "sub")
    w, h = 100, 67
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, 8, True, sky)
    want = oracle(orc, models_dir, rt, "monkey", cam, 8, True)
    rows = band_rows_owned(h)
    out = buffer(w, h, GARBAGE)
    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, out.data_ptr(), **BAND)
    device_tables(rt, ctx, scene, cam)
    assert eq(host(out)[rows], want[rows])
    out = buffer(w, len(rows), GARBAGE)
    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, out.data_ptr(), compact=True, **BAND)
    assert eq(host(out), want[rows])
    tiles = random_tile_list(w, h)
    out = buffer(w, h, GARBAGE)
    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, out.data_ptr(), tile_list=tiles)
    mask = tile_mask(w, h, tiles)
    assert eq(host(out)[mask], want[mask])


def test_the_deferred_policy_refines_on_the_first_reuse(rt, orc, models_dir, monkeypatch):
    """a launch below the threshold is handed the plane as the pre-pass wrote it; the second launch of the view refines (seen through the device
    hook), the third does not again; all three frames are the oracle's"""
    objs, sky = objects(rt, "monkey")
    ctx, scene = scene_of(rt, monkeypatch, models_dir, "monkey", "deferred")
    cam, rd = rt.Camera(96, 64), rt.RenderData(SPP, 8, True, sky)
    want = oracle(orc, models_dir, rt, "monkey", cam, 8, True)
    first = one_frame(rt, ctx, scene, cam, rd)
    assert rt.primary_cull_plane(ctx)[0] and not rt.primary_subentry_tables(ctx)[0], "the first launch below the threshold refined"
    second = one_frame(rt, ctx, scene, cam, rd)
    device_tables(rt, ctx, scene, cam)
    third = one_frame(rt, ctx, scene, cam, rd)
    device_tables(rt, ctx, scene, cam)
    assert eq(first, want) and eq(second, want) and eq(third, want)


def test_a_camera_move_and_back_and_a_larger_image(rt, orc, models_dir, monkeypatch):
    """the plane's lifetimes: every view is computed and refined again, in the allocation that grew with the image"""
    objs, sky = objects(rt, "monkey")
    ctx, scene = scene_of(rt, monkeypatch, models_dir, "monkey", "sub")
    rd = rt.RenderData(SPP, 8, True, sky)
    a, b, big = rt.Camera(96, 64), rt.Camera(96, 64, pos=INSIDE), rt.Camera(160, 104)
    for cam in (a, b, a, big, a):
        got = one_frame(rt, ctx, scene, cam, rd)
        device_tables(rt, ctx, scene, cam)
        want = oracle(orc, models_dir, rt, "monkey", cam, 8, True)
        assert eq(got, want), mismatches(got, want)


def test_two_scenes_alternate(rt, orc, models_dir, monkeypatch):
    """two scenes on one context: each launch finds the other scene's plane, computes its own and refines it"""
    ctx = ctx_of(rt, monkeypatch, "sub")
    cam = rt.Camera(96, 64)
    for name in ("monkey", "12 triangles", "monkey", "12 triangles"):
        _objs, sky = objects(rt, name)
        _ctx, scene = scene_of(rt, monkeypatch, models_dir, name, "sub")
        got = one_frame(rt, ctx, scene, cam, rt.RenderData(SPP, 8, True, sky))
        device_tables(rt, ctx, scene, cam)
        assert eq(got, oracle(orc, models_dir, rt, name, cam, 8, True)), name


def test_two_contexts_share_a_frame(rt, orc, models_dir, monkeypatch):
    """rt_render_multi_device: two contexts render bands of one frame, each with a plane and tables of its own; three progressive frames in two
    calls against the oracle's progressive loop"""
    from test_gpu_primary_cull_views import stream_of
    w, h = 100, 67
    objs, sky = objects(rt, "monkey")
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, 8, True, sky)
    want = oracle(orc, models_dir, rt, "monkey", cam, 8, True, frames=3)
    ctxs = [context_with(rt, monkeypatch, SWITCHES["sub"]) for _ in range(2)]
    scenes = [traits_scene(rt, c, monkeypatch, objs, models_dir) for c in ctxs]
    frame = buffer(w, h, GARBAGE)
    rt.render_multi_device(ctxs, scenes, cam, rd, TIMES[:1], 0, frame.data_ptr(), band_rows=8, stream=stream_of())
    rt.render_multi_device(ctxs, scenes, cam, rd, TIMES[1:], 1, frame.data_ptr(), band_rows=8, stream=stream_of())
    for c in ctxs:
        c.synchronize()
    got = host(frame)
    for c, s in zip(ctxs, scenes):
        device_tables(rt, c, s, cam)
    assert eq(got, want), mismatches(got, want)


@pytest.mark.parametrize("policy", ["sub", "deferred"])
def test_pipelined_frames(rt, orc, models_dir, monkeypatch, policy):
    """three frames in flight (rt_frame_submit).  "sub": the first frame refines at once.  "deferred": the first frame is below the threshold
    and is handed the plane as the pre-pass wrote it; the second, submitted while the first is in flight, reuses the plane and queues the
    refinement, which rewrites entry words the first frame's kernel may be reading - the host waits for the frames in flight first; the
    third finds the view refined.  The folded frames are the oracle's progressive loop's"""
    from test_gpu_primary_cull_views import stream_of
    w, h = 100, 67
    objs, sky = objects(rt, "monkey")
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, 8, True, sky)
    want = oracle(orc, models_dir, rt, "monkey", cam, 8, True, frames=3)
    ctx = context_with(rt, monkeypatch, SWITCHES[policy])
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    rt.frame_depth(ctx, 3)
    out = buffer(w, h, GARBAGE)
    for t in TIMES:
        rt.frame_submit(ctx, scene, cam, rd, t)
    assert rt.frames_pending(ctx) == 3
    for i in range(len(TIMES)):
        rt.frame_collect(ctx, i, out.data_ptr(), stream=stream_of())
    rt.frame_wait(ctx)
    got = host(out)
    device_tables(rt, ctx, scene, cam)
    assert eq(got, want), mismatches(got, want)


def test_pipelined_reuse_refines_behind_a_frame_in_flight(rt, orc, models_dir, monkeypatch):
    """the deferred policy one submit at a time, seen through the device hook: after the first submit (below the threshold) the plane is not
    refined; after the second, with the first still uncollected, it is"""
    w, h = 96, 64
    objs, sky = objects(rt, "monkey")
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, 8, True, sky)
    ctx = context_with(rt, monkeypatch, SWITCHES["deferred"])
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    rt.frame_depth(ctx, 2)
    rt.frame_submit(ctx, scene, cam, rd, TIMES[0])
    assert rt.primary_cull_plane(ctx)[0] and not rt.primary_subentry_tables(ctx)[0], "the first frame, below the threshold, refined"
    rt.frame_submit(ctx, scene, cam, rd, TIMES[1])
    assert rt.frames_pending(ctx) == 2
    device_tables(rt, ctx, scene, cam)
    data = rt.VariableRenderData(w, h)
    rt.frame_collect_host(ctx, data)
    rt.frame_collect_host(ctx, data)
    want = oracle(orc, models_dir, rt, "monkey", cam, 8, True, frames=2)
    assert eq(data.previous_render, want), mismatches(data.previous_render, want)


def test_both_forms_of_a_mesh_update(rt, orc, models_dir, monkeypatch):
    """update_mesh_device on one stream, then a launch on another; then the host form: the scene's revision drops the slot words and the tables,
    each view is computed and refined again, the tables follow the mesh, and the frames are the oracle's of the mesh as it then is"""
    import torch
    from test_gpu_primary_cull import GREY, GROUND, SKY
    from test_subtree_cull import soup
    left, right = soup(11, 400, (-0.45, 0.0, 1.6)), soup(11, 400, (0.45, 0.0, 1.6))
    cam, rd = rt.Camera(96, 64), rt.RenderData(SPP, 8, True, SKY)

    def want(tris):
        return orc.Scene([("mesh", tris, GREY), GROUND], orc.MATH_DET, models_dir).render(cam.floats(), 96, 64, SPP, 8, SKY, time_ms=TIMES[0], frame_num=0, antialias=True, prev=None)
    ctx = context_with(rt, monkeypatch, SWITCHES["sub"])
    scene = traits_scene(rt, ctx, monkeypatch, [("mesh", left, GREY), GROUND], models_dir)
    got = one_frame(rt, ctx, scene, cam, rd)
    before, _ = device_tables(rt, ctx, scene, cam)
    assert eq(got, want(left)), mismatches(got, want(left))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    moved = torch.from_numpy(right).to("cuda:0")
    out = buffer(96, 64, GARBAGE)
    torch.cuda.synchronize()
    scene.update_mesh_device(0, moved, stream=s1.cuda_stream)
    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, out.data_ptr(), stream=s2.cuda_stream)
    got = host(out)
    after, _ = device_tables(rt, ctx, scene, cam)
    assert not np.array_equal(before, after), "the tables did not follow the mesh"
    assert eq(got, want(right)), mismatches(got, want(right))
    scene.update_mesh(0, left)
    got = one_frame(rt, ctx, scene, cam, rd)
    back, _ = device_tables(rt, ctx, scene, cam)
    assert np.array_equal(back, before)
    assert eq(got, want(left)), mismatches(got, want(left))
