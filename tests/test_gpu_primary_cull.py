"""The primary-ray cull on the device (ray-tracer_amd/csrc/rt_cull.h): frames with the view's cull plane are, as uint32, the frames without it
(RT_AMD_PRIMARY_CULL=0) and the CPU oracle's, through every launch form that reads the plane; the plane follows the camera, the image size and
the scene's geometry; and what the pre-pass wrote is what the host evaluates with the same predicate.  Nothing has a tolerance.  The scenes run
on rt_traits_kernel with 1024 threads, the one kernel that reads the plane (rt_loop_culls): the monkey, and soups of triangles over a sphere.
The generic kernel has no form of the cull, so scenes that run it - reference scene 0, two meshes - are handed no plane;
that is all this file says about them.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from test_gpu_descend_pop import context_with, mismatches
from test_gpu_parity import eq
from test_gpu_shapes import commit_as

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, LIMIT = 96, 64, 8, 8
TIMES = [7001, 7002, 7003]
SKY = (0.8, 1.0, 1.0)
GREY = ("standard", (0.6, 0.6, 0.7), 0.1)
GROUND = ("sphere", (0, -100.5, 1.5), 100, ("standard", (0.5, 0.5, 0.5), 0.3))


def soup(seed, n, centre, spread=0.12):
    rng = np.random.default_rng(seed)
    return (np.array(centre) + rng.normal(0, spread, (n, 1, 3)) + rng.normal(0, 0.05, (n, 3, 3))).astype(F).reshape(n, 9)


def cases(rt):
    monkey = rt.scenes.monkey()
    return {
        "monkey": (monkey, rt.Camera(W, H), True),
        "monkey, antialias off": (monkey, rt.Camera(W, H), False),
        "camera inside the mesh's root box": (monkey, rt.Camera(W, H, pos=(0.1, -0.1, 1.6)), True),
        "camera looking away": (monkey, rt.Camera(W, H, rot=(0.0, float(np.pi), 0.0)), True),
        "a soup of triangles": (([("mesh", soup(3, 300, (0.2, 0.1, 1.4)), GREY), GROUND], SKY), rt.Camera(W, H), True),
    }


CASE_NAMES = ["monkey", "monkey, antialias off", "camera inside the mesh's root box", "camera looking away", "a soup of triangles"]


def zeros():
    import torch
    return torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def every_form(rt, ctx, scene, cam, rd):
    """the three progressive frames through render_device_batch, through one launch per frame with d_prev, and frame 0 through a tile list"""
    batch = zeros()
    rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, batch.data_ptr())
    used_batch = rt.primary_cull_plane(ctx)[0]
    a, b = zeros(), zeros()
    for i, t in enumerate(TIMES):
        rt.render_device(ctx, scene, cam, rd, t, i, b.data_ptr(), d_prev=a.data_ptr())
        a, b = b, a
    tiles = np.arange(((W + 7) // 8) * ((H + 7) // 8), dtype=np.uint32)[::-1].copy()
    listed = zeros()
    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, listed.data_ptr(), tile_list=tiles)
    used_list = rt.primary_cull_plane(ctx)[0]
    return {"batch": host(batch), "per frame": host(a), "tile list": host(listed)}, used_batch and used_list


@pytest.mark.parametrize("name", CASE_NAMES)
def test_frames_are_bit_identical_with_and_without_the_plane(rt, orc, models_dir, monkeypatch, name):
    (objs, sky), cam, antialias = cases(rt)[name]
    rd = rt.RenderData(SPP, LIMIT, antialias, sky)
    o = orc.Scene(objs, orc.MATH_DET, models_dir)
    want, prev = [], None
    for i, t in enumerate(TIMES):
        prev = o.render(cam.floats(), W, H, SPP, LIMIT, sky, time_ms=t, frame_num=i, antialias=antialias, prev=prev)
        want.append(prev)
    got = {}
    for switch in ("1", "0"):
        ctx = context_with(rt, monkeypatch, {"RT_AMD_PRIMARY_CULL": switch})
        scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": "1024"})
        info = scene.info()
        assert info["threads_per_block"] == 1024 and info["scene_in_lds"] == 1, info
        assert info["kernel_variant"] == "traits", info
        got[switch], used = every_form(rt, ctx, scene, cam, rd)
        assert used == (switch == "1"), (name, switch)
        if switch == "1" and name == "camera looking away":
            _, pw, ph, words = rt.primary_cull_plane(ctx)
            assert (pw, ph) == (W, H) and rt.cull.plane_bits(words, W, H).all(), "a camera that looks away from the mesh flags every pixel"
    for form, frame in got["1"].items():
        ref = want[0] if form == "tile list" else want[2]
        assert eq(frame, got["0"][form]), (name, form, "plane on against off", mismatches(frame, got["0"][form]))
        assert eq(frame, ref), (name, form, "against the oracle", mismatches(frame, ref))


@pytest.mark.parametrize("name", ["reference scene 0", "two meshes"])
def test_a_scene_on_the_generic_kernel_is_handed_no_plane(rt, models_dir, monkeypatch, name):
    """rt_render_kernel does not read the plane, so no pre-pass runs for its scenes and rt_debug_primary_cull reports none"""
    objs, sky = rt.scenes.reference_scene0() if name == "reference scene 0" else (
        [("mesh", soup(3, 300, (0.0, 0.0, 1.4)), GREY), ("mesh", soup(4, 500, (0.05, 0.05, 2.6), 0.3), GREY), GROUND], SKY)
    ctx = context_with(rt, monkeypatch, {})
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": "1024"})
    assert scene.info()["kernel_variant"] == "generic" and scene.info()["threads_per_block"] == 1024
    data = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, rt.Camera(W, H), rt.RenderData(1, 2, True, sky), data, 1)
    assert rt.primary_cull_plane(ctx) == (False, 0, 0, None)


def render_one(rt, ctx, scene, cam, sky, w, h, time_ms=9001):
    data = rt.VariableRenderData(w, h)
    rt.render(ctx, scene, cam, rt.RenderData(SPP, LIMIT, True, sky), data, time_ms)
    return data.previous_render.copy()


def plane_of(rt, ctx, w, h):
    used, pw, ph, words = rt.primary_cull_plane(ctx)
    assert used and (pw, ph) == (w, h)
    return words


def test_the_plane_follows_the_camera_and_the_image_size(rt, models_dir, monkeypatch):
    objs, sky = rt.scenes.monkey()
    ctx = context_with(rt, monkeypatch, {})
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    cam_a, cam_b = rt.Camera(W, H), rt.Camera(W, H, pos=(0.6, 0.2, 0.3))
    render_one(rt, ctx, scene, cam_a, sky, W, H)
    words_a = plane_of(rt, ctx, W, H)
    moved = render_one(rt, ctx, scene, cam_b, sky, W, H)
    words_b = plane_of(rt, ctx, W, H)
    assert not np.array_equal(words_a, words_b), "the camera moved: the plane must have been computed again"
    larger = render_one(rt, ctx, scene, rt.Camera(2 * W, 2 * H), sky, 2 * W, 2 * H)
    words_c = plane_of(rt, ctx, 2 * W, 2 * H)
    again = render_one(rt, ctx, scene, cam_a, sky, W, H)        # back to the first view: the larger allocation is kept, the plane is the first one's
    assert np.array_equal(plane_of(rt, ctx, W, H), words_a)
    fresh = context_with(rt, monkeypatch, {})
    fscene = fresh.commit(rt.SceneObjects(objs, models_dir))
    assert eq(moved, render_one(rt, fresh, fscene, cam_b, sky, W, H))
    fresh2 = context_with(rt, monkeypatch, {})
    fscene2 = fresh2.commit(rt.SceneObjects(objs, models_dir))
    assert eq(larger, render_one(rt, fresh2, fscene2, rt.Camera(2 * W, 2 * H), sky, 2 * W, 2 * H))
    assert np.array_equal(plane_of(rt, fresh2, 2 * W, 2 * H), words_c)
    off = context_with(rt, monkeypatch, {"RT_AMD_PRIMARY_CULL": "0"})
    oscene = off.commit(rt.SceneObjects(objs, models_dir))
    assert eq(again, render_one(rt, off, oscene, cam_a, sky, W, H))


def test_a_mesh_update_moves_the_mesh_into_flagged_pixels(rt, models_dir, monkeypatch):
    """the mesh starts at the left of the image and is moved to the right on the device: pixels the first plane flags see it afterwards"""
    import torch
    left, right = soup(11, 400, (-0.45, 0.0, 1.6)), soup(11, 400, (0.45, 0.0, 1.6))
    cam = rt.Camera(W, H)
    ctx = context_with(rt, monkeypatch, {})
    scene = commit_as(rt, ctx, monkeypatch, [("mesh", left, GREY), GROUND], models_dir, {"RT_AMD_THREADS": "1024"})
    assert scene.info()["threads_per_block"] == 1024
    render_one(rt, ctx, scene, cam, SKY, W, H)
    before = rt.cull.plane_bits(plane_of(rt, ctx, W, H), W, H)
    scene.update_mesh_device(0, torch.from_numpy(right).to("cuda:0"))
    got = render_one(rt, ctx, scene, cam, SKY, W, H)
    after = rt.cull.plane_bits(plane_of(rt, ctx, W, H), W, H)
    assert ((before == 1) & (after == 0)).sum() > 100 and ((before == 0) & (after == 1)).sum() > 100, "the plane did not follow the mesh"
    fresh = context_with(rt, monkeypatch, {})
    fscene = commit_as(rt, fresh, monkeypatch, [("mesh", right, GREY), GROUND], models_dir, {"RT_AMD_THREADS": "1024"})
    want = render_one(rt, fresh, fscene, cam, SKY, W, H)
    assert eq(got, want), mismatches(got, want)
    assert np.array_equal(after, rt.cull.plane_bits(plane_of(rt, fresh, W, H), W, H))


@pytest.mark.parametrize("name", ["monkey", "camera inside the mesh's root box", "camera looking away"])
@pytest.mark.parametrize("antialias", [True, False], ids=["antialias", "no antialias"])
def test_the_device_plane_is_the_host_predicate(rt, models_dir, monkeypatch, name, antialias):
    """a ragged image (no multiple of 8, 32 or 64 pixels): the pre-pass's words against rt_debug_primary_cull_host on the scene as it is on the device"""
    (objs, sky), cam96, _ = cases(rt)[name]
    w, h = 101, 67
    f = cam96.floats()
    cam = rt.Camera(w, h, floats=f)
    ctx = context_with(rt, monkeypatch, {})
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": "1024"})
    data = rt.VariableRenderData(w, h)
    rt.render(ctx, scene, cam, rt.RenderData(1, 1, antialias, sky), data, 1)
    words = plane_of(rt, ctx, w, h)
    host_words, stats = rt.primary_cull_host(scene, cam, antialias)
    assert words.size == host_words.size == stats["words"] and np.array_equal(words, host_words), int((words != host_words).sum())
    assert int(rt.cull.plane_bits(words, w, h).sum()) == stats["flagged"]
