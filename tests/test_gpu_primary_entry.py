"""The primary entry words on the device (ray-tracer_amd/csrc/rt_entry.h; the mesh start of rt_render_loop.inc): a primary ray of a pixel whose
word is `triangle T` starts on the one-triangle leaf (T), one of a `nothing` pixel does not enter the mesh.  A wrong word changes a pixel
silently, so every frame here is compared as uint32 across five renderings - the entries on, RT_AMD_PRIMARY_ENTRY=0 (the same kernel, every
word 0), RT_AMD_PRIMARY_CULL=0 (no plane at all), the generic kernel (RT_AMD_KERNEL_VARIANT=generic at commit) and the CPU oracle (MATH_DET) -
through every launch form that reads the plane and across the plane's lifetimes, and the words the pre-pass wrote are the host function's, word
for word.  Nothing has a tolerance.  Scenes are committed with RT_AMD_THREADS=1024 and asserted to run rt_traits_kernel with the scene in LDS,
the one kernel that reads the plane.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from test_gpu_descend_pop import context_with, mismatches
from test_gpu_primary_cull import GREY, GROUND, SKY, eq
from test_gpu_primary_cull_views import (BAND, GARBAGE, LAMP, band_rows_owned, buffer, generic_scene, host, random_tile_list, stream_of, sweep_cameras, tile_mask,
                                         traits_scene, two_meshes)
from test_subtree_cull import INSIDE, soup

pytestmark = pytest.mark.gpu

F = np.float32
SPP = 4
TIMES = [7001, 7002, 7003]
NOTHING = 2
SWITCHES = {"entries": {}, "entries off": {"RT_AMD_PRIMARY_ENTRY": "0"}, "no plane": {"RT_AMD_PRIMARY_CULL": "0"}}
SETTINGS = [(8, True), (1, True), (8, False), (1, False)]                # (bounce limit, antialias)
FRONT = ("sphere", (0.2, 0.1, 1.0), 0.08, ("standard", (0.7, 0.4, 0.4), 0.2))         # in front of part of the soup: the merge with a nearer simple object


def placed(where):
    s = soup(3, 300, (0.2, 0.1, 1.4))
    return {"mesh first": [("mesh", s, GREY), FRONT, LAMP, GROUND], "mesh last": [FRONT, LAMP, GROUND, ("mesh", s, GREY)],
            "mesh emissive": [FRONT, ("mesh", s, ("emissive", (1.0, 0.8, 0.6), 3)), GROUND]}[where]


SCENES = ["monkey", "soup", "1 triangle", "3 triangles", "12 triangles"]
PLACES = ["mesh first", "mesh last", "mesh emissive"]
CAMERAS = ["inside the root box", "looking away", "narrow field of view"] + ["view %d" % i for i in range(8)]

_CTX, _SCENE, _WANT = {}, {}, {}


def objects(rt, name):
    if name == "monkey":
        return rt.scenes.monkey()
    if name in PLACES:
        return placed(name), SKY
    n = {"soup": 200, "1 triangle": 1, "3 triangles": 3, "12 triangles": 12}[name]
    return [("mesh", soup(3 if n == 200 else 20 + n, n), GREY), GROUND], SKY


def ctx_of(rt, monkeypatch, switch):
    if switch not in _CTX:
        _CTX[switch] = context_with(rt, monkeypatch, SWITCHES[switch])
    return _CTX[switch]


def scene_of(rt, monkeypatch, models_dir, name, kind):
    """(context, scene): `kind` one of SWITCHES on the traits kernel, or "generic" (on the context with the entries on: it is handed no plane)"""
    if (name, kind) not in _SCENE:
        objs, _ = objects(rt, name)
        ctx = ctx_of(rt, monkeypatch, "entries" if kind == "generic" else kind)
        _SCENE[(name, kind)] = (ctx, (generic_scene if kind == "generic" else traits_scene)(rt, ctx, monkeypatch, objs, models_dir))
    return _SCENE[(name, kind)]


def oracle(orc, models_dir, rt, name, cam, limit, antialias, frames=1):
    key = (name, tuple(cam.floats()), cam.c.width, cam.c.height, limit, antialias, frames)
    if key not in _WANT:
        objs, sky = objects(rt, name)
        o, prev = orc.Scene(objs, orc.MATH_DET, models_dir), None
        for i in range(frames):
            prev = o.render(cam.floats(), cam.c.width, cam.c.height, SPP, limit, sky, time_ms=TIMES[i], frame_num=i, antialias=antialias, prev=prev)
        _WANT[key] = prev
    return _WANT[key]


def one_frame(rt, ctx, scene, cam, rd):
    out = buffer(cam.c.width, cam.c.height, GARBAGE)
    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, out.data_ptr())
    return host(out)


def device_words(rt, ctx, scene, cam, antialias):
    """the entry words the context's last launch was handed, asserted to be the host function's for `cam` on the scene as it is on the device,
    0 in every flagged pixel and tagged wherever they are neither 0 nor `nothing`"""
    used, words = rt.primary_entry_words(ctx)
    assert used and words.shape == (cam.c.height, cam.c.width), (used, None if words is None else words.shape)
    want, _stats = rt.primary_entry_host(scene, cam, antialias)
    assert np.array_equal(words, want), "%d entry words of the device differ from the host's" % int((words != want).sum())
    bits = rt.cull.plane_bits(rt.primary_cull_plane(ctx)[3], cam.c.width, cam.c.height)
    assert not words[bits == 1].any(), "a flagged pixel has the entry word 0"
    other = words[(words != 0) & (words != NOTHING)]
    assert (other & 1).all()
    return words


def five_way(rt, orc, monkeypatch, models_dir, name, cam, limit, antialias):
    objs, sky = objects(rt, name)
    rd = rt.RenderData(SPP, limit, antialias, sky)
    got = {}
    for kind in ("entries off", "no plane", "generic", "entries"):
        ctx, scene = scene_of(rt, monkeypatch, models_dir, name, kind)
        got[kind] = one_frame(rt, ctx, scene, cam, rd)
        assert rt.primary_cull_plane(ctx)[0] == (kind in ("entries", "entries off")), kind
        if kind == "entries off":
            used, words = rt.primary_entry_words(ctx)
            assert used and not words.any(), "RT_AMD_PRIMARY_ENTRY=0 writes every entry word as 0"
    got["oracle"] = oracle(orc, models_dir, rt, name, cam, limit, antialias)
    for kind in ("entries off", "no plane", "generic", "oracle"):
        assert eq(got["entries"], got[kind]), (name, limit, antialias, "entries on against " + kind, mismatches(got["entries"], got[kind]))
    ctx, scene = scene_of(rt, monkeypatch, models_dir, name, "entries")
    return device_words(rt, ctx, scene, cam, antialias)


@pytest.mark.parametrize("limit,antialias", SETTINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", SCENES + ["monkey, ragged tiles"])
def test_five_renderings_agree(rt, orc, models_dir, monkeypatch, name, limit, antialias):
    w, h = (100, 67) if name.endswith("ragged tiles") else (96, 64)
    name = name.split(",")[0]
    words = five_way(rt, orc, monkeypatch, models_dir, name, rt.Camera(w, h), limit, antialias)
    if name in ("monkey", "soup"):
        assert (words & 1).any() and (words == NOTHING).any(), (name, "no pixel starts on a triangle or none is `nothing`: the case decides nothing")


@pytest.mark.parametrize("limit,antialias", [(8, True), (1, False)], ids=lambda v: str(v))
@pytest.mark.parametrize("name", PLACES)
def test_the_merge_with_the_simple_objects(rt, orc, models_dir, monkeypatch, name, limit, antialias):
    """the mesh first, last and emissive in the object list, a sphere in front of part of it"""
    words = five_way(rt, orc, monkeypatch, models_dir, name, rt.Camera(96, 64), limit, antialias)
    assert (words & 1).any(), name


@pytest.mark.parametrize("limit,antialias", [(8, True), (1, False)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", CAMERAS)
def test_five_renderings_agree_across_cameras(rt, orc, models_dir, monkeypatch, which, limit, antialias):
    if which == "inside the root box":
        cam = rt.Camera(96, 64, pos=INSIDE)
    elif which == "looking away":
        cam = rt.Camera(96, 64, rot=(0.0, float(np.pi), 0.0))
    elif which == "narrow field of view":
        cam = rt.Camera(96, 64, fov=0.035)
    else:
        pos, rot, fov = sweep_cameras()[int(which.split()[1])]
        cam = rt.Camera(96, 64, pos=pos, fov=fov, rot=rot)
    words = five_way(rt, orc, monkeypatch, models_dir, "monkey", cam, limit, antialias)
    if which == "looking away":
        assert not words.any(), "the camera looks away from the monkey: every pixel is flagged, every entry word is 0"
    if which == "narrow field of view" and antialias:
        assert (words == 0).mean() > 0.5, "a cone many pixels wide: most words are 0"


def three_ways(rt, monkeypatch, models_dir, name, launch):
    """launch(ctx, scene) -> a frame, on the contexts with the entries, with every word 0 and without a plane: equal as uint32; -> the first"""
    got = {kind: launch(*scene_of(rt, monkeypatch, models_dir, name, kind)) for kind in ("entries off", "no plane", "entries")}
    for kind in ("entries off", "no plane"):
        assert eq(got["entries"], got[kind]), ("entries on against " + kind, mismatches(got["entries"], got[kind]))
    return got["entries"]


@pytest.mark.parametrize("form", ["single frame", "three-frame batch", "bands", "shuffled tile list", "compact bands", "two contexts", "pipelined frame"])
def test_every_launch_form(rt, orc, models_dir, monkeypatch, form):
    w, h = 100, 67
    objs, sky = objects(rt, "monkey")
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, 8, True, sky)
    want1, want3 = oracle(orc, models_dir, rt, "monkey", cam, 8, True), oracle(orc, models_dir, rt, "monkey", cam, 8, True, frames=3)
    if form == "single frame":
        got = three_ways(rt, monkeypatch, models_dir, "monkey", lambda ctx, scene: one_frame(rt, ctx, scene, cam, rd))
        assert eq(got, want1), mismatches(got, want1)
    elif form == "three-frame batch":
        def launch(ctx, scene):
            out = buffer(w, h, GARBAGE)
            rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, out.data_ptr())
            return host(out)
        got = three_ways(rt, monkeypatch, models_dir, "monkey", launch)
        assert eq(got, want3), mismatches(got, want3)
    elif form == "bands":
        rows = band_rows_owned(h)

        def launch(ctx, scene):
            out = buffer(w, h, GARBAGE)
            rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, out.data_ptr(), **BAND)
            return host(out)
        got = three_ways(rt, monkeypatch, models_dir, "monkey", launch)
        assert eq(got[rows], want3[rows]), mismatches(got[rows], want3[rows])
    elif form == "shuffled tile list":
        tiles = random_tile_list(w, h)
        mask = tile_mask(w, h, tiles)

        def launch(ctx, scene):
            out = buffer(w, h, GARBAGE)
            rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, out.data_ptr(), tile_list=tiles)
            return host(out)
        got = three_ways(rt, monkeypatch, models_dir, "monkey", launch)
        assert eq(got[mask], want3[mask]), mismatches(got[mask], want3[mask])
        assert np.all(got[~mask].view(np.uint32) == F(GARBAGE).view(np.uint32)), "pixels of tiles that are not listed were written"
    elif form == "compact bands":
        rows = band_rows_owned(h)

        def launch(ctx, scene):
            out = buffer(w, h, GARBAGE)
            rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, out.data_ptr(), compact=True, **BAND)
            return host(out)
        got = three_ways(rt, monkeypatch, models_dir, "monkey", launch)
        assert eq(got[:len(rows)], want3[rows]), mismatches(got[:len(rows)], want3[rows])
    elif form == "two contexts":
        got = {}
        for kind in ("entries off", "entries"):
            ctxs = [context_with(rt, monkeypatch, SWITCHES[kind]) for _ in range(2)]
            scenes = [traits_scene(rt, c, monkeypatch, objs, models_dir) for c in ctxs]
            frame = buffer(w, h, GARBAGE)
            rt.render_multi_device(ctxs, scenes, cam, rd, TIMES[:1], 0, frame.data_ptr(), band_rows=8, stream=stream_of())
            rt.render_multi_device(ctxs, scenes, cam, rd, TIMES[1:], 1, frame.data_ptr(), band_rows=8, stream=stream_of())
            for c in ctxs:
                c.synchronize()
            got[kind] = host(frame)
            if kind == "entries":
                for c, s in zip(ctxs, scenes):
                    assert (device_words(rt, c, s, cam, True) & 1).any()
        assert eq(got["entries"], got["entries off"]), mismatches(got["entries"], got["entries off"])
        assert eq(got["entries"], want3), mismatches(got["entries"], want3)
    else:
        def launch(ctx, scene):
            out = buffer(w, h, GARBAGE)
            for t in TIMES:
                rt.frame_submit(ctx, scene, cam, rd, t)
            for i in range(len(TIMES)):
                rt.frame_collect(ctx, i, out.data_ptr(), stream=stream_of())
            rt.frame_wait(ctx)
            return host(out)
        got = three_ways(rt, monkeypatch, models_dir, "monkey", launch)
        assert eq(got, want3), mismatches(got, want3)
    ctx, scene = scene_of(rt, monkeypatch, models_dir, "monkey", "entries")
    if form != "two contexts":
        assert (device_words(rt, ctx, scene, cam, True) & 1).any()


def fresh_frame(rt, monkeypatch, models_dir, objs, cam, rd):
    ctx = context_with(rt, monkeypatch, SWITCHES["no plane"])
    return one_frame(rt, ctx, traits_scene(rt, ctx, monkeypatch, objs, models_dir), cam, rd)


def test_plane_life_camera_move_and_larger_image(rt, models_dir, monkeypatch):
    objs, sky = objects(rt, "monkey")
    ctx = context_with(rt, monkeypatch, {})
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    rd = rt.RenderData(SPP, 8, True, sky)
    seen = []
    for cam in (rt.Camera(96, 64), rt.Camera(96, 64, pos=(0.6, 0.2, 0.3)), rt.Camera(192, 128), rt.Camera(96, 64)):
        got = one_frame(rt, ctx, scene, cam, rd)
        seen.append(device_words(rt, ctx, scene, cam, True))
        want = fresh_frame(rt, monkeypatch, models_dir, objs, cam, rd)
        assert eq(got, want), mismatches(got, want)
    assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[3])


def test_plane_life_mesh_updates_move_the_words(rt, models_dir, monkeypatch):
    """update_mesh_device on one stream, then a launch on another; then the host form of the update: the entry words follow the mesh, and the
    frames are a fresh commit's"""
    import torch
    left, right = soup(11, 400, (-0.45, 0.0, 1.6)), soup(11, 400, (0.45, 0.0, 1.6))
    cam, rd = rt.Camera(96, 64), rt.RenderData(SPP, 8, True, SKY)
    ctx = context_with(rt, monkeypatch, {})
    scene = traits_scene(rt, ctx, monkeypatch, [("mesh", left, GREY), GROUND], models_dir)
    one_frame(rt, ctx, scene, cam, rd)
    before = device_words(rt, ctx, scene, cam, True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    moved = torch.from_numpy(right).to("cuda:0")
    out = buffer(96, 64, GARBAGE)
    torch.cuda.synchronize()
    scene.update_mesh_device(0, moved, stream=s1.cuda_stream)
    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, out.data_ptr(), stream=s2.cuda_stream)
    got = host(out)
    after = device_words(rt, ctx, scene, cam, True)
    assert not np.array_equal(before, after), "the entry words did not follow the mesh"
    want = fresh_frame(rt, monkeypatch, models_dir, [("mesh", right, GREY), GROUND], cam, rd)
    assert eq(got, want), mismatches(got, want)
    scene.update_mesh(0, left)
    got = one_frame(rt, ctx, scene, cam, rd)
    device_words(rt, ctx, scene, cam, True)
    want = fresh_frame(rt, monkeypatch, models_dir, [("mesh", left, GREY), GROUND], cam, rd)
    assert eq(got, want), mismatches(got, want)


def test_plane_life_two_scenes_alternate_with_a_generic_one_between(rt, models_dir, monkeypatch):
    a, b = [("mesh", soup(11, 400, (-0.45, 0.0, 1.6)), GREY), GROUND], [("mesh", soup(11, 400, (0.45, 0.0, 1.6)), GREY), GROUND]
    cam, rd = rt.Camera(96, 64), rt.RenderData(SPP, 8, True, SKY)
    ctx = context_with(rt, monkeypatch, {})
    sa, sb = traits_scene(rt, ctx, monkeypatch, a, models_dir), traits_scene(rt, ctx, monkeypatch, b, models_dir)
    two = generic_scene(rt, ctx, monkeypatch, two_meshes(), models_dir)
    want = {id(sa): fresh_frame(rt, monkeypatch, models_dir, a, cam, rd), id(sb): fresh_frame(rt, monkeypatch, models_dir, b, cam, rd)}
    words = []
    for scene in (sa, sb, two, sa):
        got = one_frame(rt, ctx, scene, cam, rd)
        if scene is two:
            assert not rt.primary_cull_plane(ctx)[0] and not rt.primary_entry_words(ctx)[0], "a scene on the generic kernel is handed no plane"
            continue
        words.append(device_words(rt, ctx, scene, cam, True))
        assert eq(got, want[id(scene)]), mismatches(got, want[id(scene)])
    assert not np.array_equal(words[0], words[1]) and np.array_equal(words[0], words[2])


@pytest.mark.parametrize("antialias", [True, False], ids=["antialias", "no antialias"])
@pytest.mark.parametrize("which", ["default", "inside the root box", "view 3"])
def test_the_device_words_are_the_host_functions(rt, models_dir, monkeypatch, which, antialias):
    """a ragged image (no multiple of 8, 32 or 64 pixels): the pre-pass's entry words against rt_debug_primary_entry_host, word for word"""
    w, h = 100, 67
    if which == "default":
        cam = rt.Camera(w, h)
    elif which == "inside the root box":
        cam = rt.Camera(w, h, pos=INSIDE)
    else:
        pos, rot, fov = sweep_cameras()[3]
        cam = rt.Camera(w, h, pos=pos, fov=fov, rot=rot)
    objs, sky = objects(rt, "monkey")
    ctx, scene = scene_of(rt, monkeypatch, models_dir, "monkey", "entries")
    one_frame(rt, ctx, scene, cam, rt.RenderData(1, 1, antialias, sky))
    words = device_words(rt, ctx, scene, cam, antialias)
    if which == "default":
        assert (words & 1).any()
