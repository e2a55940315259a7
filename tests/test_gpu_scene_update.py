"""Scene.update_mesh / update_mesh_device (rt_scene_update_mesh[_device]): a committed mesh rebuilt on the device from new vertices.

The yardstick is the definition: after an update everything the kernels read - Scene.debug_read(), the blob, the object table and the texture
coordinates as they are ON THE DEVICE - equals, as bytes and in every section, SceneObjects(new geometry).debug_flatten(), what a fresh commit
uploads.  On top of that every kernel family runs on updated scenes against its own yardstick (the check_* functions of
tests/test_gpu_random_scenes.py), an animated monkey is rendered against the CPU oracle, and the launch order is tried without host waits.
Sizes straddle what the code branches on: the chain shapes of tiny trees (1-9), the first full leaf level (1023-2049), REBUILD_LDS_TRIS (the
workgroup-local path against the global sort) and meshes of several global levels.  Nothing has a tolerance.  Run with -m gpu on an MI355X."""
import os

import numpy as np
import pytest

from test_gpu_random_scenes import FAMILIES, SOUP_FAMILIES, Case

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, LIMIT = 64, 48, 4, 4
SKY = (0.8, 1.0, 1.0)
GREY = ("standard", (0.6, 0.6, 0.7), 0.1)


def soup(seed, n, spread=0.5):
    rng = np.random.default_rng(seed)
    return (np.array([0.0, 0.1, 2.5]) + rng.normal(0, spread, (n, 1, 3)) + rng.normal(0, 0.06, (n, 3, 3))).astype(F).reshape(n, 9)


def around(tris):
    """a sphere, the mesh, a quad: the mesh's sections lie between other objects'"""
    return [("sphere", (0.9, 0.2, 2.0), 0.3, ("standard", (0.7, 0.3, 0.3), 0.5)), ("mesh", tris, GREY),
            ("quad", (-3, -1, 0), (3, -1, 0), (3, -1, 6), (-3, -1, 6), ("standard", (0.5, 0.5, 0.5), 0.2))]


def sections(d):
    """the flattened layout as named byte strings"""
    blob, off_objtab = d["blob"], d["off_meshes"] + 2 * d["num_meshes"]
    cuts = [("nodes", d["off_nodes"], d["off_objlds"]), ("objlds", d["off_objlds"], d["off_meshes"]), ("meshes", d["off_meshes"], off_objtab),
            ("objtab", off_objtab, d["off_tris"]), ("tris", d["off_tris"], len(blob))]
    out = {name: blob[a:b].tobytes() for name, a, b in cuts}
    out["objects"] = d["objects"].tobytes()
    out["tri_uv"] = b"" if d["tri_uv"] is None else d["tri_uv"].tobytes()
    return out


def assert_flat_equal(got, want, what):
    for k in ("off_nodes", "off_tris", "off_objlds", "off_meshes", "num_meshes", "stack_entries", "num_triangles", "num_nodes", "has_mesh"):
        assert got[k] == want[k], (what, k)
    g, w = sections(got), sections(want)
    for name in w:
        if g[name] != w[name]:
            a, b = np.frombuffer(g[name], np.uint32), np.frombuffer(w[name], np.uint32)
            bad = np.flatnonzero(a != b)
            raise AssertionError((what, name, "%d of %d words differ, first at %s" % (len(bad), len(b), bad[:6].tolist())))


def flat_of(rt, objs, models_dir):
    return rt.SceneObjects(objs, models_dir).debug_flatten()


def on_gpu(tris):
    import torch
    return torch.from_numpy(np.ascontiguousarray(tris, F)).to("cuda:0")


# ---- blob bytes against a fresh commit ----------------------------------------------------------------------------------------------------
LDS_TRIS = 2048                                          # rt.REBUILD_LDS_TRIS, asserted below: the sizes are written out so that they can name the cases
# every chain shape; the first full leaf level; LDS_TRIS - 1 (= 2047), LDS_TRIS, LDS_TRIS + 1 (= 2049), 2 LDS_TRIS + 3; the soup's and the surface's sizes; a large mesh
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049, 4099, 6000, 50880, 200003]


def test_the_sizes_straddle_the_paths(rt):
    assert rt.REBUILD_LDS_TRIS == LDS_TRIS and {LDS_TRIS - 1, LDS_TRIS, LDS_TRIS + 1, 2 * LDS_TRIS + 3} <= set(SIZES)


@pytest.mark.parametrize("n", SIZES)
def test_update_equals_a_fresh_commit(rt, ctx, models_dir, n):
    """old soup -> new soup by the device form, then back by the host form: both times the device holds the fresh commit's bytes"""
    old, new = soup(100 + n, n), soup(200 + n, n, 0.3)
    scene = ctx.commit(rt.SceneObjects(around(old), models_dir))
    want_old, want_new = flat_of(rt, around(old), models_dir), flat_of(rt, around(new), models_dir)
    assert_flat_equal(scene.debug_read(), want_old, (n, "as committed"))
    d_new = on_gpu(new)
    scene.update_mesh_device(1, d_new)
    assert_flat_equal(scene.debug_read(), want_new, (n, "device form"))
    scene.update_mesh(1, old)
    assert_flat_equal(scene.debug_read(), want_old, (n, "host form, back to the old soup"))


# ---- ties, signed zeros ---------------------------------------------------------------------------------------------------------------------
def root_keys(tris):
    """the root level's keys, restated in binary32: box, reference point, |p0 - ref| as sqrt((dx dx + dy dy) + dz dz)"""
    p = tris.reshape(-1, 3).astype(F)
    lo, hi = p.min(axis=0), p.max(axis=0)
    w, h, d = (hi - lo).astype(F)
    half = F(2)
    if w >= h and w >= d:
        ref = np.array([lo[0] + w / half, lo[1], lo[2] + d / half], F)
    elif h >= w and h >= d:
        ref = np.array([lo[0], lo[1] + h / half, lo[2] + d / half], F)
    else:
        ref = np.array([lo[0] + w / half, lo[1] + h / half, lo[2]], F)
    delta = (tris[:, 0:3] - ref).astype(F)
    sq = (delta * delta).astype(F)
    return np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)).astype(F)


def tied_meshes(n):
    base = soup(7, n)
    dup = base[np.arange(n) // 4].copy()
    fan = base.copy()
    fan[:, 0:3] = base[0, 0:3]
    same = np.repeat(base[:1], n, axis=0)
    return {"every triangle four times": dup, "a fan around one p0": fan, "identical triangles": same}


@pytest.mark.parametrize("which", ["every triangle four times", "a fan around one p0", "identical triangles"])
@pytest.mark.parametrize("n", [256, 2600])
def test_equal_keys_keep_the_reference_order(rt, ctx, models_dir, which, n):
    """a wrong tie direction changes the leaf order; n = 2600 ties in the global sort as well"""
    tris = tied_meshes(n)[which]
    keys = root_keys(tris)
    assert n - len(np.unique(keys)) >= n // 4, (which, len(np.unique(keys)))
    scene = ctx.commit(rt.SceneObjects(around(soup(8, n)), models_dir))
    scene.update_mesh_device(1, on_gpu(tris))
    assert_flat_equal(scene.debug_read(), flat_of(rt, around(tris), models_dir), (which, n))


def zero_mesh(n, seed=5):
    """Coordinates are -0, +0 or of one sign per triangle: a box of positive triangles has its low planes at a zero, one of negative triangles its
    high planes, at the zero its list meets first.  a.x, b.y, c.z are never zero, so no triangle has zero area."""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.integers(0, 2, (n, 1)) == 1, F(1), F(-1))
    t = (sign * rng.uniform(0.5, 1.5, (n, 9))).astype(F)
    pick = rng.integers(0, 3, (n, 9))
    pick[:, [0, 4, 8]] = 2
    t[pick == 0] = F(-0.0)
    t[pick == 1] = F(0.0)
    return t


@pytest.mark.parametrize("n", [600, 2500])
def test_signed_zeros_stay_where_the_list_order_puts_them(rt, ctx, models_dir, n):
    tris = zero_mesh(n)
    want = flat_of(rt, around(tris), models_dir)
    nodes = want["blob"][want["off_nodes"]:want["off_objlds"]].reshape(-1, 4, 4)
    # per stored node: the left and right boxes (lo.xyz, hi.xyz); each of the six planes lies at +0 somewhere and at -0 somewhere
    left = np.concatenate([nodes[:, 0, :], nodes[:, 1, :2]], axis=1)
    right = np.concatenate([nodes[:, 1, 2:], nodes[:, 2, :]], axis=1)
    boxes = np.concatenate([left, right]).view(np.uint32)
    for plane in range(6):
        assert (boxes[:, plane] == 0).any() and (boxes[:, plane] == 0x80000000).any(), plane
    for first in (soup(9, n), tris[::-1].copy()):
        scene = ctx.commit(rt.SceneObjects(around(first), models_dir))
        scene.update_mesh_device(1, on_gpu(tris))
        assert_flat_equal(scene.debug_read(), want, ("signed zeros", n))


# ---- several meshes, texture coordinates ---------------------------------------------------------------------------------------------------
def three_meshes(models_dir, angle, shift, seed):
    image = ("image", np.random.default_rng(3).uniform(0, 1, (4, 5, 3)).astype(F), 0.0)
    return [("mesh", soup(31, 40), GREY), ("sphere", (0.5, 0.5, 2.0), 0.2, GREY),
            ("obj", "cube.obj", [("enlarge", 0.3), ("rotate", angle, 0.4, 0.2), ("translate", shift, 0.0, 2.0)], image),
            ("sphere", (-0.5, 0.5, 2.0), 0.2, ("checkerboard", (1, 1, 1), (0, 0, 0), 4, 0.0)), ("mesh", soup(seed, 2100), GREY)]


def obj_triangles(rt, models_dir, o):
    m = rt.ObjFileMesh(os.path.join(models_dir, o[1]))
    for t in o[2]:
        getattr(m, t[0])(*t[1:])
    return m.triangles()


def test_the_middle_mesh_of_three_and_its_texture_coordinates(rt, ctx, models_dir):
    old, new = three_meshes(models_dir, 0.1, -0.2, 32), three_meshes(models_dir, 1.3, 0.3, 32)
    scene = ctx.commit(rt.SceneObjects(old, models_dir))
    before, want = scene.debug_read(), flat_of(rt, new, models_dir)
    assert want["tri_uv"] is not None and want["tri_uv"][40:52].any()          # the cube's quads carry texture coordinates
    assert not np.array_equal(flat_of(rt, old, models_dir)["tri_uv"], want["tri_uv"])      # ... which the new order moves
    scene.update_mesh(2, obj_triangles(rt, models_dir, new[2]))
    after = scene.debug_read()
    assert_flat_equal(after, want, "the cube between two soups")
    # the other two meshes and everything that is no mesh's: untouched
    tris_b, tris_a = sections(before)["tris"], sections(after)["tris"]
    assert tris_b[:40 * 48] == tris_a[:40 * 48] and tris_b[52 * 48:] == tris_a[52 * 48:]
    # the last mesh (2,100 triangles: one global level) after the middle one: its nodes and triangles lie behind another mesh's
    last = soup(33, 2100)
    scene.update_mesh_device(4, on_gpu(last))
    assert_flat_equal(scene.debug_read(), flat_of(rt, new[:4] + [("mesh", last, GREY)], models_dir), "the last of three")


# ---- every kernel family on an updated scene ------------------------------------------------------------------------------------------------
class UpdatedCase(Case):
    """a case of tests/test_gpu_random_scenes.py whose scene is committed with OTHER mesh geometry and then updated to the case's: objs, and with
    them every yardstick, describe the new geometry"""

    def __init__(self, kind, seed, placement="own"):
        super().__init__(kind, seed, placement)
        self.name = "updated " + self.name               # (the oracle's answers are cached by name)
        self.id = "updated-" + self.id

    def old_objs(self):
        rng = np.random.default_rng(1000 + self.seed)
        out = []
        for o in self.objs:
            if o[0] == "mesh":
                out.append(("mesh", (o[1] + rng.normal(0, 0.07, o[1].shape)).astype(F), o[2]))
            elif o[0] == "obj":
                out.append(("obj", o[1], list(o[2]) + [("rotate", 0.3, -0.2, 0.1), ("translate", 0.05, 0.02, -0.04)], o[3]))
            else:
                out.append(o)
        return out

    def commit(self, rt, ctx, monkeypatch, models_dir):
        new_objs, self.objs = self.objs, self.old_objs()
        try:
            scene = super().commit(rt, ctx, monkeypatch, models_dir)      # (asserts the placement)
        finally:
            self.objs = new_objs
        cam, rd = rt.Camera(W, H), rt.RenderData(2, 3, True, SKY)
        for _ in range(2):                               # a warm view of the OLD geometry: its tile order and costs must not outlive it
            rt.render(ctx, scene, cam, rd, rt.VariableRenderData(W, H), 77)
        info = scene.info()
        for i, o in enumerate(self.objs):
            if o[0] == "mesh":
                scene.update_mesh_device(i, on_gpu(o[1]))
            elif o[0] == "obj":
                scene.update_mesh(i, obj_triangles(rt, models_dir, o))
        assert scene.info() == info
        assert_flat_equal(scene.debug_read(), flat_of(rt, self.objs, models_dir), self.id)
        return scene


UPDATED = [UpdatedCase("random", 13), UpdatedCase("random", 13, "threads1024"), UpdatedCase("random", 13, "global"), UpdatedCase("soup", 0, "hybrid")]
UPDATED_CASES = [(f, c) for c in UPDATED for f in (FAMILIES if c.kind == "random" else SOUP_FAMILIES)]


@pytest.mark.parametrize("family,case", UPDATED_CASES, ids=["%s-%s" % (f, c.id) for f, c in UPDATED_CASES])
def test_family_on_an_updated_scene(rt, orc, ctx, models_dir, monkeypatch, family, case):
    scene = case.commit(rt, ctx, monkeypatch, models_dir)
    FAMILIES[family](rt, orc, ctx, models_dir, case, scene)


# ---- an animation ---------------------------------------------------------------------------------------------------------------------------
def test_an_animated_monkey(rt, orc, ctx, models_dir):
    objs, _ = rt.scenes.CONFIG_SCENES["monkey"]()
    base = obj_triangles(rt, models_dir, objs[0])
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    original = scene.debug_read()
    assert_flat_equal(original, flat_of(rt, objs, models_dir), "as committed")
    cam, rd = rt.Camera(W, H), rt.RenderData(SPP, LIMIT, True, SKY)
    for step in range(1, 6):
        tris = base.copy().reshape(-1, 3, 3)
        tris[:, :, 1] += (F(0.05) * np.sin(F(step) + F(3) * tris[:, :, 0])).astype(F)
        tris = tris.reshape(-1, 9)
        now = [("mesh", tris, objs[0][-1])] + list(objs[1:])
        scene.update_mesh_device(0, on_gpu(tris))
        assert_flat_equal(scene.debug_read(), flat_of(rt, now, models_dir), ("step", step))
        want = orc.Scene(now, orc.MATH_DET, models_dir).render(cam.floats(), W, H, SPP, LIMIT, SKY, time_ms=500 + step)
        got = rt.render(ctx, scene, cam, rd, rt.VariableRenderData(W, H), 500 + step)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("step", step, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    scene.update_mesh(0, base)
    assert_flat_equal(scene.debug_read(), original, "back to the original triangles")


# ---- the launch order, without host waits ---------------------------------------------------------------------------------------------------
N_ORDER = 2300                                           # one global level: the update is a chain of launches


@pytest.fixture(scope="module")
def order_rig(rt, models_dir):
    """streams, the calibrated sleep of tests/test_gpu_streams.py, the two geometries and their frames from fully synchronised calls on a fresh context"""
    import torch
    from test_gpu_streams import Rig
    rig = Rig(rt, models_dir)
    rig.old, rig.new = soup(41, N_ORDER), soup(42, N_ORDER, 0.3)
    rig.cam, rig.rd = rt.Camera(W, H), rt.RenderData(SPP, LIMIT, True, SKY)
    c = rt.Context(0)
    s = c.commit(rt.SceneObjects(around(rig.old), models_dir))
    rig.frame_old = rt.render(c, s, rig.cam, rig.rd, rt.VariableRenderData(W, H), 9).copy()
    s.update_mesh(1, rig.new)
    rig.frame_new = rt.render(c, s, rig.cam, rig.rd, rt.VariableRenderData(W, H), 9).copy()
    assert not np.array_equal(rig.frame_old, rig.frame_new)
    rig.d_new = on_gpu(rig.new)
    torch.cuda.synchronize()
    return rig


def fresh_scene(rt, rig, models_dir):
    c = rt.Context(0)
    return c, c.commit(rt.SceneObjects(around(rig.old), models_dir))


def frame_buffer(rig):
    return rig.torch.full((H, W, 3), 7.0, dtype=rig.torch.float32, device=rig.dev)


def same(frame, want):
    return np.array_equal(frame.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_vertices_written_on_the_stream_just_ahead_of_the_update(rt, models_dir, order_rig):
    rig, torch = order_rig, order_rig.torch
    c, s = fresh_scene(rt, rig, models_dir)
    s1, s2 = rig.streams[0], rig.streams[1]
    verts, out = torch.zeros_like(rig.d_new), frame_buffer(rig)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        rig.sleep(30.0)
        verts.copy_(rig.d_new, non_blocking=True)        # the vertices exist only once the sleep has passed
        s.update_mesh_device(1, verts, stream=s1.cuda_stream)
    rt.render_device(c, s, rig.cam, rig.rd, 9, 0, out.data_ptr(), stream=s2.cuda_stream)       # another stream: ordered by the context
    c.synchronize()
    torch.cuda.synchronize()
    assert same(out, rig.frame_new)


def test_a_render_queued_before_the_update_shows_the_old_mesh(rt, models_dir, order_rig):
    rig, torch = order_rig, order_rig.torch
    c, s = fresh_scene(rt, rig, models_dir)
    s1, s2 = rig.streams[0], rig.streams[1]
    before, after = frame_buffer(rig), frame_buffer(rig)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        rig.sleep(30.0)
    rt.render_device(c, s, rig.cam, rig.rd, 9, 0, before.data_ptr(), stream=s1.cuda_stream)     # behind the sleep
    s.update_mesh_device(1, rig.d_new, stream=s2.cuda_stream)                                   # issued later, on a free stream
    rt.render_device(c, s, rig.cam, rig.rd, 9, 0, after.data_ptr(), stream=s2.cuda_stream)
    c.synchronize()
    torch.cuda.synchronize()
    assert same(before, rig.frame_old) and same(after, rig.frame_new)


def test_an_update_behind_frames_in_flight(rt, models_dir, order_rig):
    rig, torch = order_rig, order_rig.torch
    c, s = fresh_scene(rt, rig, models_dir)
    first, second, after = frame_buffer(rig), frame_buffer(rig), frame_buffer(rig)
    torch.cuda.synchronize()
    rt.frame_submit(c, s, rig.cam, rig.rd, 9)
    rt.frame_submit(c, s, rig.cam, rig.rd, 9)
    s.update_mesh_device(1, rig.d_new, stream=rig.streams[2].cuda_stream)
    rt.frame_collect(c, 0, first.data_ptr(), stream=rig.streams[0].cuda_stream)
    rt.frame_collect(c, 0, second.data_ptr(), stream=rig.streams[0].cuda_stream)
    rt.render_device(c, s, rig.cam, rig.rd, 9, 0, after.data_ptr(), stream=rig.streams[1].cuda_stream)
    c.synchronize()
    torch.cuda.synchronize()
    assert same(first, rig.frame_old) and same(second, rig.frame_old) and same(after, rig.frame_new)


def test_a_larger_update_regrows_the_scratch_a_pending_one_uses(rt, models_dir, order_rig):
    rig, torch = order_rig, order_rig.torch
    c, s = fresh_scene(rt, rig, models_dir)
    big_old, big_new = soup(43, 9000), soup(44, 9000, 0.3)
    big = c.commit(rt.SceneObjects(around(big_old), models_dir))
    d_big = on_gpu(big_new)
    torch.cuda.synchronize()
    with torch.cuda.stream(rig.streams[0]):
        rig.sleep(30.0)
    s.update_mesh_device(1, rig.d_new, stream=rig.streams[0].cuda_stream)       # pending behind the sleep, on scratch sized for 2,300 triangles
    big.update_mesh_device(1, d_big, stream=rig.streams[1].cuda_stream)         # needs four times the words and lists
    c.synchronize()
    torch.cuda.synchronize()
    assert_flat_equal(s.debug_read(), flat_of(rt, around(rig.new), models_dir), "the pending update")
    assert_flat_equal(big.debug_read(), flat_of(rt, around(big_new), models_dir), "the larger one")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_alone(rt, models_dir, order_rig):
    rig = order_rig
    c, s = fresh_scene(rt, rig, models_dir)
    other = rt.Context(0)
    before = s.debug_read()
    d = rig.d_new
    bad_host = rig.new.copy()
    bad_host[17, 4] = np.nan
    huge = rig.new.copy()
    huge[3, 0] = F(1e30)
    calls = [lambda: s.update_mesh_device(-1, d), lambda: s.update_mesh_device(3, d), lambda: s.update_mesh_device(0, d), lambda: s.update_mesh_device(2, d),
             lambda: s.update_mesh_device(1, d[:-9]), lambda: s.update_mesh(1, rig.new[:-1]), lambda: s.update_mesh(1, np.concatenate([rig.new, rig.new[:1]])),
             lambda: s.update_mesh(1, bad_host), lambda: s.update_mesh(1, huge), lambda: s.update_mesh(0, rig.new), lambda: s.update_mesh_device(1, 0, n=N_ORDER),
             lambda: c._check(rt.lib().rt_scene_update_mesh_device(other._h, s._h, 1, rt.C.c_void_p(d.data_ptr()), N_ORDER, None)),
             lambda: other._check(rt.lib().rt_scene_update_mesh(other._h, s._h, 1, rig.new.ctypes.data_as(rt.C.POINTER(rt.C.c_float)), N_ORDER))]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert_flat_equal(s.debug_read(), before, ("after refusal", i))
    got = rt.render(c, s, rig.cam, rig.rd, rt.VariableRenderData(W, H), 9)
    assert np.array_equal(got.view(np.uint32), rig.frame_old.view(np.uint32))
