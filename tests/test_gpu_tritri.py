"""The triangle-overlap queries on the GPU (rt_overlap_triangles[_device]) against tests/tritri_ref.py, the NumPy binary32 yardstick that
evaluates every candidate of every query: every count, every byte, every id and every segment compared as BYTES.

Scenes (tests/multihit_scenes.py): three-sphere, cube, monkey, reference scenes 0 and 4, the two richest seeds of tests/random_scenes.py,
nine meshes of 1 to 9 triangles, a 3,000-triangle mesh read from global memory, soup6k on the hybrid and on the global placement - the
placement asserted from scene.info() - with 300 seeded queries each (tritri_ref.query_triangles: centres in the bounds of the scene's
triangles, 5, 10 and 30 % of their diagonal across; a fifth of them tritri_ref.anchored_triangles: a vertex on a scene vertex, an edge
through one, the query in a triangle's plane).  Each scene and shape test first asserts, from the yardstick alone, that its queries reach
the walk: at least ten of them meet some but not all of the meshes' triangles, and one meets more than eight candidates.  Every shape of
RT_SHAPES is forced the way tests/test_gpu_shapes.py forces it, on the smallest scene that reaches it.  k: 0, 1, 2, 3, 8, with the
segments wherever k > 0; each output alone and all together; the any-only mode against count > 0.  The yardstick's answers are computed
once per scene (at k = 8: the ids and segments of a smaller k are their first columns) and shared.  Further: query counts around a wave
and past one chunk per resident wave, queries that are not finite, a zero-area query, a query holding the scene, a query in a cube face's
plane, an updated mesh, the launch order on a sleeping stream and beside a box-overlap call, collide_mesh, the refusals,
host/example_slice.cpp.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import multihit_scenes as S
import tritri_ref as R
from overlap_ref import surface_bounds
from test_gpu_shapes import SHAPES, _id, commit_as, plan, spheres_beyond_lds

pytestmark = pytest.mark.gpu

N_RANDOM, N_ANCHORED = 240, 60
KS = (0, 1, 2, 3, 8)
_REFS = {}
SEEDS = {"three_sphere": 1, "cube": 2, "monkey": 3, "reference_scene0": 4, "reference_scene4": 5, "random13": 6, "random15": 7, "tiny_meshes": 8,
         "soup3000": 9, "soup6k": 10, "spheres_beyond_lds": 11}


def objects_of(rt, name):
    if name == "spheres_beyond_lds":
        return rt.scenes.reference_scene4(num_spheres=spheres_beyond_lds(rt))[0]
    return S.objects_of(rt, name)


def answers(flat, tris):
    """the yardstick's answers at k = 8 with segments, and what its queries reach"""
    detail = {}
    counts, flags, ids, segs = R.overlap(flat, tris, 8, True, detail)
    in_mesh, mesh_tris = R.mesh_counts(flat, detail)
    return {"flat": flat, "tris": tris, "counts": counts, "any": flags, "ids": ids, "segs": segs, "in_mesh": in_mesh, "mesh_tris": mesh_tris}


def reference(rt, models_dir, name):
    if name not in _REFS:
        flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
        tris = np.concatenate([R.query_triangles(flat, SEEDS[name], N_RANDOM), R.anchored_triangles(flat, 100 + SEEDS[name], N_ANCHORED)])
        _REFS[name] = answers(flat, tris)
    return _REFS[name]


def reaches_the_walk(ref, name):
    """the queries ask both answers, and on a scene with a mesh at least ten of them meet some but not all of the meshes' triangles - the
    walk of the tree is entered and prunes - and one meets more than eight candidates where the scene has that many"""
    assert (ref["counts"] > 0).any() and (ref["counts"] == 0).any(), (name, "the queries do not reach both answers")
    if ref["mesh_tris"] > 1:
        partial = (ref["in_mesh"] > 0) & (ref["in_mesh"] < ref["mesh_tris"])
        assert partial.sum() >= 10, (name, "fewer than ten queries meet a part of the meshes", int(partial.sum()))
        assert (ref["counts"] > 3).any(), (name, "no query has more hits than the k of 1, 2 and 3 keep")
    if ref["mesh_tris"] > 50:
        assert (ref["counts"] > 8).any(), (name, "no query meets more than eight candidates")
        assert ((ref["counts"] > 0) & (ref["counts"] < 8)).any(), (name, "no query leaves slots empty behind its ids")
        assert (ref["segs"]["kind"] == 1).any(), (name, "no segment")


def same(got, ref, k, what, rows=slice(None)):
    counts, ids = got[0], got[1]
    assert counts.dtype == np.int32 and counts.tobytes() == ref["counts"][rows].tobytes(), (what, "counts differ at", np.nonzero(counts != ref["counts"][rows])[0][:5])
    want = np.ascontiguousarray(ref["ids"][rows][:, :k])
    assert ids.dtype == want.dtype and ids.shape == want.shape and ids.tobytes() == want.tobytes(), (what, "ids differ at", np.argwhere(ids != want)[:5].tolist())
    if len(got) > 2:
        want = np.ascontiguousarray(ref["segs"][rows][:, :k])
        segs = got[2]
        assert segs.dtype == want.dtype and segs.shape == want.shape
        assert segs.tobytes() == want.tobytes(), (what, "segments differ at", np.argwhere(segs.view(np.uint8).reshape(want.shape + (32,)) != want.view(np.uint8).reshape(want.shape + (32,)))[:5].tolist())


def check_scene(rt, ctx, scene, ref, what, ks=KS):
    tris = ref["tris"]
    for k in ks:
        same(rt.overlap_triangles(scene, tris, k, segments=k > 0), ref, k, "%s, k=%d" % (what, k))
    same(rt.overlap_triangles(scene, tris, 8), ref, 8, "%s, k=8 without segments" % what)
    touch = rt.triangles_touch(scene, tris)
    assert touch.dtype == bool and np.array_equal(touch, ref["counts"] > 0), (what, "any-only differs at", np.nonzero(touch != (ref["counts"] > 0))[0][:5])


# ---- scenes on the placement they pick or are given ---------------------------------------------------------------------------------
PLACED = [("three_sphere", {}, 1), ("cube", {}, 1), ("monkey", {}, 1), ("reference_scene0", {}, 1), ("reference_scene4", {}, 1), ("random13", {}, 1),
          ("random15", {}, 1), ("tiny_meshes", {}, 1), ("soup3000", {"RT_AMD_SCENE_MODE": "0"}, 0), ("soup6k", {}, 2), ("soup6k", {"RT_AMD_SCENE_MODE": "0"}, 0)]


@pytest.mark.parametrize("name,env,mode", PLACED, ids=["%s-%s" % (n, {0: "global", 1: "lds", 2: "hybrid"}[m]) for n, _, m in PLACED])
def test_answers_equal_the_yardstick(rt, ctx, models_dir, monkeypatch, name, env, mode):
    scene = commit_as(rt, ctx, monkeypatch, objects_of(rt, name), models_dir, env)
    info = scene.info()
    assert info["scene_in_lds"] == mode, (name, info)
    ref = reference(rt, models_dir, name)
    reaches_the_walk(ref, name)
    check_scene(rt, ctx, scene, ref, "%s %s" % (name, info))


# ---- every shape, forced ------------------------------------------------------------------------------------------------------------
def smallest_scene(shape):
    has_mesh, mode, _ = shape
    if mode == 1:
        return "cube" if has_mesh else "three_sphere"
    return plan(shape)[1][0]                                            # soup6k, or the spheres that leave LDS


@pytest.mark.parametrize("shape", SHAPES, ids=[_id(s) for s in SHAPES])
def test_every_shape_equals_the_yardstick(rt, ctx, models_dir, monkeypatch, shape):
    env, scenes = plan(shape)
    assert scenes, "RT_SHAPES has the shape %s and tests/test_gpu_shapes.py has no scene that reaches it" % (shape,)
    name = smallest_scene(shape)
    objs = objects_of(rt, name)
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    ref = reference(rt, models_dir, name)
    assert (int(ref["flat"]["has_mesh"]), info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    reaches_the_walk(ref, name)
    check_scene(rt, ctx, scene, ref, "%s on %s" % (name, _id(shape)), ks=(0, 3, 8))


# ---- each output alone and all together ---------------------------------------------------------------------------------------------
def test_each_output_alone_and_all_together(rt, ctx, models_dir):
    import torch
    name = "random13"
    ref = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    n = ref["tris"].shape[0]
    d_tris = torch.from_numpy(ref["tris"]).to("cuda:0")
    fresh = lambda: (torch.full((n, 3, 8), 0xA5, dtype=torch.uint8, device="cuda:0"), torch.full((n,), -7, dtype=torch.int32, device="cuda:0"),
                     torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0"), torch.full((n, 3, 32), 0xA5, dtype=torch.uint8, device="cuda:0"))
    want_ids = np.ascontiguousarray(ref["ids"][:, :3]).tobytes()
    want_segs = np.ascontiguousarray(ref["segs"][:, :3]).tobytes()
    for use in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 1, 0, 0), (1, 0, 1, 0), (0, 1, 1, 0), (1, 1, 1, 0), (1, 0, 0, 1), (1, 1, 1, 1)):
        ids, counts, flags, segs = fresh()
        rt.overlap_triangles_device(scene, d_tris, 3 if use[0] else 0, ids=ids if use[0] else None, counts=counts if use[1] else None,
                                    any=flags if use[2] else None, segments=segs if use[3] else None)
        torch.cuda.synchronize()
        assert ids.cpu().numpy().tobytes() == (want_ids if use[0] else b"\xa5" * (n * 24)), use
        assert counts.cpu().numpy().tobytes() == (ref["counts"].tobytes() if use[1] else np.full(n, -7, np.int32).tobytes()), use
        assert flags.cpu().numpy().tobytes() == (ref["any"].tobytes() if use[2] else b"\xa5" * n), use
        assert segs.cpu().numpy().tobytes() == (want_segs if use[3] else b"\xa5" * (n * 96)), use
    # new tensors where none were passed; pointers with n
    counts, ids, flags, segs = rt.overlap_triangles_device(scene, d_tris, 2, segments=True)
    torch.cuda.synchronize()
    assert flags is None and counts.cpu().numpy().tobytes() == ref["counts"].tobytes()
    assert ids.cpu().numpy().view(rt.OverlapId)[..., 0].tobytes() == np.ascontiguousarray(ref["ids"][:, :2]).tobytes()
    assert segs.cpu().numpy().view(rt.TriSegment)[..., 0].tobytes() == np.ascontiguousarray(ref["segs"][:, :2]).tobytes()
    ids, counts, flags, segs = fresh()
    rt.overlap_triangles_device(scene, d_tris.data_ptr(), 3, ids=ids.data_ptr(), counts=None, any=flags.data_ptr(), segments=segs.data_ptr(), n=n)
    torch.cuda.synchronize()
    assert ids.cpu().numpy().tobytes() == want_ids and flags.cpu().numpy().tobytes() == ref["any"].tobytes() and segs.cpu().numpy().tobytes() == want_segs
    assert ctx.last_kernel_ms() > 0.0


# ---- counts around a wave and a chunk, and past one chunk per resident wave ------------------------------------------------------------
def test_query_counts(rt, ctx, models_dir):
    from test_gpu_refill import batch_size
    name = "monkey"
    ref = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    tris = ref["tris"]
    for k in (3, 0):
        for n in (1, 63, 64, 65):
            same(rt.overlap_triangles(scene, tris[:n], k, segments=k > 0), ref, k, "%s n=%d k=%d" % (name, n, k), slice(0, n))
    for n in (1, 63, 64, 65):
        assert np.array_equal(rt.triangles_touch(scene, tris[:n]), ref["counts"][:n] > 0), n
    counts, ids, segs = rt.overlap_triangles(scene, np.zeros((0, 9), np.float32), 4, segments=True)
    assert ids.shape == (0, 4) and counts.shape == (0,) and segs.shape == (0, 4)
    # more queries than one chunk per resident wave: the refill path, every lane of every wave more than once
    n = batch_size()
    idx = np.random.default_rng(5).integers(0, tris.shape[0], n)
    many = np.ascontiguousarray(tris[idx])
    same(rt.overlap_triangles(scene, many, 3, segments=True), ref, 3, "%s n=%d k=3" % (name, n), idx)
    same(rt.overlap_triangles(scene, many, 0), ref, 0, "%s n=%d k=0" % (name, n), idx)
    assert np.array_equal(rt.triangles_touch(scene, many), ref["counts"][idx] > 0), "any-only past one chunk per wave"


# ---- queries that are not finite, a zero-area query, a query that holds the scene, a query in a cube face's plane ------------------------
def test_invalid_zero_area_whole_scene_and_coplanar_queries(rt, ctx, models_dir):
    name = "random15"
    ref = reference(rt, models_dir, name)
    flat = ref["flat"]
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    slo, shi = (np.asarray(b, np.float64) for b in surface_bounds(flat))
    mid, ext = (slo + shi) / 2, (shi - slo)
    # a triangle whose bounding box holds every triangle of the scene: the walk enters every leaf (and the triangle cuts what it cuts)
    big = np.concatenate([mid - 4 * ext, mid + [4 * ext[0], 4 * ext[1], -4 * ext[2]], mid + [0, 0, 6 * ext[2]]]).astype(np.float32)
    v = R.record_vertices(R.sections(flat)[2])[R.sections(flat)[2].shape[0] // 2]
    q = np.stack([big, big, big, big, np.concatenate([v[0], v[1], v[1]]), np.concatenate([v[0], v[0], v[0]])]).astype(np.float32)
    q[1, 0] = np.nan
    q[2, 5] = np.inf
    q[3, 7] = -np.inf
    got = answers(flat, q)
    assert (got["counts"][1:4] == 0).all() and got["counts"][0] > 8 and got["counts"][4] >= 1 and got["counts"][5] >= 1, got["counts"]
    same(rt.overlap_triangles(scene, q, 8, segments=True), got, 8, "invalid, zero-area and whole-scene queries")
    assert np.array_equal(rt.triangles_touch(scene, q), got["counts"] > 0)
    # an axis-aligned cube: queries in its faces' planes take the coplanar path, on exactly representable coordinates
    objs = [("obj", "cube.obj", [("enlarge", 0.25), ("translate", 0, 0, 2)], ("standard", (0.8, 0.4, 0.2), 0))]
    cube_flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    cq = R.anchored_triangles(cube_flat, 21, 90, sizes=(0.1, 0.3, 0.5))[2::3]
    want = answers(cube_flat, cq)
    coplanar = (want["segs"]["kind"] == 2) & (want["ids"]["triangle"] >= 0)
    assert coplanar.sum() >= 10 and (want["counts"] == 0).any(), ("the queries do not reach the coplanar path", int(coplanar.sum()))
    cube = ctx.commit(rt.SceneObjects(objs, models_dir))
    same(rt.overlap_triangles(cube, cq, 8, segments=True), want, 8, "queries in a cube face's plane")


# ---- a scene updated on the device ---------------------------------------------------------------------------------------------------
def test_after_update_mesh_device(rt, ctx, models_dir):
    import torch
    rng = np.random.default_rng(8)
    n = 700
    old = (np.array([0.0, 0.0, 2.0]) + rng.normal(0, 0.3, (n, 1, 3)) + rng.normal(0, 0.1, (n, 3, 3))).astype(np.float32).reshape(n, 9)
    new = (old * np.float32(1.15) + rng.normal(0, 0.02, old.shape)).astype(np.float32)
    sphere = ("sphere", (0.7, 0.4, 1.4), 0.2, ("standard", (0.5, 0.5, 0.5), 0.0))
    mat = ("standard", (0.6, 0.6, 0.6), 0.1)
    scene = ctx.commit(rt.SceneObjects([sphere, ("mesh", old, mat)], models_dir))
    fresh_objs = rt.SceneObjects([sphere, ("mesh", new, mat)], models_dir)
    tris = R.query_triangles(fresh_objs.debug_flatten(), 3, 300)
    before = rt.overlap_triangles(scene, tris, 4, segments=True)
    scene.update_mesh_device(1, torch.from_numpy(new).to("cuda:0"))
    after = rt.overlap_triangles(scene, tris, 4, segments=True)
    fresh = rt.overlap_triangles(ctx.commit(fresh_objs), tris, 4, segments=True)
    assert all(a.tobytes() == f.tobytes() for a, f in zip(after, fresh)), "updated against a fresh commit"
    counts, _, ids, segs = R.overlap(scene.debug_read(), tris, 4, True)
    assert after[0].tobytes() == counts.tobytes() and after[1].tobytes() == ids.tobytes() and after[2].tobytes() == segs.tobytes(), "updated against the yardstick on the device's scene"
    assert before[0].tobytes() != after[0].tobytes()


# ---- the launch order: a sleeping stream, and the box-overlap kernel on a second stream --------------------------------------------------
def test_triangles_produced_on_the_stream_just_ahead_of_the_call(rt, models_dir):
    """In the manner of tests/test_gpu_overlap.py: on a sleeping stream the triangles are copied into place, the call is queued, the
    answers are copied out - the host waits for nothing in between - and the answers are the yardstick's."""
    import torch
    name = "monkey"
    ref = reference(rt, models_dir, name)
    n, k = ref["tris"].shape[0], 4
    dev = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    src = torch.from_numpy(ref["tris"]).to(dev)
    buf = torch.empty_like(src)
    ids = torch.empty((n, k, 8), dtype=torch.uint8, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    segs = torch.empty((n, k, 32), dtype=torch.uint8, device=dev)
    res_ids, res_cnt, res_flags, res_segs = torch.empty_like(ids), torch.empty_like(cnt), torch.empty_like(flags), torch.empty_like(segs)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rt.overlap_triangles_device(scene, src, k, ids=ids, counts=cnt, any=flags, segments=segs, stream=stream.cuda_stream)      # warm: the kernel is loaded, the stream has its queue
    torch.cuda.synchronize()
    buf.fill_(float("nan"))
    ids.fill_(0xEE)
    cnt.fill_(-7)
    flags.fill_(0xEE)
    segs.fill_(0xEE)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(60000000)
        buf.copy_(src, non_blocking=True)
        rt.overlap_triangles_device(scene, buf, k, ids=ids, counts=cnt, any=flags, segments=segs, stream=stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        pending = not ev.query()
        res_ids.copy_(ids, non_blocking=True)
        res_cnt.copy_(cnt, non_blocking=True)
        res_flags.copy_(flags, non_blocking=True)
        res_segs.copy_(segs, non_blocking=True)
    torch.cuda.synchronize()
    assert pending, "the stream had run dry before the call returned: the window was not open"
    assert res_cnt.cpu().numpy().tobytes() == ref["counts"].tobytes() and res_flags.cpu().numpy().tobytes() == ref["any"].tobytes(), "queued behind the producer of its triangles"
    assert res_ids.cpu().numpy().tobytes() == np.ascontiguousarray(ref["ids"][:, :k]).tobytes(), "queued behind the producer of its triangles"
    assert res_segs.cpu().numpy().tobytes() == np.ascontiguousarray(ref["segs"][:, :k]).tobytes(), "queued behind the producer of its triangles"


def test_beside_a_box_overlap_call_on_a_second_stream(rt, models_dir):
    """rt_overlap_triangles_device and rt_overlap_boxes_device share a launcher and an argument type: queued back to back on two streams
    of one context, without a wait between them, both answer as their synchronised selves"""
    import torch
    name = "monkey"
    ref = reference(rt, models_dir, name)
    q = ref["tris"].reshape(-1, 3, 3)
    lo, hi = np.ascontiguousarray(q.min(axis=1)), np.ascontiguousarray(q.max(axis=1))
    n, k = q.shape[0], 3
    dev = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    want_box = rt.overlap_boxes(scene, lo, hi, k)
    want_tri = rt.overlap_triangles(scene, ref["tris"], k, segments=True)
    same(want_tri, ref, k, "the synchronised call")
    d_lo, d_hi, d_tris = (torch.from_numpy(a).to(dev) for a in (lo, hi, ref["tris"]))
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    ids = torch.full((n, k, 8), 0xEE, dtype=torch.uint8, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    segs = torch.full((n, k, 32), 0xEE, dtype=torch.uint8, device=dev)
    bids = torch.full((n, k, 8), 0xEE, dtype=torch.uint8, device=dev)
    bcnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for _ in range(2):
        rt.overlap_triangles_device(scene, d_tris, k, ids=ids, counts=cnt, segments=segs, stream=s1.cuda_stream)
        rt.overlap_boxes_device(scene, d_lo, d_hi, k, ids=bids, counts=bcnt, stream=s2.cuda_stream)
        rt.overlap_triangles_device(scene, d_tris, k, ids=ids, counts=cnt, segments=segs, stream=s1.cuda_stream)
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tobytes() == want_tri[0].tobytes() and ids.cpu().numpy().tobytes() == want_tri[1].tobytes(), "the triangle answers beside a box-overlap launch"
    assert segs.cpu().numpy().tobytes() == want_tri[2].tobytes(), "the segments beside a box-overlap launch"
    assert bcnt.cpu().numpy().tobytes() == want_box[0].tobytes() and bids.cpu().numpy().tobytes() == want_box[1].tobytes(), "the box answers beside a triangle-overlap launch"


# ---- a mesh against the scene ---------------------------------------------------------------------------------------------------------
def test_collide_mesh_cube_lowered_into_the_monkey(rt, ctx, models_dir):
    name = "monkey"
    flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    # the cube's twelve triangles, read from its own flattened scene, set down over the monkey's head
    cube = [("obj", "cube.obj", [("enlarge", 0.2), ("rotate", 0.3, 0.5, 0.1), ("translate", 0.1, 0.15, 1.6)], ("standard", (1, 1, 1), 0))]
    tool = R.record_vertices(R.sections(rt.SceneObjects(cube, models_dir).debug_flatten())[2]).reshape(-1, 9)
    assert tool.shape == (12, 9)
    want = answers(flat, tool)
    assert (want["counts"] > 8).any() and (want["counts"] > 0).sum() >= 6, want["counts"]
    for k in (8, 3):
        got = rt.collide_mesh(scene, tool.reshape(-1, 3, 3), k)
        held = want["ids"][:, :k]["object"] >= 0
        rows = np.broadcast_to(np.arange(12)[:, None], held.shape)[held]
        assert np.array_equal(got["query"], rows) and np.array_equal(got["object"], want["ids"][:, :k]["object"][held])
        assert np.array_equal(got["triangle"], want["ids"][:, :k]["triangle"][held]) and np.array_equal(got["kind"], want["segs"][:, :k]["kind"][held])
        assert got["p"].tobytes() == want["segs"][:, :k]["p"][held].tobytes() and got["q"].tobytes() == want["segs"][:, :k]["q"][held].tobytes()
        assert np.array_equal(got["truncated"], want["counts"] > k) and got["truncated"].any() and got["counts"].tobytes() == want["counts"].tobytes()
    with pytest.raises(ValueError):
        rt.collide_mesh(scene, tool, 0)


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    name = "three_sphere"
    ref = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    before = rt.overlap_triangles(scene, ref["tris"], 2, segments=True)
    tris = torch.zeros((4, 9), dtype=torch.float32, device="cuda:0")
    out = torch.full((4 * 2 * 8 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    sg = torch.full((4 * 2 * 32 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    cnt = torch.full((4,), -3, dtype=torch.int32, device="cuda:0")
    flags = torch.full((4,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert out.data_ptr() % 8 == 0 and sg.data_ptr() % 16 == 0
    p, h, c, a, s = (C.c_void_p(x.data_ptr()) for x in (tris, out, cnt, flags, sg))
    dev = L.rt_overlap_triangles_device
    bad = rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, -1, 2, h, c, a, s, None) == bad and dev(ctx._h, scene._h, p, (1 << 30) + 1, 2, h, c, a, s, None) == bad
    assert dev(ctx._h, scene._h, p, 4, -1, h, c, a, s, None) == bad and dev(ctx._h, scene._h, p, 4, 9, h, c, a, s, None) == bad
    assert dev(ctx._h, scene._h, None, 4, 2, h, c, a, s, None) == bad
    assert dev(ctx._h, scene._h, p, 4, 2, None, c, a, None, None) == bad and "null ids" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, 4, 2, C.c_void_p(out.data_ptr() + 4), c, a, s, None) == bad and "8-byte aligned" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, 4, 2, h, c, a, C.c_void_p(sg.data_ptr() + 8), None) == bad and "16-byte aligned" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, 4, 0, None, None, None, None, None) == bad and "no output" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, 4, 0, None, c, None, s, None) == bad and "segments asked for" in ctx.last_error()
    assert dev(ctx._h, foreign._h, p, 4, 2, h, c, a, s, None) == bad and "another context" in ctx.last_error()
    assert dev(None, scene._h, p, 4, 2, h, c, a, s, None) == bad and dev(ctx._h, None, p, 4, 2, h, c, a, s, None) == bad
    assert dev(ctx._h, scene._h, None, 0, 2, None, None, None, None, None) == rt.RT_OK
    crowd = [("sphere", (0.01 * (i % 70), 0.01 * (i // 70), 2.0), 0.004, ("standard", (0.5, 0.5, 0.5), 0.0)) for i in range(4097)]
    crowded = ctx.commit(rt.SceneObjects(crowd, models_dir))
    assert dev(ctx._h, crowded._h, p, 4, 2, h, c, a, s, None) == bad and "too many objects" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x77).all()) and bool((sg == 0x77).all()) and bool((cnt == -3).all()) and bool((flags == 0x77).all()), "a refused call wrote"
    with pytest.raises(ValueError):
        rt.overlap_triangles(scene, np.zeros((1, 9), np.float32), 9)
    with pytest.raises(ValueError):
        rt.overlap_triangles(scene, np.zeros((1, 9), np.float32), 0, segments=True)
    with pytest.raises(ValueError):
        rt.overlap_triangles_device(scene, tris.double(), 2)
    after = rt.overlap_triangles(scene, ref["tris"], 2, segments=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(after, before)), "a call behind the refusals answers as before"
    same(after, ref, 2, "behind the refusals")


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_example_slice_program(rt, models_dir, tmp_path):
    """host/example_slice.cpp (Renderer::overlap_triangles, Renderer::touches of host/raytracer.hpp): it builds, its tile, segment and
    truncation counts and its probe are the yardstick's for the same scene and tiles, and the PGM holds an outline"""
    import re
    import subprocess
    exe = rt.build.build_slice_example()
    M, height = 12, -0.05
    pgm = tmp_path / "slice.pgm"
    r = subprocess.run([exe, models_dir, str(height), str(M), str(pgm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    objs = [("obj", "low_poly_monkey.obj", [("enlarge", 0.3), ("rotate", 0, 2.3, 0), ("translate", 0.1, -0.1, 1.6)], ("standard", (1, 1, 1), 0.0))]
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    side = 1.3
    ex = (0.1 - side / 2 + side * np.arange(M + 1, dtype=np.float64) / M).astype(np.float32)
    ez = (1.6 - side / 2 + side * np.arange(M + 1, dtype=np.float64) / M).astype(np.float32)
    y = np.float32(height)
    tiles = []
    for i in range(M):
        for j in range(M):
            xa, xb, za, zb = ex[i], ex[i + 1], ez[j], ez[j + 1]
            tiles += [[xa, y, za, xb, y, za, xb, y, zb], [xa, y, za, xb, y, zb, xa, y, zb]]
    tiles = np.array(tiles, np.float32)
    counts, flags, ids, segs = R.overlap(flat, tiles, 8, True)
    assert (counts > 8).any() and (counts == 0).any(), "the tiling reaches neither a truncated tile nor an empty one"
    m = re.search(r"slice: y = (\S+), (\d+) tiles, (\d+) cut the mesh, (\d+) segments, (\d+) truncated", r.stdout)
    want = [2 * M * M, int((counts > 0).sum()), int((segs["kind"] == 1).sum()), int((counts > 8).sum())]
    assert m and [int(x) for x in m.groups()[1:]] == want, (r.stdout, want)
    m = re.search(r"touches: ([01])", r.stdout)
    assert m and int(m.group(1)) == int(flags[0]), r.stdout
    data = pgm.read_bytes()
    head = b"P5\n256 256\n255\n"
    assert data.startswith(head) and len(data) == len(head) + 256 * 256
    lit = np.frombuffer(data[len(head):], np.uint8).reshape(256, 256) == 255
    assert 100 < lit.sum() < 256 * 256 // 8, int(lit.sum())
    # every end of a segment lies in the cutting plane's height, to the rounding of an edge crossing
    ends = np.concatenate([segs["p"][segs["kind"] == 1], segs["q"][segs["kind"] == 1]])
    assert np.abs(ends[:, 1] - y).max() <= 4 * 2.0 ** -24 * 2.0, float(np.abs(ends[:, 1] - y).max())
