"""The box-overlap queries on the GPU (rt_overlap_boxes[_device]) against tests/overlap_ref.py, the NumPy binary32 yardstick that evaluates
every candidate of every box: every count, every byte and every id compared as BYTES.

Scenes (tests/multihit_scenes.py): three-sphere, cube, monkey, reference scenes 0 and 4, the two richest seeds of tests/random_scenes.py,
nine meshes of 1 to 9 triangles, a 3,000-triangle mesh read from global memory, soup6k on the hybrid and on the global placement - the
placement asserted from scene.info() - with 300 seeded boxes each (overlap_ref.query_boxes: half drawn from the scene's bounds, half from
the bounds of its triangles, a quarter of each with a face exactly on a vertex coordinate or a node-box plane, those of the second half
placed where that face decides).  Each scene and shape test first asserts, from the yardstick alone, that its boxes reach the walk: at
least ten of them meet some but not all of the meshes' triangles.  Every shape of RT_SHAPES is forced the way tests/test_gpu_shapes.py forces it, on the smallest
scene that reaches it.  k: 0, 1, 2, 3, 8; each output alone and all three together; the any-only mode against count > 0.  The yardstick's
answers are computed once per scene (at k = 8: the ids of a smaller k are their first columns) and shared.  Further: box counts around a
wave and past one chunk per resident wave, boxes that are not valid, a zero-extent box, a box holding the scene, an updated mesh, the
launch order on a sleeping stream and beside a multi-hit call, voxelize at 16^3, the refusals, host/example_voxelize.cpp.  Run with
-m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import multihit_scenes as S
import overlap_ref as R
from test_gpu_shapes import SHAPES, _id, commit_as, plan, spheres_beyond_lds

pytestmark = pytest.mark.gpu

N_BOXES = 300
KS = (0, 1, 2, 3, 8)
_REFS = {}
SEEDS = {"three_sphere": 1, "cube": 2, "monkey": 3, "reference_scene0": 4, "reference_scene4": 5, "random13": 6, "random15": 7, "tiny_meshes": 8,
         "soup3000": 9, "soup6k": 10, "spheres_beyond_lds": 11}


def objects_of(rt, name):
    if name == "spheres_beyond_lds":
        return rt.scenes.reference_scene4(num_spheres=spheres_beyond_lds(rt))[0]
    return S.objects_of(rt, name)


def reference(rt, models_dir, name, flat=None, seed=None, n=N_BOXES):
    """dict(flat, lo, hi, counts, any, ids) of the scene's seeded boxes: the yardstick's answers at k = 8, kept"""
    key = name if flat is None else (name, seed, n)
    if key not in _REFS:
        flat = flat if flat is not None else rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
        lo, hi = R.query_boxes(flat, SEEDS[name] if seed is None else seed, n)
        detail = {}
        counts, flags, ids = R.overlap(flat, lo, hi, 8, detail)
        in_mesh, mesh_tris = R.mesh_counts(flat, detail)
        _REFS[key] = {"flat": flat, "lo": lo, "hi": hi, "counts": counts, "any": flags, "ids": ids, "in_mesh": in_mesh, "mesh_tris": mesh_tris}
    return _REFS[key]


def reaches_the_walk(ref, name):
    """the boxes ask both answers, and on a scene with a mesh some box meets some but not all of the meshes' triangles - the walk of the
    tree is entered and prunes - and some box meets more than eight candidates where the scene has that many"""
    assert (ref["counts"] > 0).any() and (ref["counts"] == 0).any(), (name, "the boxes do not reach both answers")
    if ref["mesh_tris"] > 1:
        partial = (ref["in_mesh"] > 0) & (ref["in_mesh"] < ref["mesh_tris"])
        assert partial.sum() >= 10, (name, "fewer than ten boxes meet a part of the meshes", int(partial.sum()))
    if ref["mesh_tris"] > 50:
        assert (ref["counts"] > 8).any(), (name, "no box meets more than eight candidates")


def same(got, ref, k, what, rows=slice(None)):
    counts, ids = got
    assert counts.dtype == np.int32 and counts.tobytes() == ref["counts"][rows].tobytes(), (what, "counts differ at", np.nonzero(counts != ref["counts"][rows])[0][:5])
    want = np.ascontiguousarray(ref["ids"][rows][:, :k])
    assert ids.dtype == want.dtype and ids.shape == want.shape and ids.tobytes() == want.tobytes(), (what, "ids differ at", np.argwhere(ids != want)[:5].tolist())


def check_scene(rt, ctx, scene, ref, what, ks=KS):
    lo, hi = ref["lo"], ref["hi"]
    for k in ks:
        same(rt.overlap_boxes(scene, lo, hi, k), ref, k, "%s, k=%d" % (what, k))
    touch = rt.boxes_touch(scene, lo, hi)
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


# ---- each output alone and all three together -----------------------------------------------------------------------------------------
def test_each_output_alone_and_all_together(rt, ctx, models_dir):
    import torch
    name = "random13"
    ref = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    n = ref["lo"].shape[0]
    d_lo, d_hi = torch.from_numpy(ref["lo"]).to("cuda:0"), torch.from_numpy(ref["hi"]).to("cuda:0")
    fresh = lambda: (torch.full((n, 3, 8), 0xA5, dtype=torch.uint8, device="cuda:0"), torch.full((n,), -7, dtype=torch.int32, device="cuda:0"),
                     torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0"))
    want_ids = np.ascontiguousarray(ref["ids"][:, :3]).tobytes()
    for use in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
        ids, counts, flags = fresh()
        rt.overlap_boxes_device(scene, d_lo, d_hi, 3 if use[0] else 0, ids=ids if use[0] else None, counts=counts if use[1] else None, any=flags if use[2] else None)
        torch.cuda.synchronize()
        assert ids.cpu().numpy().tobytes() == (want_ids if use[0] else b"\xa5" * (n * 24)), use
        assert counts.cpu().numpy().tobytes() == (ref["counts"].tobytes() if use[1] else np.full(n, -7, np.int32).tobytes()), use
        assert flags.cpu().numpy().tobytes() == (ref["any"].tobytes() if use[2] else b"\xa5" * n), use
    # new tensors where none were passed; pointers with n
    counts, ids, flags = rt.overlap_boxes_device(scene, d_lo, d_hi, 2)
    torch.cuda.synchronize()
    assert flags is None and counts.cpu().numpy().tobytes() == ref["counts"].tobytes()
    assert ids.cpu().numpy().view(rt.OverlapId)[..., 0].tobytes() == np.ascontiguousarray(ref["ids"][:, :2]).tobytes()
    ids, counts, flags = fresh()
    rt.overlap_boxes_device(scene, d_lo.data_ptr(), d_hi.data_ptr(), 3, ids=ids.data_ptr(), counts=None, any=flags.data_ptr(), n=n)
    torch.cuda.synchronize()
    assert ids.cpu().numpy().tobytes() == want_ids and flags.cpu().numpy().tobytes() == ref["any"].tobytes()
    # ids at an address that is 8 but not 16 bytes aligned, with an even k: the 8-byte stores
    raw = torch.full((n * 2 * 8 + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    off = 8 if raw.data_ptr() % 16 == 0 else 0
    rt.overlap_boxes_device(scene, d_lo.data_ptr(), d_hi.data_ptr(), 2, ids=raw.data_ptr() + off, n=n)
    torch.cuda.synchronize()
    got = raw.cpu().numpy()
    assert got[off:off + n * 16].tobytes() == np.ascontiguousarray(ref["ids"][:, :2]).tobytes() and (got[:off] == 0xA5).all() and (got[off + n * 16:] == 0xA5).all()
    assert ctx.last_kernel_ms() > 0.0


# ---- counts around a wave and a chunk, and past one chunk per resident wave ------------------------------------------------------------
def test_box_counts(rt, ctx, models_dir):
    from test_gpu_refill import batch_size
    name = "monkey"
    ref = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    for k in (3, 0):
        for n in (1, 63, 64, 65):
            same(rt.overlap_boxes(scene, ref["lo"][:n], ref["hi"][:n], k), ref, k, "%s n=%d k=%d" % (name, n, k), slice(0, n))
    for n in (1, 63, 64, 65):
        assert np.array_equal(rt.boxes_touch(scene, ref["lo"][:n], ref["hi"][:n]), ref["counts"][:n] > 0), n
    counts, ids = rt.overlap_boxes(scene, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 4)
    assert ids.shape == (0, 4) and counts.shape == (0,)
    # more boxes than one chunk per resident wave: the refill path, every lane of every wave more than once
    n = batch_size()
    idx = np.random.default_rng(5).integers(0, ref["lo"].shape[0], n)
    lo, hi = np.ascontiguousarray(ref["lo"][idx]), np.ascontiguousarray(ref["hi"][idx])
    same(rt.overlap_boxes(scene, lo, hi, 3), ref, 3, "%s n=%d k=3" % (name, n), idx)
    same(rt.overlap_boxes(scene, lo, hi, 0), ref, 0, "%s n=%d k=0" % (name, n), idx)
    assert np.array_equal(rt.boxes_touch(scene, lo, hi), ref["counts"][idx] > 0), "any-only past one chunk per wave"


# ---- boxes that are not valid, a zero-extent box, a box that holds the scene -------------------------------------------------------------
def test_invalid_zero_extent_and_whole_scene_boxes(rt, ctx, models_dir):
    name = "random15"
    ref = reference(rt, models_dir, name)
    flat = ref["flat"]
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    _, _, tris, objects = R.sections(flat)
    slo, shi = R.scene_bounds(flat)
    # a record's own p0: v0 is then exactly zero, every projection of it is 0, which is neither above a radius of 0 nor below -0, and the
    # other two vertices lie on the other side of no axis alone - so the box overlaps that record whatever the rounding of the rest
    v = tris[tris.shape[0] // 2, 0:3]
    lo = np.array([slo - 1, slo - 1, slo - 1, slo - 1, slo - 1, v, slo - 1, [0, 0, 0]], np.float32)
    hi = np.array([shi + 1, shi + 1, shi + 1, shi + 1, shi + 1, v, shi + 1, [0, 0, 0]], np.float32)
    lo[1, 0] = np.nan
    hi[2, 2] = np.inf
    lo[3, 1] = -np.inf
    lo[4, 1], hi[4, 1] = hi[4, 1], lo[4, 1]
    counts, flags, ids = R.overlap(flat, lo, hi, 8)
    candidates = tris.shape[0] + int((objects["type"] == R.OBJ_SPHERE).sum())
    assert counts[0] == counts[6] == candidates and (counts[1:5] == 0).all() and counts[5] >= 1, counts
    got = rt.overlap_boxes(scene, lo, hi, 8)
    assert got[0].tobytes() == counts.tobytes() and got[1].tobytes() == ids.tobytes(), (got[0], counts)
    assert np.array_equal(rt.boxes_touch(scene, lo, hi), counts > 0)


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
    lo, hi = R.query_boxes(fresh_objs.debug_flatten(), 3, 400)
    before = rt.overlap_boxes(scene, lo, hi, 4)
    scene.update_mesh_device(1, torch.from_numpy(new).to("cuda:0"))
    after = rt.overlap_boxes(scene, lo, hi, 4)
    fresh = rt.overlap_boxes(ctx.commit(fresh_objs), lo, hi, 4)
    assert after[0].tobytes() == fresh[0].tobytes() and after[1].tobytes() == fresh[1].tobytes(), "updated against a fresh commit"
    counts, _, ids = R.overlap(scene.debug_read(), lo, hi, 4)
    assert after[0].tobytes() == counts.tobytes() and after[1].tobytes() == ids.tobytes(), "updated against the yardstick on the device's scene"
    assert before[0].tobytes() != after[0].tobytes()


# ---- the launch order: a sleeping stream, and the multi-hit kernel on a second stream ---------------------------------------------------
def test_boxes_produced_on_the_stream_just_ahead_of_the_call(rt, models_dir):
    """In the manner of tests/test_gpu_multihit.py: on a sleeping stream the boxes are copied into place, the call is queued, the answers
    are copied out - the host waits for nothing in between - and the answers are the yardstick's."""
    import torch
    name = "monkey"
    ref = reference(rt, models_dir, name)
    n, k = ref["lo"].shape[0], 4
    dev = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    src_lo, src_hi = torch.from_numpy(ref["lo"]).to(dev), torch.from_numpy(ref["hi"]).to(dev)
    buf_lo, buf_hi = torch.empty_like(src_lo), torch.empty_like(src_hi)
    ids = torch.empty((n, k, 8), dtype=torch.uint8, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    res_ids, res_cnt, res_flags = torch.empty_like(ids), torch.empty_like(cnt), torch.empty_like(flags)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rt.overlap_boxes_device(scene, src_lo, src_hi, k, ids=ids, counts=cnt, any=flags, stream=stream.cuda_stream)      # warm: the kernel is loaded, the stream has its queue
    torch.cuda.synchronize()
    buf_lo.fill_(float("nan"))
    buf_hi.fill_(float("nan"))
    ids.fill_(0xEE)
    cnt.fill_(-7)
    flags.fill_(0xEE)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(60000000)
        buf_lo.copy_(src_lo, non_blocking=True)
        buf_hi.copy_(src_hi, non_blocking=True)
        rt.overlap_boxes_device(scene, buf_lo, buf_hi, k, ids=ids, counts=cnt, any=flags, stream=stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        pending = not ev.query()
        res_ids.copy_(ids, non_blocking=True)
        res_cnt.copy_(cnt, non_blocking=True)
        res_flags.copy_(flags, non_blocking=True)
    torch.cuda.synchronize()
    assert pending, "the stream had run dry before the call returned: the window was not open"
    assert res_cnt.cpu().numpy().tobytes() == ref["counts"].tobytes() and res_flags.cpu().numpy().tobytes() == ref["any"].tobytes(), "queued behind the producer of its boxes"
    assert res_ids.cpu().numpy().tobytes() == np.ascontiguousarray(ref["ids"][:, :k]).tobytes(), "queued behind the producer of its boxes"


def test_beside_a_multi_hit_call_on_a_second_stream(rt, models_dir):
    """rt_overlap_boxes_device and rt_trace_rays_multi_device share a launcher and an argument type: queued back to back on two streams of
    one context, without a wait between them, both answer as their synchronised selves"""
    import torch
    name = "monkey"
    ref = reference(rt, models_dir, name)
    mh = S.reference(rt, models_dir, name)
    o, d = mh["o"][:1024], mh["d"][:1024]
    n, k = ref["lo"].shape[0], 3
    dev = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    want_hits, want_counts = rt.trace_rays_multi(c, scene, o, d, k)
    want_ov = rt.overlap_boxes(scene, ref["lo"], ref["hi"], k)
    same(want_ov, ref, k, "the synchronised call")
    d_lo, d_hi, d_o, d_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ref["lo"], ref["hi"], o, d))
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    ids = torch.full((n, k, 8), 0xEE, dtype=torch.uint8, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    hits = torch.full((o.shape[0], k, 48), 0xEE, dtype=torch.uint8, device=dev)
    hcnt = torch.full((o.shape[0],), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for _ in range(2):
        rt.overlap_boxes_device(scene, d_lo, d_hi, k, ids=ids, counts=cnt, stream=s1.cuda_stream)
        rt.trace_rays_multi_device(c, scene, d_o, d_d, k, hits=hits, counts=hcnt, stream=s2.cuda_stream)
        rt.overlap_boxes_device(scene, d_lo, d_hi, k, ids=ids, counts=cnt, stream=s1.cuda_stream)
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tobytes() == want_ov[0].tobytes() and ids.cpu().numpy().tobytes() == want_ov[1].tobytes(), "the overlap answers beside a multi-hit launch"
    assert hcnt.cpu().numpy().tobytes() == want_counts.tobytes() and hits.cpu().numpy().tobytes() == want_hits.tobytes(), "the multi-hit answers beside an overlap launch"


# ---- the voxeliser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "monkey"])
def test_voxelize(rt, ctx, models_dir, name):
    objs = objects_of(rt, name)
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    slo, shi = R.surface_bounds(flat)                                   # the mesh's own bounds: the scene stands on a sphere of radius 100
    pad = (shi - slo) * np.float32(0.07)
    lo, hi, shape = slo - pad, shi + pad, (16, 16, 16)
    cell_lo, cell_hi, centre = rt.voxel_boxes(lo, hi, shape)
    assert cell_lo.shape == (4096, 3) and np.array_equal(cell_lo.reshape(16, 16, 16, 3)[1:, :, :, 0], cell_hi.reshape(16, 16, 16, 3)[:-1, :, :, 0]), "neighbours share a face"
    assert np.array_equal(cell_lo[0], lo.astype(np.float32)) and np.array_equal(cell_hi[-1], hi.astype(np.float32))
    detail = {}
    surface_want = (R.overlap(flat, cell_lo, cell_hi, 0, detail)[0] > 0).reshape(shape)
    in_mesh, mesh_tris = R.mesh_counts(flat, detail)
    assert ((in_mesh > 0) & (in_mesh < mesh_tris)).sum() >= 50, (name, "the grid does not resolve the mesh")
    surface = rt.voxelize(scene, lo, hi, shape).cpu().numpy()
    assert surface.dtype == bool and np.array_equal(surface, surface_want), (name, int((surface != surface_want).sum()))
    assert surface.any() and not surface.all()
    inside = rt.contains_points(ctx, scene, centre).reshape(shape)
    solid = rt.voxelize(scene, lo, hi, shape, solid=True).cpu().numpy()
    assert np.array_equal(solid, surface_want | inside), (name, int((solid != (surface_want | inside)).sum()))
    mesh_object = int(np.nonzero(flat["objects"]["type"] == 5)[0][0])
    inside_mesh = rt.contains_points(ctx, scene, centre, object=mesh_object).reshape(shape)
    assert (solid & ~surface & inside_mesh).any(), (name, "no cell inside the mesh that its surface does not touch: the solid leg shows nothing")
    fast = rt.voxelize(scene, lo, hi, shape, solid=True, beta=2.0).cpu().numpy()
    assert np.array_equal(fast, surface_want | rt.contains_points(ctx, scene, centre, beta=2.0).reshape(shape)), name


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    name = "three_sphere"
    ref = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    before = rt.overlap_boxes(scene, ref["lo"], ref["hi"], 2)
    boxes = torch.zeros((4, 3), dtype=torch.float32, device="cuda:0")
    out = torch.full((4 * 2 * 8 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    cnt = torch.full((4,), -3, dtype=torch.int32, device="cuda:0")
    flags = torch.full((4,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert out.data_ptr() % 8 == 0
    p, h, c, a = C.c_void_p(boxes.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(flags.data_ptr())
    dev = L.rt_overlap_boxes_device
    bad = rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, p, -1, 2, h, c, a, None) == bad and dev(ctx._h, scene._h, p, p, (1 << 30) + 1, 2, h, c, a, None) == bad
    assert dev(ctx._h, scene._h, p, p, 4, -1, h, c, a, None) == bad and dev(ctx._h, scene._h, p, p, 4, 9, h, c, a, None) == bad
    assert dev(ctx._h, scene._h, None, p, 4, 2, h, c, a, None) == bad and dev(ctx._h, scene._h, p, None, 4, 2, h, c, a, None) == bad
    assert dev(ctx._h, scene._h, p, p, 4, 2, None, c, a, None) == bad and "null ids" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, p, 4, 2, C.c_void_p(out.data_ptr() + 4), c, a, None) == bad and "8-byte aligned" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, p, 4, 0, None, None, None, None) == bad and "no output" in ctx.last_error()
    assert dev(ctx._h, foreign._h, p, p, 4, 2, h, c, a, None) == bad and "another context" in ctx.last_error()
    assert dev(None, scene._h, p, p, 4, 2, h, c, a, None) == bad and dev(ctx._h, None, p, p, 4, 2, h, c, a, None) == bad
    assert dev(ctx._h, scene._h, None, None, 0, 2, None, None, None, None) == rt.RT_OK
    crowd = [("sphere", (0.01 * (i % 70), 0.01 * (i // 70), 2.0), 0.004, ("standard", (0.5, 0.5, 0.5), 0.0)) for i in range(4097)]
    crowded = ctx.commit(rt.SceneObjects(crowd, models_dir))
    assert dev(ctx._h, crowded._h, p, p, 4, 2, h, c, a, None) == bad and "too many objects" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x77).all()) and bool((cnt == -3).all()) and bool((flags == 0x77).all()), "a refused call wrote"
    with pytest.raises(ValueError):
        rt.overlap_boxes(scene, np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32), 9)
    with pytest.raises(ValueError):
        rt.overlap_boxes_device(scene, boxes.double(), boxes, 2)
    after = rt.overlap_boxes(scene, ref["lo"], ref["hi"], 2)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes(), "a call behind the refusals answers as before"
    same(after, ref, 2, "behind the refusals")


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_example_voxelize_program(rt, ctx, models_dir, tmp_path):
    """host/example_voxelize.cpp (Renderer::touches, Renderer::contains, Renderer::overlap_boxes of host/raytracer.hpp): it builds, its cell
    counts and its probe are the yardstick's for the same scene and cells, and the PGM holds the slice at half the grid's depth"""
    import re
    import subprocess
    exe = rt.build.build_voxelize_example()
    N = 12
    pgm = tmp_path / "voxels.pgm"
    r = subprocess.run([exe, models_dir, str(N), str(pgm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    objs = [("obj", "low_poly_monkey.obj", [("enlarge", 0.3), ("rotate", 0, 2.3, 0), ("translate", 0.1, -0.1, 1.6)], ("standard", (1, 1, 1), 0.0))]
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    side = 1.3
    corner = np.array([0.1 - side / 2, -0.1 - side / 2, 1.6 - side / 2])
    edges = [(corner[a] + side * np.arange(N + 1, dtype=np.float64) / N).astype(np.float32) for a in range(3)]
    lo = np.stack(np.meshgrid(*[e[:-1] for e in edges], indexing="ij"), axis=-1).reshape(-1, 3)
    hi = np.stack(np.meshgrid(*[e[1:] for e in edges], indexing="ij"), axis=-1).reshape(-1, 3)
    counts, _, ids = R.overlap(flat, lo, hi, 8)
    surface = counts > 0
    inside = rt.contains_points(ctx, ctx.commit(rt.SceneObjects(objs, models_dir)), (lo + hi) * np.float32(0.5))
    m = re.search(r"grid: (\d+)\^3 cells, (\d+) surface, (\d+) solid", r.stdout)
    assert m and [int(x) for x in m.groups()] == [N, int(surface.sum()), int((surface | inside).sum())], (r.stdout, int(surface.sum()), int((surface | inside).sum()))
    first = int(np.argmax(surface))
    m = re.search(r"probe: cell (\d+) (\d+) (\d+) meets (\d+) triangles, the lowest((?: -?\d+)*)", r.stdout)
    assert m and [int(x) for x in m.groups()[:4]] == [first // (N * N), first // N % N, first % N, int(counts[first])], (r.stdout, first, counts[first])
    assert [int(x) for x in m.group(5).split()] == ids["triangle"][first][:min(8, counts[first])].tolist(), (r.stdout, ids[first])
    data = pgm.read_bytes()
    head = b"P5\n%d %d\n255\n" % (N, N)
    s, i = surface.reshape(N, N, N)[:, :, N // 2], inside.reshape(N, N, N)[:, :, N // 2]
    want = bytes(255 if s[x, y] else 128 if i[x, y] else 0 for y in range(N - 1, -1, -1) for x in range(N))
    assert data.startswith(head) and data[len(head):] == want
