"""The fast winding numbers on the GPU (rt_winding_numbers_fast[_device], rt_signed_distance_fast[_device]) against tests/winding_fast_ref.py,
the NumPy binary32 yardstick that restates the moments and the walk over the cluster trees Scene.debug_winding_tree() reports: every output
compared as BYTES (floats as uint32).  Nothing is skipped and nothing is tolerated - how far the fast answer lies from the exact one is the
CPU tests' business (tests/test_winding_fast_ref.py).

Scenes: cube, monkey, reference_scene0 with every object index, a two-mesh scene of tests/random_scenes.py, meshes of 1, 8 and 9 triangles
(one leaf, a full leaf, the first split), soup6k and sphere50k (4,096 points).  Points: test_gpu_winding's (uniform in twice the bounds,
vertices, edge midpoints, centroids, 2^20, signed zeros, points that are not finite) and cluster centres.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import nearest_ref as NR
import winding_fast_ref as F
import winding_ref as W
from random_scenes import num_meshes
from test_gpu_winding import BAD, objects_of, points_of, same

pytestmark = pytest.mark.gpu

INF = float("inf")
_REFS = {}


def tiny_mesh(n, seed):
    """n random triangles in the unit cube around (0, 0, 2), as a scene description"""
    rng = np.random.default_rng(seed)
    tris = (rng.uniform(-0.5, 0.5, (n, 3, 3)) + np.array([0, 0, 2.0])).astype(np.float32).reshape(n, 9)
    return [("mesh", tris, ("standard", (1, 1, 1), 0.0))]


def objects_for(rt, name):
    if name.startswith("tiny"):
        return tiny_mesh(int(name[4:]), 40 + int(name[4:]))
    return objects_of(rt, name)


def committed(rt, ctx, models_dir, name):
    """(scene, flat, tree as the device holds it, points) - the flattened scene and the points once per scene name"""
    scene = ctx.commit(rt.SceneObjects(objects_for(rt, name), models_dir))
    if name not in _REFS:
        flat = rt.SceneObjects(objects_for(rt, name), models_dir).debug_flatten()
        if name == "sphere50k":
            pts = F.uniform_points(flat, 5, 4096)
        elif name == "soup6k":
            pts = points_of(flat, name, 130 - points_of(flat, name, 0, 8).shape[0], 8)
        else:
            pts = points_of(flat, name, 300)
        _REFS[name] = (flat, pts)
    flat, pts = _REFS[name]
    return scene, flat, scene.debug_winding_tree(), pts


def check_outputs(rt, ctx, scene, pts, want, obj, beta, what):
    """winding only, inside only, and both"""
    same(rt.winding_numbers_fast(ctx, scene, pts, obj, beta), want, what + ", winding only")
    same(rt.contains_points(ctx, scene, pts, obj, beta=beta).astype(np.uint8), W.inside(want), what + ", inside only")
    w, flags = rt.winding_numbers_fast(ctx, scene, pts, obj, beta, inside=True)
    same(w, want, what + ", both: winding")
    same(flags, W.inside(want), what + ", both: inside")


def moments_equal(flat, tree, what):
    want = F.moments(flat, tree)
    same(tree["moments"].view(np.uint32), want.view(np.uint32), what + ": the device's moments against the yardstick's")
    return want


@pytest.mark.parametrize("name", ["cube", "monkey", "reference_scene0", "random6", "random14", "tiny1", "tiny8", "tiny9"])
def test_solids_equal_the_yardstick(rt, ctx, models_dir, name):
    if name.startswith("random"):
        assert num_meshes(objects_for(rt, name)) == 2, name
    scene, flat, tree, pts = committed(rt, ctx, models_dir, name)
    F.check_topology(flat, tree)
    mom = moments_equal(flat, tree, name)
    centres = mom[:: max(1, mom.shape[0] // 16), 0:3]
    pts = np.concatenate([pts, centres]).astype(np.float32)
    for beta in (1.0, 2.0, 4.0, INF):
        want = F.winding(flat, tree, pts, beta, mom=mom)
        check_outputs(rt, ctx, scene, pts, want, rt.WINDING_SOLIDS, beta, "%s beta=%g" % (name, beta))
        finite = np.isfinite(pts).all(axis=1)
        assert (want[~finite].view(np.uint32) == 0x7FC00000).all() and not np.isnan(want[finite]).any()
    assert ctx.last_kernel_ms() > 0.0
    if name == "monkey":
        exact = rt.winding_numbers(ctx, scene, pts)
        fast = rt.winding_numbers_fast(ctx, scene, pts, beta=2.0)
        assert fast.tobytes() != exact.tobytes() and np.nanmax(np.abs(fast - exact)) < 0.1, "beta = 2 approximates: near the exact answer, not its bytes"


def test_every_object_of_reference_scene0(rt, ctx, models_dir):
    scene, flat, tree, pts = committed(rt, ctx, models_dir, "reference_scene0")
    kinds = set()
    for i in range(len(flat["objects"])):
        kinds.add(int(flat["objects"][i]["type"]))
        want = F.winding(flat, tree, pts, 2.0, i)
        check_outputs(rt, ctx, scene, pts, want, i, 2.0, "reference_scene0 object %d" % i)
        if int(flat["objects"][i]["type"]) != W.OBJ_MESH:
            same(want, W.winding(flat, pts, i), "an object that is no mesh answers exactly")
    assert kinds >= {W.OBJ_SPHERE, W.OBJ_QUAD, W.OBJ_ONE_WAY_QUAD, W.OBJ_CUBOID, W.OBJ_MESH}, kinds


def test_soup6k(rt, ctx, models_dir):
    scene, flat, tree, pts = committed(rt, ctx, models_dir, "soup6k")
    assert pts.shape[0] == 130 and flat["num_triangles"] == 6000
    mom = moments_equal(flat, tree, "soup6k")
    for beta in (2.0, INF):
        check_outputs(rt, ctx, scene, pts, F.winding(flat, tree, pts, beta, mom=mom), rt.WINDING_SOLIDS, beta, "soup6k beta=%g" % beta)


def test_sphere50k(rt, ctx, models_dir):
    scene, flat, tree, pts = committed(rt, ctx, models_dir, "sphere50k")
    assert pts.shape[0] == 4096 and flat["num_triangles"] == 50880
    F.check_topology(flat, tree)
    mom = moments_equal(flat, tree, "sphere50k")
    same(rt.winding_numbers_fast(ctx, scene, pts, beta=2.0), F.winding(flat, tree, pts, 2.0, mom=mom), "sphere50k beta=2")
    for beta in (1.0, 4.0):
        same(rt.winding_numbers_fast(ctx, scene, pts[:512], beta=beta), F.winding(flat, tree, pts[:512], beta, mom=mom), "sphere50k beta=%g" % beta)


def test_point_counts(rt, ctx, models_dir):
    scene, flat, tree, pts = committed(rt, ctx, models_dir, "monkey")
    want = F.winding(flat, tree, pts, 2.0)
    for n in (0, 1, 63, 64, 65, 200):
        check_outputs(rt, ctx, scene, pts[:n], want[:n], rt.WINDING_SOLIDS, 2.0, "monkey n=%d" % n)


def test_a_scene_without_a_mesh_answers_the_exact_bytes(rt, ctx, models_dir):
    import torch
    scene, flat, tree, pts = committed(rt, ctx, models_dir, "three_sphere")
    assert tree["skip"].shape[0] == 0
    d_pts = torch.from_numpy(pts).to("cuda:0")
    exact, _ = rt.winding_numbers_device(ctx, scene, d_pts)
    fast, _ = rt.winding_numbers_fast_device(ctx, scene, d_pts, beta=2.0)
    same(fast.cpu().numpy(), exact.cpu().numpy(), "three_sphere: fast against winding_numbers_device")
    same(fast.cpu().numpy(), W.winding(flat, pts), "three_sphere: fast against the exact yardstick")


# ---- the signed distance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["monkey", "reference_scene0"])
def test_signed_distance_fast(rt, ctx, models_dir, name):
    import torch
    scene, flat, tree, pts = committed(rt, ctx, models_dir, name)
    w = F.winding(flat, tree, pts, 2.0)
    free = NR.nearest(flat, pts)
    sdf, rec = rt.signed_distance_fast(ctx, scene, pts, beta=2.0)
    same(rec, free, name + ": the records, no limits")
    same(sdf, W.sdf(w, free["distance"]), name + ": sdf, no limits")
    lim = free["distance"].copy()
    k = np.arange(lim.shape[0]) % 4
    lim[k == 1] = np.nextafter(lim[k == 1], np.float32(0))
    lim[k == 2] = np.nextafter(lim[k == 2], np.float32(np.inf))
    lim[k == 3] = np.nan
    limited = NR.nearest(flat, pts, lim)
    sdf_l, rec_l = rt.signed_distance_fast(ctx, scene, pts, lim, beta=2.0)
    same(rec_l, limited, name + ": the records under limits")
    same(sdf_l, W.sdf(w, limited["distance"]), name + ": sdf under limits")
    d_pts, d_lim = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(lim).to("cuda:0")
    out = torch.full((pts.shape[0], 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_sdf, d_rec = rt.signed_distance_fast_device(ctx, scene, d_pts, d_lim, beta=2.0, records=out)
    assert d_rec is out
    same(d_sdf.cpu().numpy(), W.sdf(w, limited["distance"]), name + ": device form, sdf")
    same(out.cpu().numpy().view(rt.NearestRecord).reshape(-1), limited, name + ": device form, records")
    d_sdf2, none = rt.signed_distance_fast_device(ctx, scene, d_pts, beta=2.0)
    assert none is None
    same(d_sdf2.cpu().numpy(), W.sdf(w, free["distance"]), name + ": device form, the context's record buffer")


def test_signed_distance_grid_with_beta(rt, ctx, models_dir):
    scene, flat, tree, _ = committed(rt, ctx, models_dir, "monkey")
    tris = NR.sections(flat)[2]
    lo, hi = tris[:, 0:3].min(axis=0), tris[:, 0:3].max(axis=0)
    shape = (5, 4, 3)
    sdf, rec = rt.signed_distance_grid(scene, lo, hi, shape, beta=3.0)
    grid = rt.query._lattice(scene, lo, hi, shape).cpu().numpy()
    want = NR.nearest(flat, grid)
    same(sdf.cpu().numpy().reshape(-1), W.sdf(F.winding(flat, tree, grid, 3.0), want["distance"]), "signed_distance_grid(beta=3)")


# ---- a scene updated on the device -------------------------------------------------------------------------------------------------------
def bent_monkey(rt, models_dir, amount):
    import os
    objs = objects_of(rt, "monkey")
    mesh = rt.ObjFileMesh(os.path.join(models_dir, objs[0][1]))
    for t in objs[0][2]:
        getattr(mesh, t[0])(*t[1:])
    tris = mesh.triangles().reshape(-1, 3, 3).astype(np.float32)
    bent = tris.copy()
    bent[:, :, 0] = tris[:, :, 0] + np.float32(amount) * tris[:, :, 1] * tris[:, :, 1]
    return bent.reshape(-1, 9)


def test_after_update_mesh_device(rt, ctx, models_dir):
    """the monkey bent: the topology stays, the device's moments are the yardstick's refit of the OLD topology over the NEW vertices, and the
    answers follow; a second update is followed by a query alone, whose refit runs inside the query's launch"""
    import torch
    scene, flat, tree0, pts = committed(rt, ctx, models_dir, "monkey")
    before = rt.winding_numbers_fast(ctx, scene, pts, beta=2.0)
    same(before, F.winding(flat, tree0, pts, 2.0), "before the update")
    scene.update_mesh_device(0, torch.from_numpy(bent_monkey(rt, models_dir, 0.25)).to("cuda:0"))
    tree1, read1 = scene.debug_winding_tree(), scene.debug_read()
    for key in ("skip", "first", "count", "order", "object_range"):
        assert (tree1[key] == tree0[key]).all(), key + " changed with the update"
    F.check_topology(read1, tree1)
    mom1 = moments_equal(read1, tree1, "after the update")
    assert mom1.tobytes() != tree0["moments"].tobytes()
    after = rt.winding_numbers_fast(ctx, scene, pts, beta=2.0)
    same(after, F.winding(read1, tree1, pts, 2.0, mom=mom1), "updated, against the yardstick over what is on the device")
    assert before.tobytes() != after.tobytes()
    # the second update, then the query at once: its refit is queued ahead of it
    scene.update_mesh_device(0, torch.from_numpy(bent_monkey(rt, models_dir, -0.4)).to("cuda:0"))
    again = rt.winding_numbers_fast(ctx, scene, pts, beta=2.0)
    tree2, read2 = scene.debug_winding_tree(), scene.debug_read()
    assert (tree2["skip"] == tree0["skip"]).all() and (tree2["order"] == tree0["order"]).all()
    mom2 = moments_equal(read2, tree2, "after the second update")
    same(again, F.winding(read2, tree2, pts, 2.0, mom=mom2), "the query right behind the second update")
    assert again.tobytes() != after.tobytes()
    sdf, rec = rt.signed_distance_fast(ctx, scene, pts, beta=2.0)
    near = NR.nearest(read2, pts)
    same(rec, near, "updated: the records")
    same(sdf, W.sdf(again, near["distance"]), "updated: sdf")


def test_update_query_and_consumer_on_a_sleeping_stream(rt, models_dir):
    """In the manner of tests/test_gpu_streams.py: on a sleeping stream the vertices are updated, the fast query (with its refit) is queued and
    the answers are copied out - the host waits for nothing in between - and the answers are those of synchronised calls on a fresh context."""
    import torch
    dev = torch.device("cuda:0")
    bent = bent_monkey(rt, models_dir, 0.25)
    fresh = rt.Context(0)
    fscene = fresh.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir))
    flat = rt.SceneObjects(objects_of(rt, "monkey"), models_dir).debug_flatten()
    pts = points_of(flat, "monkey", 300)
    rt.winding_numbers_fast(fresh, fscene, pts, beta=2.0)
    fscene.update_mesh(0, bent)
    want = rt.winding_numbers_fast(fresh, fscene, pts, beta=2.0)
    tree, read = fscene.debug_winding_tree(), fscene.debug_read()
    same(want, F.winding(read, tree, pts, 2.0), "the synchronised calls")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir))
    src, d_bent = torch.from_numpy(pts).to(dev), torch.from_numpy(bent).to(dev)
    d_tris = torch.empty_like(d_bent)
    out, res = torch.empty((pts.shape[0],), dtype=torch.float32, device=dev), torch.empty((pts.shape[0],), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rt.winding_numbers_fast_device(c, scene, src, beta=2.0, winding=out, stream=stream.cuda_stream)      # warm: kernels loaded, trees built
        d_tris.copy_(torch.from_numpy(bent_monkey(rt, models_dir, 0.0)).to(dev))
        scene.update_mesh_device(0, d_tris, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    out.fill_(123.0)
    res.fill_(123.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(60000000)
        d_tris.copy_(d_bent, non_blocking=True)
        scene.update_mesh_device(0, d_tris, stream=stream.cuda_stream)
        rt.winding_numbers_fast_device(c, scene, src, beta=2.0, winding=out, stream=stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        pending = not ev.query()
        res.copy_(out, non_blocking=True)
    torch.cuda.synchronize()
    assert pending, "the stream had run dry before the calls returned: the window was not open"
    same(res.cpu().numpy(), want, "fast winding numbers queued behind the update of their mesh")


def test_a_fast_and_a_nearest_call_on_two_streams(rt, models_dir):
    """one context, two streams, back to back: both use the context's point counter, so the second is ordered behind the first"""
    import torch
    dev = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir))
    flat = rt.SceneObjects(objects_of(rt, "monkey"), models_dir).debug_flatten()
    pts = points_of(flat, "monkey", 300)
    want = F.winding(flat, scene.debug_winding_tree(), pts, 2.0)
    want_near = NR.nearest(flat, pts)
    d_pts = torch.from_numpy(pts).to(dev)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for first in ("winding", "nearest"):
        w = torch.full((pts.shape[0],), 9.0, dtype=torch.float32, device=dev)
        rec = torch.full((pts.shape[0], 32), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        calls = {"winding": lambda s: rt.winding_numbers_fast_device(c, scene, d_pts, beta=2.0, winding=w, stream=s.cuda_stream),
                 "nearest": lambda s: rt.nearest_points_device(c, scene, d_pts, out=rec, stream=s.cuda_stream)}
        second = "nearest" if first == "winding" else "winding"
        calls[first](s1)
        calls[second](s2)
        torch.cuda.synchronize()
        same(w.cpu().numpy(), want, "fast winding numbers, %s first" % first)
        same(rec.cpu().numpy().view(rt.NearestRecord).reshape(-1), want_near, "nearest records, %s first" % first)


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_answer_alone(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    scene, flat, tree, pts_all = committed(rt, ctx, models_dir, "reference_scene0")
    n = 70
    pts_h = pts_all[:n]
    want = F.winding(flat, tree, pts_h, 2.0)
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objects_of(rt, "three_sphere"), models_dir))
    pts = torch.from_numpy(pts_h).to("cuda:0")
    w = torch.full((n,), 5.0, dtype=torch.float32, device="cuda:0")
    flags = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda:0")
    rec = torch.full((n * 32 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p, pw, pf, pr = (C.c_void_p(t.data_ptr()) for t in (pts, w, flags, rec))
    dev, S, B = L.rt_winding_numbers_fast_device, rt.WINDING_SOLIDS, 2.0
    n_obj = len(flat["objects"])
    for bad_beta in (0.0, -1.0, float("nan"), -INF):
        assert dev(ctx._h, scene._h, p, n, S, bad_beta, pw, pf, None) == rt.RT_ERR_INVALID and "beta" in ctx.last_error(), bad_beta
    assert dev(ctx._h, scene._h, p, -1, S, B, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, (1 << 30) + 1, S, B, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, None, n, S, B, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, n, S, B, None, None, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, n, n_obj, B, pw, pf, None) == rt.RT_ERR_INVALID and "object" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, n, -2, B, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, foreign._h, p, n, S, B, pw, pf, None) == rt.RT_ERR_INVALID and "another context" in ctx.last_error()
    assert dev(None, scene._h, p, n, S, B, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, None, p, n, S, B, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, None, 0, S, B, None, None, None) == rt.RT_OK
    sd = L.rt_signed_distance_fast_device
    assert sd(ctx._h, scene._h, p, None, n, 0.0, pr, pw, None) == rt.RT_ERR_INVALID and "beta" in ctx.last_error()
    assert sd(ctx._h, scene._h, p, None, -1, B, pr, pw, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, None, None, n, B, pr, pw, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, p, None, n, B, pr, None, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, p, None, n, B, C.c_void_p(rec.data_ptr() + 4), pw, None) == rt.RT_ERR_INVALID and "16-byte aligned" in ctx.last_error()
    assert sd(ctx._h, foreign._h, p, None, n, B, pr, pw, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, None, None, 0, B, None, None, None) == rt.RT_OK
    fp = C.POINTER(C.c_float)
    host_w = np.zeros(n, np.float32)
    assert L.rt_winding_numbers_fast(ctx._h, scene._h, pts_h.ctypes.data_as(fp), n, n_obj, B, host_w.ctypes.data_as(fp), None) == rt.RT_ERR_INVALID
    assert L.rt_winding_numbers_fast(ctx._h, scene._h, pts_h.ctypes.data_as(fp), n, S, 0.0, host_w.ctypes.data_as(fp), None) == rt.RT_ERR_INVALID
    assert L.rt_signed_distance_fast(ctx._h, scene._h, pts_h.ctypes.data_as(fp), None, n, B, None, None) == rt.RT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((w == 5.0).all()) and bool((flags == 0x77).all()) and bool((rec == 0x77).all()), "a refused call wrote answers"
    rt.winding_numbers_fast_device(ctx, scene, pts, beta=2.0, winding=w, inside=flags)
    same(w.cpu().numpy(), want, "the call after the refusals: winding")
    same(flags.cpu().numpy(), W.inside(want), "the call after the refusals: inside")
    assert abs(rt.WINDING_BETA_DEFAULT - 2.0) == 0 and rt.WINDING_LEAF_TRIS == 8
