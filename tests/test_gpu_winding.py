"""The winding-number queries on the GPU (rt_winding_numbers[_device], rt_signed_distance[_device]) against tests/winding_ref.py, the NumPy
binary32 yardstick that sums every record of every point in the header's order: every output compared as BYTES (floats as uint32).  Nothing
is skipped and nothing is tolerated.

Scenes: cube (12 triangles, every one a quad half: the flip bytes decide), monkey, reference_scene0 (quads, a one-way quad, a cuboid, a mesh,
a sphere) with every object index, three_sphere (no triangle), two seeds of tests/random_scenes.py that hold two meshes, soup6k with 130
points (the global placement and the long loop).  Points (winding_ref.query_points): uniform in twice the bounds, vertices, edge midpoints and
centroids of sampled triangles - so on-vertex, on-edge and in-plane points -, sphere centres, 2^20, signed zeros, and points that are not
finite.  The yardstick's answers are computed once per scene and shared.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import nearest_ref as NR
import winding_ref as W
from random_scenes import num_meshes, random_scene
from test_gpu_shapes import commit_as

pytestmark = pytest.mark.gpu

TWO_MESH_SEEDS = (6, 14)
SCENES = ["cube", "monkey", "reference_scene0", "three_sphere"] + ["random%d" % s for s in TWO_MESH_SEEDS]
BAD = np.array([[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
_REFS = {}


def objects_of(rt, name):
    if name.startswith("random"):
        return random_scene(int(name[6:]))[0]
    return rt.scenes.CONFIG_SCENES[name]()[0]


def points_of(flat, name, n_uniform, n_sample=40):
    """the surface, far and zero points first, then the uniform ones, then the points that are not finite"""
    q = W.query_points(flat, sum(name.encode()), n_uniform, n_sample)
    return np.concatenate([q[n_uniform:], q[:n_uniform], BAD]).astype(np.float32)


def reference(rt, models_dir, name):
    """(flat, points, the solids' winding numbers) of a scene, from the yardstick alone"""
    if name not in _REFS:
        flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
        if name == "soup6k":            # 130 points in all: the long loop stays within the yardstick's seconds
            pts = points_of(flat, name, 130 - points_of(flat, name, 0, 8).shape[0], 8)
        else:
            pts = points_of(flat, name, 400)
        _REFS[name] = (flat, pts, W.winding(flat, pts))
    return _REFS[name]


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.shape[0] == 0:
        return
    a, b = got.view(np.uint8).reshape(got.shape[0], -1), want.view(np.uint8).reshape(want.shape[0], -1)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, (what, "%d of %d differ, first at %s: got %s want %s" % (bad.size, got.shape[0], bad[:5], got[bad[:5]], want[bad[:5]]))


def check_outputs(rt, ctx, scene, pts, want, obj, what):
    """d_winding only, d_inside only, and both"""
    same(rt.winding_numbers(ctx, scene, pts, obj), want, what + ", winding only")
    same(rt.contains_points(ctx, scene, pts, obj).astype(np.uint8), W.inside(want), what + ", inside only")
    w, flags = rt.winding_numbers(ctx, scene, pts, obj, inside=True)
    same(w, want, what + ", both: winding")
    same(flags, W.inside(want), what + ", both: inside")


@pytest.mark.parametrize("name", SCENES)
def test_solids_equal_the_yardstick(rt, ctx, models_dir, name):
    objs = objects_of(rt, name)
    if name.startswith("random"):
        assert num_meshes(objs) == 2, name
    flat, pts, want = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    check_outputs(rt, ctx, scene, pts, want, rt.WINDING_SOLIDS, name)
    assert ctx.last_kernel_ms() > 0.0
    finite = np.isfinite(pts).all(axis=1)
    assert np.isnan(want[~finite]).all() and (want[~finite].view(np.uint32) == 0x7FC00000).all() and not np.isnan(want[finite]).any()
    if name == "cube":
        centre = np.array([NR.sections(flat)[2][:, 0:3].min(axis=0) / 2 + NR.sections(flat)[2][:, 0:3].max(axis=0) / 2], np.float32)
        assert flat["tri_flip"].sum() == 6 and abs(abs(float(rt.winding_numbers(ctx, scene, centre)[0])) - 1.0) < 1e-5


def test_every_object_of_reference_scene0(rt, ctx, models_dir):
    flat, pts, _ = reference(rt, models_dir, "reference_scene0")
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, "reference_scene0"), models_dir))
    kinds = set()
    for i in range(len(flat["objects"])):
        kinds.add(int(flat["objects"][i]["type"]))
        check_outputs(rt, ctx, scene, pts, W.winding(flat, pts, i), i, "reference_scene0 object %d" % i)
    assert kinds >= {W.OBJ_SPHERE, W.OBJ_QUAD, W.OBJ_ONE_WAY_QUAD, W.OBJ_CUBOID, W.OBJ_MESH}, kinds


def test_soup6k_from_global_memory(rt, ctx, models_dir, monkeypatch):
    scene = commit_as(rt, ctx, monkeypatch, objects_of(rt, "soup6k"), models_dir, {"RT_AMD_SCENE_MODE": "0"})
    assert scene.info()["scene_in_lds"] == 0, scene.info()
    flat, pts, want = reference(rt, models_dir, "soup6k")
    assert pts.shape[0] == 130 and flat["num_triangles"] == 6000
    check_outputs(rt, ctx, scene, pts, want, rt.WINDING_SOLIDS, "soup6k")


@pytest.mark.parametrize("name", ["monkey", "reference_scene0"])
def test_point_counts(rt, ctx, models_dir, name):
    flat, pts, want = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    for n in (0, 1, 63, 64, 65, 257):
        check_outputs(rt, ctx, scene, pts[:n], want[:n], rt.WINDING_SOLIDS, "%s n=%d" % (name, n))


# ---- the signed distance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "monkey", "reference_scene0", "three_sphere", "random14"])
def test_signed_distance(rt, ctx, models_dir, name):
    import torch
    flat, pts, w = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    free = NR.nearest(flat, pts)
    sdf, rec = rt.signed_distance(ctx, scene, pts)
    same(rec, free, name + ": the records, no limits")
    same(sdf, W.sdf(w, free["distance"]), name + ": sdf, no limits")
    finite = np.isfinite(pts).all(axis=1)
    assert (sdf[finite] < 0).any() and (sdf[finite] > 0).any() and (sdf[~finite] == rt.HIT_MISS_T).all(), name
    # limits: per point in turn the distance itself, one ulp down (a miss: +-HIT_MISS_T), one ulp up, a NaN
    lim = free["distance"].copy()
    k = np.arange(lim.shape[0]) % 4
    lim[k == 1] = np.nextafter(lim[k == 1], np.float32(0))
    lim[k == 2] = np.nextafter(lim[k == 2], np.float32(np.inf))
    lim[k == 3] = np.nan
    limited = NR.nearest(flat, pts, lim)
    sdf_l, rec_l = rt.signed_distance(ctx, scene, pts, lim)
    same(rec_l, limited, name + ": the records under limits")
    same(sdf_l, W.sdf(w, limited["distance"]), name + ": sdf under limits")
    assert (sdf_l == -rt.HIT_MISS_T).any() or not (W.inside(w) == 1).any(), name
    # the device form: the caller's record buffer, and none (the context's)
    d_pts, d_lim = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(lim).to("cuda:0")
    out = torch.full((pts.shape[0], 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_sdf, d_rec = rt.signed_distance_device(ctx, scene, d_pts, d_lim, records=out)
    assert d_rec is out
    same(d_sdf.cpu().numpy(), W.sdf(w, limited["distance"]), name + ": device form, sdf")
    same(out.cpu().numpy().view(rt.NearestRecord).reshape(-1), limited, name + ": device form, records")
    d_sdf2, none = rt.signed_distance_device(ctx, scene, d_pts)
    assert none is None
    same(d_sdf2.cpu().numpy(), W.sdf(w, free["distance"]), name + ": device form, the context's record buffer")


def test_signed_distance_grid(rt, ctx, models_dir):
    import torch
    flat, _, _ = reference(rt, models_dir, "monkey")
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir))
    tris = NR.sections(flat)[2]
    lo, hi = tris[:, 0:3].min(axis=0), tris[:, 0:3].max(axis=0)
    shape = (7, 6, 5)
    sdf, rec = rt.signed_distance_grid(scene, lo, hi, shape)
    axes = [torch.linspace(float(lo[k]), float(hi[k]), shape[k], dtype=torch.float32).numpy() for k in range(3)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    want = NR.nearest(flat, grid)
    same(rec.cpu().numpy().view(rt.NearestRecord).reshape(-1), want, "signed_distance_grid's records")
    assert sdf.shape == shape
    same(sdf.cpu().numpy().reshape(-1), W.sdf(W.winding(flat, grid), want["distance"]), "signed_distance_grid's field")


# ---- a scene updated on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "monkey"])
def test_after_update_mesh_device(rt, ctx, models_dir, name):
    """the mesh's vertices bent (x += 0.25 y^2, the same map for every vertex, so a closed mesh stays closed): the updated scene answers like
    the yardstick over what is on the device, flip bytes included, and like a fresh commit of the bent mesh"""
    import torch
    objs = objects_of(rt, name)
    mesh = rt.ObjFileMesh(__import__("os").path.join(models_dir, objs[0][1]))
    for t in objs[0][2]:
        getattr(mesh, t[0])(*t[1:])
    tris = mesh.triangles().reshape(-1, 3, 3).astype(np.float32)
    bent = tris.copy()
    bent[:, :, 0] = tris[:, :, 0] + np.float32(0.25) * tris[:, :, 1] * tris[:, :, 1]
    bent = bent.reshape(-1, 9)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    flat0 = rt.SceneObjects(objs, models_dir).debug_flatten()
    assert int(flat0["objects"][0]["type"]) == W.OBJ_MESH and bent.shape[0] == W.object_records(flat0, 0)[1]
    _, pts, before_want = reference(rt, models_dir, name)
    before = rt.winding_numbers(ctx, scene, pts)
    same(before, before_want, name + " before the update")
    scene.update_mesh_device(0, torch.from_numpy(bent).to("cuda:0"))
    after = rt.winding_numbers(ctx, scene, pts)
    read = scene.debug_read()
    same(after, W.winding(read, pts), name + " updated, against the yardstick over what is on the device")
    assert read["tri_flip"].sum() == flat0["tri_flip"].sum() and before.tobytes() != after.tobytes()
    corners = NR.sections(read)[2]
    first, end, _ = W.object_records(read, 0)
    centre = np.array([(corners[first:end, 0:3].min(axis=0) + corners[first:end, 0:3].max(axis=0)) / np.float32(2)], np.float32)
    assert abs(float(rt.winding_numbers(ctx, scene, centre, 0)[0])) >= 0.5, (name, "the bent mesh still encloses its centre")
    sdf, rec = rt.signed_distance(ctx, scene, pts)
    near = NR.nearest(read, pts)
    same(rec, near, name + " updated: the records")
    same(sdf, W.sdf(after, near["distance"]), name + " updated: sdf")


# ---- the device form and the launch order ------------------------------------------------------------------------------------------------
def test_device_form_tensors_and_pointers(rt, ctx, models_dir):
    import torch
    flat, pts, want = reference(rt, models_dir, "monkey")
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir))
    d_pts = torch.from_numpy(pts).to("cuda:0")
    w, flags = rt.winding_numbers_device(ctx, scene, d_pts)
    assert flags is None
    same(w.cpu().numpy(), want, "tensors, a new winding tensor")
    flags = torch.full((pts.shape[0],), 0x77, dtype=torch.uint8, device="cuda:0")
    w2, f2 = rt.winding_numbers_device(ctx, scene, d_pts, inside=flags)
    assert w2 is None and f2 is flags
    same(flags.cpu().numpy(), W.inside(want), "tensors, inside only")
    w.fill_(7.0)
    flags.fill_(0x77)
    rt.winding_numbers_device(ctx, scene, d_pts.data_ptr(), rt.WINDING_SOLIDS, w.data_ptr(), flags.data_ptr(), n=pts.shape[0])
    torch.cuda.synchronize()
    same(w.cpu().numpy(), want, "pointers: winding")
    same(flags.cpu().numpy(), W.inside(want), "pointers: inside")
    with pytest.raises(ValueError):
        rt.winding_numbers_device(ctx, scene, d_pts.double())
    with pytest.raises(ValueError):
        rt.winding_numbers_device(ctx, scene, d_pts.data_ptr(), winding=w.data_ptr())


def test_points_produced_on_the_stream_just_ahead_of_the_call(rt, models_dir):
    """In the manner of tests/test_gpu_streams.py: on a sleeping stream the points are copied into place, the call is queued, the answers are
    copied out - the host waits for nothing in between - and the answers are those of a synchronised call on a fresh context."""
    import torch
    flat, pts, ref = reference(rt, models_dir, "monkey")
    dev = torch.device("cuda:0")
    fresh = rt.Context(0)
    want = rt.winding_numbers(fresh, fresh.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir)), pts)
    same(want, ref, "the synchronised call")
    want_sdf = rt.signed_distance(fresh, fresh.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir)), pts)[0]
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir))
    src = torch.from_numpy(pts).to(dev)
    buf = torch.empty_like(src)
    out = torch.empty((pts.shape[0],), dtype=torch.float32, device=dev)
    sdf = torch.empty_like(out)
    res, res_sdf = torch.empty_like(out), torch.empty_like(out)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rt.winding_numbers_device(c, scene, src, winding=out, stream=stream.cuda_stream)      # warm: the kernels are loaded, the scene has its flip bytes
        rt.signed_distance_device(c, scene, src, sdf=sdf, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    buf.fill_(float("nan"))
    for t in (out, sdf, res, res_sdf):
        t.fill_(123.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(60000000)
        buf.copy_(src, non_blocking=True)
        rt.winding_numbers_device(c, scene, buf, winding=out, stream=stream.cuda_stream)
        rt.signed_distance_device(c, scene, buf, sdf=sdf, stream=stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        pending = not ev.query()
        res.copy_(out, non_blocking=True)
        res_sdf.copy_(sdf, non_blocking=True)
    torch.cuda.synchronize()
    assert pending, "the stream had run dry before the calls returned: the window was not open"
    same(res.cpu().numpy(), want, "winding numbers queued behind the producer of their points")
    same(res_sdf.cpu().numpy(), want_sdf, "signed distances queued behind the producer of their points")


def test_a_winding_and_a_nearest_call_on_two_streams(rt, models_dir):
    """one context, two streams, back to back: both use the context's point counter, so the second is ordered behind the first"""
    import torch
    flat, pts, want = reference(rt, models_dir, "monkey")
    want_near = NR.nearest(flat, pts)
    dev = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, "monkey"), models_dir))
    d_pts = torch.from_numpy(pts).to(dev)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for first in ("winding", "nearest"):
        w = torch.full((pts.shape[0],), 9.0, dtype=torch.float32, device=dev)
        rec = torch.full((pts.shape[0], 32), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        calls = {"winding": lambda s: rt.winding_numbers_device(c, scene, d_pts, winding=w, stream=s.cuda_stream),
                 "nearest": lambda s: rt.nearest_points_device(c, scene, d_pts, out=rec, stream=s.cuda_stream)}
        second = "nearest" if first == "winding" else "winding"
        calls[first](s1)
        calls[second](s2)
        torch.cuda.synchronize()
        same(w.cpu().numpy(), want, "winding numbers, %s first" % first)
        same(rec.cpu().numpy().view(rt.NearestRecord).reshape(-1), want_near, "nearest records, %s first" % first)


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_answer_alone(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    flat, pts_all, want_all = reference(rt, models_dir, "reference_scene0")
    n = 70
    pts_h, want = pts_all[:n], want_all[:n]
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, "reference_scene0"), models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objects_of(rt, "three_sphere"), models_dir))
    pts = torch.from_numpy(pts_h).to("cuda:0")
    w = torch.full((n,), 5.0, dtype=torch.float32, device="cuda:0")
    flags = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda:0")
    rec = torch.full((n * 32 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p, pw, pf, pr = (C.c_void_p(t.data_ptr()) for t in (pts, w, flags, rec))
    dev, S = L.rt_winding_numbers_device, rt.WINDING_SOLIDS
    n_obj = len(flat["objects"])
    assert dev(ctx._h, scene._h, p, -1, S, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, (1 << 30) + 1, S, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, None, n, S, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, n, S, None, None, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, n, n_obj, pw, pf, None) == rt.RT_ERR_INVALID and "object" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, n, -2, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, foreign._h, p, n, S, pw, pf, None) == rt.RT_ERR_INVALID and "another context" in ctx.last_error()
    assert dev(None, scene._h, p, n, S, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, None, p, n, S, pw, pf, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, None, 0, S, None, None, None) == rt.RT_OK
    sd = L.rt_signed_distance_device
    assert sd(ctx._h, scene._h, p, None, -1, pr, pw, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, None, None, n, pr, pw, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, p, None, n, pr, None, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, p, None, n, C.c_void_p(rec.data_ptr() + 4), pw, None) == rt.RT_ERR_INVALID and "16-byte aligned" in ctx.last_error()
    assert sd(ctx._h, foreign._h, p, None, n, pr, pw, None) == rt.RT_ERR_INVALID
    assert sd(ctx._h, scene._h, None, None, 0, None, None, None) == rt.RT_OK
    fp = C.POINTER(C.c_float)
    host_w = np.zeros(n, np.float32)
    assert L.rt_winding_numbers(ctx._h, scene._h, pts_h.ctypes.data_as(fp), n, n_obj, host_w.ctypes.data_as(fp), None) == rt.RT_ERR_INVALID
    assert L.rt_winding_numbers(ctx._h, scene._h, None, n, S, host_w.ctypes.data_as(fp), None) == rt.RT_ERR_INVALID
    assert L.rt_signed_distance(ctx._h, scene._h, pts_h.ctypes.data_as(fp), None, n, None, None) == rt.RT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((w == 5.0).all()) and bool((flags == 0x77).all()) and bool((rec == 0x77).all()), "a refused call wrote answers"
    # the valid call that follows answers as if nothing had been refused
    rt.winding_numbers_device(ctx, scene, pts, winding=w, inside=flags)
    same(w.cpu().numpy(), want, "the call after the refusals: winding")
    same(flags.cpu().numpy(), W.inside(want), "the call after the refusals: inside")


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------------
def test_example_sdf_program(rt, ctx, models_dir, tmp_path):
    """host/example_sdf.cpp (Renderer::winding_numbers, contains, signed_distance of host/raytracer.hpp): it builds, its probe and its slice are
    the yardstick's for the same scene, and the PGM has the slice's size"""
    import re
    import subprocess
    exe = rt.build.build_sdf_example()
    Wd, H = 40, 32
    pgm = tmp_path / "slice.pgm"
    r = subprocess.run([exe, models_dir, str(Wd), str(H), str(pgm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    objs = [("obj", "low_poly_monkey.obj", [("enlarge", 0.3), ("rotate", 0, 2.3, 0), ("translate", 0.1, -0.1, 1.6)], ("standard", (1, 1, 1), 0.0))]
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    probe = np.array([[0.1, -0.1, 1.6]], np.float32)
    m = re.search(r"probe: winding (\S+) inside (\d) sdf (\S+)", r.stdout)
    w = W.winding(flat, probe)
    assert m and np.float32(m.group(1)) == w[0] and int(m.group(2)) == int(W.inside(w)[0]) == 1, (r.stdout, w)
    assert np.float32(m.group(3)) == W.sdf(w, NR.nearest(flat, probe)["distance"])[0]
    xs = (np.float32(-0.6) + np.float32(1.2) * np.arange(Wd, dtype=np.float32) / np.float32(Wd - 1)).astype(np.float32)
    ys = (np.float32(0.6) - np.float32(1.2) * np.arange(H, dtype=np.float32) / np.float32(H - 1)).astype(np.float32)
    grid = np.stack([np.broadcast_to(xs[None, :], (H, Wd)), np.broadcast_to(ys[:, None], (H, Wd)), np.full((H, Wd), 1.6, np.float32)], axis=-1).reshape(-1, 3)
    field = W.sdf(W.winding(flat, grid), NR.nearest(flat, grid)["distance"])
    m = re.search(r"slice: (\d+) points, (\d+) inside, sdf from (\S+) to (\S+)", r.stdout)
    assert m and int(m.group(1)) == Wd * H and int(m.group(2)) == int((field < 0).sum()), (r.stdout, int((field < 0).sum()))
    assert np.float32(m.group(3)) == field.min() and np.float32(m.group(4)) == field.max(), (r.stdout, field.min(), field.max())
    data = pgm.read_bytes()
    head = b"P5\n%d %d\n255\n" % (Wd, H)
    assert data.startswith(head) and len(data) == len(head) + Wd * H
