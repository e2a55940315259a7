"""The nearest-surface queries on the GPU (rt_nearest_points[_device]) against tests/nearest_ref.py, the NumPy binary32 yardstick that
evaluates every candidate of every point: every record compared as BYTES.  Nothing is skipped and nothing is tolerated.

Scenes: three-sphere, cube, monkey, reference scenes 0 and 4 (quads, cuboids, 100 spheres), the two richest seeds of tests/random_scenes.py,
nine meshes of 1 to 9 triangles (every chain shape), a 3,000-triangle mesh read from global memory, soup6k on the hybrid and on the global
placement - the placement asserted from scene.info().  Every shape of RT_SHAPES is forced the way tests/test_gpu_shapes.py forces it, on
the smallest scene that reaches it.  Points, seeded per scene (nearest_ref.query_points): uniform in twice the scene's bounds, vertices, edge
midpoints and centroids of a sample of triangles, sphere centres, points at 2^20, signed zeros, and points that are not finite.  Limits: per
point, in turn, the yardstick's distance, that one ulp down, one ulp up, 0, a negative one, NaN and +Inf - and no limit array at all.
The yardstick's answers are computed once per scene and shared.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import nearest_ref as R
from random_scenes import random_scene
from test_gpu_shapes import SHAPES, _id, commit_as, plan, spheres_beyond_lds

pytestmark = pytest.mark.gpu

N_UNIFORM = {"soup6k": 1700, "soup3000": 1500, "spheres_beyond_lds": 1200}       # (at most 2,048 points on the large scenes: the yardstick stays within seconds)
_REFS = {}


def tiny_meshes():
    """nine meshes of 1 to 9 triangles and a sphere: every shape a tree of few triangles takes (a leaf at the root, chains, one node, two levels)"""
    rng = np.random.default_rng(5)
    objs = []
    for n in range(1, 10):
        c = rng.uniform([-1.0, -0.6, 1.2], [1.0, 0.8, 3.0])
        tris = (c + rng.normal(0, 0.2, (n, 1, 3)) + rng.normal(0, 0.1, (n, 3, 3))).astype(np.float32).reshape(n, 9)
        objs.append(("mesh", tris, ("standard", (0.6, 0.6, 0.6), 0.1)))
    objs.append(("sphere", (0.0, 0.2, 2.0), 0.15, ("standard", (0.5, 0.5, 0.5), 0.0)))
    return objs


def soup3000():
    rng = np.random.default_rng(31)
    tris = (np.array([0.0, 0.0, 2.2]) + rng.normal(0, 0.4, (3000, 1, 3)) + rng.normal(0, 0.05, (3000, 3, 3))).astype(np.float32).reshape(3000, 9)
    return [("mesh", tris, ("standard", (0.6, 0.6, 0.6), 0.1)), ("sphere", (0.0, 1.3, 1.5), 0.5, ("emissive", (1, 1, 1), 5.0))]


def objects_of(rt, name):
    if name.startswith("random"):
        return random_scene(int(name[6:]))[0]
    if name == "tiny_meshes":
        return tiny_meshes()
    if name == "soup3000":
        return soup3000()
    if name == "spheres_beyond_lds":
        return rt.scenes.reference_scene4(num_spheres=spheres_beyond_lds(rt))[0]
    return rt.scenes.CONFIG_SCENES[name]()[0]


def limits_for(d):
    """per point, in turn: the yardstick's distance, one ulp down, one ulp up, 0, negative, NaN, +Inf"""
    lim = d.copy()
    k = np.arange(d.shape[0]) % 7
    lim[k == 1] = np.nextafter(d[k == 1], np.float32(0))
    lim[k == 2] = np.nextafter(d[k == 2], np.float32(np.inf))
    lim[k == 3] = 0.0
    lim[k == 4] = -0.5
    lim[k == 5] = np.nan
    lim[k == 6] = np.inf
    return lim


def reference(rt, models_dir, name):
    """(points, records without a limit, limits, records under them) of the scene, from the yardstick alone"""
    if name not in _REFS:
        flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
        pts = R.query_points(flat, sum(name.encode()), N_UNIFORM.get(name, 3000))
        pts = np.concatenate([pts, np.array([[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf], [np.nan, np.nan, np.nan]], np.float32)])
        assert name not in N_UNIFORM or pts.shape[0] <= 2048
        free = R.nearest(flat, pts)
        lim = limits_for(free["distance"])
        _REFS[name] = (pts, free, lim, R.nearest(flat, pts, lim))
        hit = free["object"] >= 0
        assert hit.sum() == pts.shape[0] - 4 and (free["triangle"][hit] >= 0).any() == (flat["num_triangles"] > 0), name
    return _REFS[name]


def same(got, want, what):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, "%d of %d records differ, first at %s" % (
        int((got != want).sum()), got.size, np.nonzero(got != want)[0][:5]))


def check_scene(rt, ctx, scene, ref, what):
    pts, free, lim, limited = ref
    same(rt.nearest_points(ctx, scene, pts), free, what + ", no limits")
    same(rt.nearest_points(ctx, scene, pts, lim), limited, what + ", limits")
    same(rt.nearest_points(ctx, scene, pts, np.float32(np.inf)), free, what + ", +Inf everywhere")


# ---- scenes on the placement they pick or are given ---------------------------------------------------------------------------------
PLACED = [("three_sphere", {}, 1), ("cube", {}, 1), ("monkey", {}, 1), ("reference_scene0", {}, 1), ("reference_scene4", {}, 1), ("random13", {}, 1),
          ("random15", {}, 1), ("tiny_meshes", {}, 1), ("soup3000", {"RT_AMD_SCENE_MODE": "0"}, 0), ("soup6k", {}, 2), ("soup6k", {"RT_AMD_SCENE_MODE": "0"}, 0)]


@pytest.mark.parametrize("name,env,mode", PLACED, ids=["%s-%s" % (n, {0: "global", 1: "lds", 2: "hybrid"}[m]) for n, _, m in PLACED])
def test_records_equal_the_yardstick(rt, ctx, models_dir, monkeypatch, name, env, mode):
    scene = commit_as(rt, ctx, monkeypatch, objects_of(rt, name), models_dir, env)
    info = scene.info()
    assert info["scene_in_lds"] == mode, (name, info)
    check_scene(rt, ctx, scene, reference(rt, models_dir, name), "%s %s" % (name, info))


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
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    check_scene(rt, ctx, scene, reference(rt, models_dir, name), "%s on %s" % (name, _id(shape)))


# ---- counts around a wave and a chunk -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["monkey", "reference_scene4"])
def test_point_counts(rt, ctx, models_dir, name):
    flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
    key = ("counts", name)
    if key not in _REFS:
        q = R.query_points(flat, 99, 4097)
        pts = np.concatenate([q[4097:], q[:4097]])[:4097]              # the points on surfaces, at 2^20 and at the zeros first, then the uniform ones
        assert pts.shape == (4097, 3)
        _REFS[key] = (pts, R.nearest(flat, pts))
    pts, want = _REFS[key]
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    for n in (1, 63, 64, 65, 4097):
        same(rt.nearest_points(ctx, scene, pts[:n]), want[:n], "%s n=%d" % (name, n))
    assert rt.nearest_points(ctx, scene, np.zeros((0, 3), np.float32)).shape == (0,)
    assert ctx.last_kernel_ms() > 0.0


# ---- a scene updated on the device ---------------------------------------------------------------------------------------------------
def test_after_update_mesh_device(rt, ctx, models_dir):
    import torch
    rng = np.random.default_rng(8)
    n = 700
    old = (np.array([0.0, 0.0, 2.0]) + rng.normal(0, 0.3, (n, 1, 3)) + rng.normal(0, 0.06, (n, 3, 3))).astype(np.float32).reshape(n, 9)
    new = (old * np.float32(1.15) + rng.normal(0, 0.02, old.shape)).astype(np.float32)
    sphere = ("sphere", (0.7, 0.4, 1.4), 0.2, ("standard", (0.5, 0.5, 0.5), 0.0))
    mat = ("standard", (0.6, 0.6, 0.6), 0.1)
    scene = ctx.commit(rt.SceneObjects([sphere, ("mesh", old, mat)], models_dir))
    fresh_objs = rt.SceneObjects([sphere, ("mesh", new, mat)], models_dir)
    flat = fresh_objs.debug_flatten()
    pts = R.query_points(flat, 3, 1500)
    before = rt.nearest_points(ctx, scene, pts)
    scene.update_mesh_device(1, torch.from_numpy(new).to("cuda:0"))
    after = rt.nearest_points(ctx, scene, pts)
    same(after, rt.nearest_points(ctx, ctx.commit(fresh_objs), pts), "updated against a fresh commit")
    same(after, R.nearest(scene.debug_read(), pts), "updated against the yardstick on the device's scene")
    same(after, R.nearest(flat, pts), "updated against the yardstick on a fresh flatten")
    assert before.tobytes() != after.tobytes()


# ---- device form: tensors, a stream, the lattice ---------------------------------------------------------------------------------------
def test_device_form_and_distance_grid(rt, ctx, models_dir):
    import torch
    name = "monkey"
    pts, free, lim, limited = reference(rt, models_dir, name)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    d_pts, d_lim = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(lim).to("cuda:0")
    same(rt.nearest_points_device(ctx, scene, d_pts).cpu().numpy().view(rt.NearestRecord).reshape(-1), free, "tensors")
    out = torch.full((pts.shape[0], 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert rt.nearest_points_device(ctx, scene, d_pts, d_lim, out=out) is out
    same(out.cpu().numpy().view(rt.NearestRecord).reshape(-1), limited, "tensors, limits, a buffer of the caller's")
    out.fill_(0x5A)
    rt.nearest_points_device(ctx, scene, d_pts.data_ptr(), None, out=out.data_ptr(), n=pts.shape[0])
    torch.cuda.synchronize()
    same(out.cpu().numpy().view(rt.NearestRecord).reshape(-1), free, "pointers")
    # the lattice: what torch.linspace gives, answered like any other points
    flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
    lo, hi = R.scene_bounds(flat)
    shape = (9, 7, 5)
    dist, rec = rt.distance_grid(scene, lo, hi, shape)
    axes = [torch.linspace(float(lo[k]), float(hi[k]), shape[k], dtype=torch.float32).numpy() for k in range(3)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    want = R.nearest(flat, grid)
    same(rec.cpu().numpy().view(rt.NearestRecord).reshape(-1), want, "distance_grid's records")
    assert dist.shape == shape and dist.cpu().numpy().tobytes() == want["distance"].tobytes()


# ---- the launch order ----------------------------------------------------------------------------------------------------------------
def test_points_produced_on_the_stream_just_ahead_of_the_call(rt, models_dir):
    """In the manner of tests/test_gpu_streams.py: on a sleeping stream the points are copied into place, the call is queued, the records
    are copied out - the host waits for nothing in between - and the records are those of a synchronised call on a fresh context."""
    import torch
    name = "monkey"
    pts, free, _, _ = reference(rt, models_dir, name)
    dev = torch.device("cuda:0")
    fresh = rt.Context(0)
    want = rt.nearest_points(fresh, fresh.commit(rt.SceneObjects(objects_of(rt, name), models_dir)), pts)
    same(want, free, "the synchronised call")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    src = torch.from_numpy(pts).to(dev)
    buf = torch.empty_like(src)
    out = torch.empty((pts.shape[0], 32), dtype=torch.uint8, device=dev)
    res = torch.empty_like(out)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rt.nearest_points_device(c, scene, src, out=out, stream=stream.cuda_stream)          # warm: the kernel is loaded, the stream has its queue
    torch.cuda.synchronize()
    buf.fill_(float("nan"))
    out.fill_(0xEE)
    res.fill_(0xEE)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(60000000)
        buf.copy_(src, non_blocking=True)
        rt.nearest_points_device(c, scene, buf, out=out, stream=stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        pending = not ev.query()
        res.copy_(out, non_blocking=True)
    torch.cuda.synchronize()
    assert pending, "the stream had run dry before the call returned: the window was not open"
    same(res.cpu().numpy().view(rt.NearestRecord).reshape(-1), want, "queued behind the producer of its points")


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, "three_sphere"), models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objects_of(rt, "three_sphere"), models_dir))
    pts = torch.zeros((4, 3), dtype=torch.float32, device="cuda:0")
    out = torch.full((4 * 32 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p, o = C.c_void_p(pts.data_ptr()), C.c_void_p(out.data_ptr())
    dev = L.rt_nearest_points_device
    assert dev(ctx._h, scene._h, p, None, -1, o, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, None, (1 << 30) + 1, o, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, None, None, 4, o, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, None, 4, None, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, None, 4, C.c_void_p(out.data_ptr() + 4), None) == rt.RT_ERR_INVALID and "16-byte aligned" in ctx.last_error()
    assert dev(ctx._h, foreign._h, p, None, 4, o, None) == rt.RT_ERR_INVALID and "another context" in ctx.last_error()
    assert dev(None, scene._h, p, None, 4, o, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, None, p, None, 4, o, None) == rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, None, None, 0, None, None) == rt.RT_OK
    host = np.zeros((4, 3), np.float32)
    rec = np.zeros(4, rt.NearestRecord)
    fp = C.POINTER(C.c_float)
    assert L.rt_nearest_points(ctx._h, scene._h, host.ctypes.data_as(fp), None, -1, C.c_void_p(rec.ctypes.data)) == rt.RT_ERR_INVALID
    assert L.rt_nearest_points(ctx._h, scene._h, None, None, 4, C.c_void_p(rec.ctypes.data)) == rt.RT_ERR_INVALID
    assert L.rt_nearest_points(ctx._h, foreign._h, host.ctypes.data_as(fp), None, 4, C.c_void_p(rec.ctypes.data)) == rt.RT_ERR_INVALID
    assert L.rt_nearest_points(ctx._h, scene._h, None, None, 0, None) == rt.RT_OK
    torch.cuda.synchronize()
    assert bool((out == 0x77).all()), "a refused call wrote records"
    with pytest.raises(ValueError):
        rt.nearest_points_device(ctx, scene, pts.double())
    with pytest.raises(ValueError):
        rt.nearest_points_device(ctx, scene, pts.data_ptr(), None, out=None, n=4)


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_example_nearest_program(rt, ctx, models_dir, tmp_path):
    """host/example_nearest.cpp (Renderer::nearest_point, Renderer::nearest_points of host/raytracer.hpp): it builds, its probe and its slice
    are the yardstick's for the same scene, and the PGM has the slice's size"""
    import re
    import subprocess
    exe = rt.build.build_nearest_example()
    W, H = 48, 40
    pgm = tmp_path / "slice.pgm"
    r = subprocess.run([exe, models_dir, str(W), str(H), str(pgm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    objs = [("obj", "low_poly_monkey.obj", [("enlarge", 0.3), ("rotate", 0, 2.3, 0), ("translate", 0.1, -0.1, 1.6)], ("standard", (1, 1, 1), 0.0))]
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    want = R.nearest(flat, np.array([[0.1, 0.4, 1.6]], np.float32))[0]
    m = re.search(r"probe: object (-?\d+) triangle (-?\d+) distance (\S+) point (\S+) (\S+) (\S+)", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (want["object"], want["triangle"]), r.stdout
    assert np.float32(m.group(3)) == want["distance"] and [np.float32(m.group(k)) for k in (4, 5, 6)] == list(want["point"]), (r.stdout, want)
    xs = (np.float32(-0.6) + np.float32(1.2) * np.arange(W, dtype=np.float32) / np.float32(W - 1)).astype(np.float32)
    ys = (np.float32(0.6) - np.float32(1.2) * np.arange(H, dtype=np.float32) / np.float32(H - 1)).astype(np.float32)
    grid = np.stack([np.broadcast_to(xs[None, :], (H, W)), np.broadcast_to(ys[:, None], (H, W)), np.full((H, W), 1.6, np.float32)], axis=-1).reshape(-1, 3)
    field = R.nearest(flat, grid)["distance"]
    m = re.search(r"slice: (\d+) points, nearest (\S+) farthest (\S+), (\d+) within", r.stdout)
    assert m and int(m.group(1)) == W * H and np.float32(m.group(2)) == field.min() and np.float32(m.group(3)) == field.max(), (r.stdout, field.min(), field.max())
    assert int(m.group(4)) == int((field <= np.float32(0.3)).sum())
    data = pgm.read_bytes()
    assert data.startswith(b"P5\n%d %d\n255\n" % (W, H)) and len(data) == len(b"P5\n%d %d\n255\n" % (W, H)) + W * H
