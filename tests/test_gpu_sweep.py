"""The sphere-cast queries on the GPU (rt_sweep_spheres[_device]) against tests/sweep_ref.py, the NumPy binary32 yardstick that evaluates
every candidate of every ball: every record compared as BYTES.  Nothing is skipped and nothing is tolerated.  Every output buffer holds a
pattern before the call, so that a record the kernel never wrote shows.

Scenes and placements: tests/test_gpu_nearest.py's PLACED, the placement asserted from scene.info(); every shape of RT_SHAPES forced the
way tests/test_gpu_shapes.py forces it, on the smallest scene that reaches it.  Balls, seeded per scene (sweep_ref.query_sweeps: aimed at
vertices, edges, interiors and sphere centres, origins inside spheres and within r of the surface, radii from 0 to larger than a mesh),
then inputs that are not valid.  Limits: per ball, in turn, the winner's key, one ulp below it, one ulp above it, 0, a negative one, NaN
and +Inf - and no limit array at all.  The yardstick's answers are computed once per scene (tests/sweep_scenes.py) and shared.
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import sweep_ref as R
import sweep_scenes as SS
from test_gpu_nearest import PLACED
from test_gpu_random_scenes import Case
from test_gpu_refill import PATTERN, batch_size, dev, filled
from test_gpu_shapes import SHAPES, _id, commit_as, plan

pytestmark = pytest.mark.gpu


def same(got, want, what):
    a, b = got.view(np.uint8).reshape(-1, R.DTYPE.itemsize), want.view(np.uint8).reshape(-1, R.DTYPE.itemsize)
    assert got.dtype == want.dtype and a.shape == b.shape, (what, got.shape, want.shape)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, (what, "%d of %d records differ, first at %s: got %s, want %s" % (bad.size, got.size, bad[:5], got[bad[:2]], want[bad[:2]]))


def sweep_device(rt, ctx, scene, o, d, r, lim):
    """the device form into a buffer that holds PATTERN, one launch, one copy back"""
    import torch
    out = filled((len(o), rt.SweepRecord.itemsize))
    torch.cuda.synchronize()
    res = rt.sweep_spheres_device(ctx, scene, dev(o), dev(d), dev(r), dev(lim) if lim is not None else None, out=out)
    assert res is out
    torch.cuda.synchronize()
    return out.cpu().numpy().view(rt.SweepRecord).reshape(-1)


def check_scene(rt, ctx, scene, ref, what):
    o, d, r = ref["o"], ref["d"], ref["r"]
    same(sweep_device(rt, ctx, scene, o, d, r, None), ref["free"], what + ", no limits")
    same(sweep_device(rt, ctx, scene, o, d, r, ref["lim"]), ref["limited"], what + ", limits")
    same(sweep_device(rt, ctx, scene, o, d, r, np.full(len(o), np.inf, np.float32)), ref["free"], what + ", +Inf everywhere")


# ---- scenes on the placement they pick or are given ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env,mode", PLACED, ids=["%s-%s" % (n, {0: "global", 1: "lds", 2: "hybrid"}[m]) for n, _, m in PLACED])
def test_records_equal_the_yardstick(rt, ctx, models_dir, monkeypatch, name, env, mode):
    scene = commit_as(rt, ctx, monkeypatch, SS.objects_of(rt, name), models_dir, env)
    info = scene.info()
    assert info["scene_in_lds"] == mode, (name, info)
    check_scene(rt, ctx, scene, SS.reference(rt, models_dir, name), "%s %s" % (name, info))


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
    objs = SS.objects_of(rt, name)
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, env)
    info = scene.info()
    has_mesh = int(rt.SceneObjects(objs, models_dir).debug_flatten()["has_mesh"])
    assert (has_mesh, info["scene_in_lds"], info["threads_per_block"]) == shape, (name, info)
    ref = SS.reference(rt, models_dir, name)
    o, d, r = ref["o"], ref["d"], ref["r"]
    same(sweep_device(rt, ctx, scene, o, d, r, None), ref["free"], "%s on %s, no limits" % (name, _id(shape)))
    same(sweep_device(rt, ctx, scene, o, d, r, ref["lim"]), ref["limited"], "%s on %s, limits" % (name, _id(shape)))


# ---- the limits and the invalid inputs, looked at one kind at a time -----------------------------------------------------------------
def test_limits_around_the_winners_key(rt, ctx, models_dir):
    """the yardstick's own records say what each kind of limit does - the winner stays at its key and one ulp above, goes one ulp below, and
    0, a negative limit and NaN miss - and the device gives those records"""
    name = "monkey"
    ref = SS.reference(rt, models_dir, name)
    free, limited, lim = ref["free"], ref["limited"], ref["lim"]
    k = np.arange(free.shape[0]) % 7
    hit = (free["object"] >= 0) & (free["overlap"] == 0)
    for kind in (0, 2, 6):
        assert hit[k == kind].sum() > 100 and limited[(k == kind) & hit].tobytes() == free[(k == kind) & hit].tobytes(), kind
    below = (k == 1) & hit
    assert below.sum() > 100 and not (limited["t"][below] == free["t"][below]).all()
    moved = below & ((limited["object"] != free["object"]) | (limited["triangle"] != free["triangle"]))
    assert moved.sum() > 50, "one ulp below the key the winner must go"
    for kind in (3, 4, 5):
        assert (limited["object"][k == kind] == -1).all() and (limited["t"][k == kind] == R.MISS_T).all(), kind
    scene = ctx.commit(rt.SceneObjects(SS.objects_of(rt, name), models_dir))
    same(sweep_device(rt, ctx, scene, ref["o"], ref["d"], ref["r"], lim), limited, "the limits in turn")


def test_invalid_inputs_miss(rt, ctx, models_dir):
    name = "random13"
    ref = SS.reference(rt, models_dir, name)
    io, id_, ir = SS.invalid_balls()
    scene = ctx.commit(rt.SceneObjects(SS.objects_of(rt, name), models_dir))
    miss = np.zeros(io.shape[0], R.DTYPE)
    miss["t"] = R.MISS_T
    miss["object"] = miss["triangle"] = miss["feature"] = -1
    assert ref["free"][ref["n_seeded"]:].tobytes() == miss.tobytes()
    same(sweep_device(rt, ctx, scene, io, id_, ir, None), miss, "inputs that are not valid")
    same(rt.sweep_spheres(ctx, scene, io, id_, ir, 5.0), miss, "inputs that are not valid, the host form")


# ---- the host form, scalars broadcast, pointers, the lattice ---------------------------------------------------------------------------
def test_host_form_and_python_forms(rt, ctx, models_dir):
    import torch
    name = "monkey"
    ref = SS.reference(rt, models_dir, name)
    o, d, r = ref["o"], ref["d"], ref["r"]
    scene = ctx.commit(rt.SceneObjects(SS.objects_of(rt, name), models_dir))
    same(rt.sweep_spheres(ctx, scene, o, d, r), ref["free"], "the host form")
    same(rt.sweep_spheres(ctx, scene, o, d, r, ref["lim"]), ref["limited"], "the host form, limits")
    assert ctx.last_kernel_ms() > 0.0
    assert rt.sweep_spheres(ctx, scene, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0.1).shape == (0,)
    # a scalar radius and a scalar limit are broadcast
    rad, tmax = np.float32(0.05), np.float32(2.5)
    want = R.sweep(ref["flat"], o[:500], d[:500], rad, tmax)
    same(rt.sweep_spheres(ctx, scene, o[:500], d[:500], rad, tmax), want, "scalars, the host form")
    got = rt.sweep_spheres_device(ctx, scene, dev(o[:500]), dev(d[:500]), float(rad), float(tmax))
    torch.cuda.synchronize()
    same(got.cpu().numpy().view(rt.SweepRecord).reshape(-1), want, "scalars, tensors")
    # pointers
    out = filled((len(o), rt.SweepRecord.itemsize))
    t_o, t_d, t_r = dev(o), dev(d), dev(r)
    torch.cuda.synchronize()
    rt.sweep_spheres_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), t_r.data_ptr(), None, out=out.data_ptr(), n=len(o))
    torch.cuda.synchronize()
    same(out.cpu().numpy().view(rt.SweepRecord).reshape(-1), ref["free"], "pointers")
    # the lattice: a ball dropped straight down on a grid above the monkey
    lo, hi = R.scene_bounds(ref["flat"])
    shape = (9, 1, 7)
    top = float(hi[1]) + 1.0
    t, rec = rt.sweep_grid(scene, (lo[0], top, lo[2]), (hi[0], top, hi[2]), shape, (0.0, -1.0, 0.0), 0.08)
    axes = [torch.linspace(float(lo[0]), float(hi[0]), 9, dtype=torch.float32).numpy(), np.array([top], np.float32),
            torch.linspace(float(lo[2]), float(hi[2]), 7, dtype=torch.float32).numpy()]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    want = R.sweep(ref["flat"], grid, np.broadcast_to(np.array([0, -1, 0], np.float32), grid.shape), np.float32(0.08))
    same(rec.cpu().numpy().view(rt.SweepRecord).reshape(-1), want, "sweep_grid's records")
    assert t.shape == shape and t.cpu().numpy().tobytes() == want["t"].tobytes() and (want["object"] >= 0).any()


# ---- a scene updated on the device ---------------------------------------------------------------------------------------------------
def test_after_update_mesh_device(rt, ctx, models_dir):
    """the monkey bent on the device (as tests/test_gpu_scene_update.py's animation bends it): the balls of the committed scene answered for
    the new triangles, against the yardstick on what the device holds and on a fresh flatten of the new geometry"""
    import torch
    from test_gpu_scene_update import obj_triangles
    objs, _ = rt.scenes.CONFIG_SCENES["monkey"]()
    assert objs[0][0] == "obj"
    base = obj_triangles(rt, models_dir, objs[0])
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    ref = SS.reference(rt, models_dir, "monkey")
    o, d, r = ref["o"], ref["d"], ref["r"]
    before = sweep_device(rt, ctx, scene, o, d, r, None)
    same(before, ref["free"], "before the update")
    tris = base.copy().reshape(-1, 3, 3)
    tris[:, :, 1] += (np.float32(0.05) * np.sin(np.float32(2) + np.float32(3) * tris[:, :, 0])).astype(np.float32)
    tris = np.ascontiguousarray(tris.reshape(-1, 9), np.float32)
    scene.update_mesh_device(0, torch.from_numpy(tris).to("cuda:0"))
    after = sweep_device(rt, ctx, scene, o, d, r, None)
    now = [("mesh", tris, objs[0][-1])] + list(objs[1:])
    want = R.sweep(rt.SceneObjects(now, models_dir).debug_flatten(), o, d, r)
    same(after, want, "updated against the yardstick on a fresh flatten")
    same(after, R.sweep(scene.debug_read(), o, d, r), "updated against the yardstick on the device's scene")
    assert before.tobytes() != after.tobytes()


# ---- the launch order ----------------------------------------------------------------------------------------------------------------
def test_inputs_produced_on_the_stream_just_ahead_of_the_call(rt, models_dir):
    """In the manner of tests/test_gpu_streams.py: on a sleeping stream the balls are copied into place, the call is queued, the records
    are copied out - the host waits for nothing in between - and the records are the yardstick's."""
    import torch
    name = "monkey"
    ref = SS.reference(rt, models_dir, name)
    dev0 = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(SS.objects_of(rt, name), models_dir))
    src = [dev(ref[k]) for k in ("o", "d", "r")]
    buf = [torch.empty_like(s) for s in src]
    out = torch.empty((ref["o"].shape[0], rt.SweepRecord.itemsize), dtype=torch.uint8, device=dev0)
    res = torch.empty_like(out)
    stream = torch.cuda.Stream(device=dev0)
    with torch.cuda.stream(stream):
        rt.sweep_spheres_device(c, scene, src[0], src[1], src[2], out=out, stream=stream.cuda_stream)      # warm: the kernels are loaded, the stream has its queue
    torch.cuda.synchronize()
    for b in buf:
        b.fill_(float("nan"))
    out.fill_(PATTERN)
    res.fill_(PATTERN)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(60000000)
        for b, s in zip(buf, src):
            b.copy_(s, non_blocking=True)
        rt.sweep_spheres_device(c, scene, buf[0], buf[1], buf[2], out=out, stream=stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        pending = not ev.query()
        res.copy_(out, non_blocking=True)
    torch.cuda.synchronize()
    assert pending, "the stream had run dry before the call returned: the window was not open"
    same(res.cpu().numpy().view(rt.SweepRecord).reshape(-1), ref["free"], "queued behind the producer of its balls")


def test_a_sweep_and_a_nearest_call_on_two_streams_of_one_context(rt, models_dir):
    """the sweep keeps its nearest-surface records in the context's record buffer, which rt_signed_distance_device uses too when it is given
    none: a sweep on one stream, and on another, with nothing waited for in between, a signed-distance call without a record buffer and a
    nearest call - each answer is the one of a call made alone"""
    import torch
    import nearest_ref as NR
    name = "monkey"
    ref = SS.reference(rt, models_dir, name)
    dev0 = torch.device("cuda:0")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(SS.objects_of(rt, name), models_dir))
    t_o, t_d, t_r = dev(ref["o"]), dev(ref["d"]), dev(ref["r"])
    pts = np.ascontiguousarray(ref["o"][::-1])
    t_p = dev(pts)
    want_near = NR.nearest(ref["flat"], pts)
    a, b = torch.cuda.Stream(device=dev0), torch.cuda.Stream(device=dev0)
    out = filled((len(pts), rt.SweepRecord.itemsize))
    near = filled((len(pts), rt.NearestRecord.itemsize))
    sdf_alone, _ = rt.signed_distance_device(c, scene, t_p)
    torch.cuda.synchronize()
    sdf = torch.full_like(sdf_alone, float("nan"))
    torch.cuda.synchronize()
    rt.sweep_spheres_device(c, scene, t_o, t_d, t_r, out=out, stream=a.cuda_stream)
    rt.signed_distance_device(c, scene, t_p, sdf=sdf, stream=b.cuda_stream)
    rt.nearest_points_device(c, scene, t_p, out=near, stream=b.cuda_stream)
    rt.sweep_spheres_device(c, scene, t_o, t_d, t_r, out=out, stream=a.cuda_stream)
    torch.cuda.synchronize()
    same(out.cpu().numpy().view(rt.SweepRecord).reshape(-1), ref["free"], "the sweep, two streams")
    got_near = near.cpu().numpy().view(rt.NearestRecord).reshape(-1)
    assert got_near.tobytes() == want_near.tobytes(), "the nearest call, two streams"
    assert sdf.cpu().numpy().tobytes() == sdf_alone.cpu().numpy().tobytes(), "the signed distance, two streams"


# ---- past one chunk per resident wave ---------------------------------------------------------------------------------------------------
REFILL = [Case("random", 13), Case("soup", 0, "hybrid")]
_BASE = {}


@pytest.mark.parametrize("case", REFILL, ids=[c.id for c in REFILL])
def test_refill_past_one_chunk_per_resident_wave(rt, ctx, models_dir, monkeypatch, case):
    """n = 2 * 64 * cus * (max threads per CU / 64) + 37 balls, read from the device, drawn with replacement from a base batch of at most
    3,000 that the yardstick answered: a lane that keeps state of its last ball across a refill gives another record"""
    scene = case.commit(rt, ctx, monkeypatch, models_dir)
    if case.id not in _BASE:
        flat = rt.SceneObjects(case.objs, models_dir).debug_flatten()
        o, d, r = R.query_sweeps(flat, 13, 3000 if case.kind == "random" else 2048)
        io, id_, ir = SS.invalid_balls()
        o, d, r = np.concatenate([o, io]), np.concatenate([d, id_]), np.concatenate([r, ir])
        (free, detail), = R.sweep_many(flat, o, d, r, [None])
        lim = SS.limits_for(detail["key"])
        (limited, _), = R.sweep_many(flat, o, d, r, [lim])
        _BASE[case.id] = (o, d, r, free, lim, limited, R.mesh_winner_share(flat, free))
    o, d, r, free, lim, limited, mesh_share = _BASE[case.id]
    assert mesh_share > 0.1 and (free["object"] < 0).sum() >= 12 and (free["overlap"] == 1).any(), (case.id, mesh_share)
    n = batch_size()
    idx = np.random.default_rng(13).integers(0, o.shape[0], n)
    same(sweep_device(rt, ctx, scene, o[idx], d[idx], r[idx], None), free[idx], case.id + ", no limits")
    same(sweep_device(rt, ctx, scene, o[idx], d[idx], r[idx], lim[idx]), limited[idx], case.id + ", limits")


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    scene = ctx.commit(rt.SceneObjects(SS.objects_of(rt, "three_sphere"), models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(SS.objects_of(rt, "three_sphere"), models_dir))
    pts = torch.zeros((4, 3), dtype=torch.float32, device="cuda:0")
    dirs = torch.ones((4, 3), dtype=torch.float32, device="cuda:0")
    rad = torch.full((4,), 0.1, dtype=torch.float32, device="cuda:0")
    out = torch.full((4 * 48 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p, d, r, o = C.c_void_p(pts.data_ptr()), C.c_void_p(dirs.data_ptr()), C.c_void_p(rad.data_ptr()), C.c_void_p(out.data_ptr())
    f = L.rt_sweep_spheres_device
    assert f(ctx._h, scene._h, p, d, r, None, -1, o, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, scene._h, p, d, r, None, (1 << 30) + 1, o, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, scene._h, None, d, r, None, 4, o, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, scene._h, p, None, r, None, 4, o, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, scene._h, p, d, None, None, 4, o, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, scene._h, p, d, r, None, 4, None, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, scene._h, p, d, r, None, 4, C.c_void_p(out.data_ptr() + 4), None) == rt.RT_ERR_INVALID and "16-byte aligned" in ctx.last_error()
    assert f(ctx._h, foreign._h, p, d, r, None, 4, o, None) == rt.RT_ERR_INVALID and "another context" in ctx.last_error()
    assert f(None, scene._h, p, d, r, None, 4, o, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, None, p, d, r, None, 4, o, None) == rt.RT_ERR_INVALID
    assert f(ctx._h, scene._h, None, None, None, None, 0, None, None) == rt.RT_OK
    torch.cuda.synchronize()
    assert bool((out == 0x77).all()), "a refused call wrote records"
    with pytest.raises(ValueError):
        rt.sweep_spheres_device(ctx, scene, pts.double(), dirs, rad)
    with pytest.raises(ValueError):
        rt.sweep_spheres_device(ctx, scene, pts.data_ptr(), dirs.data_ptr(), rad.data_ptr(), None, out=None, n=4)


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_example_sweep_program(rt, ctx, models_dir, tmp_path):
    """host/example_sweep.cpp (Renderer::sweep_sphere, Renderer::sweep_spheres of host/raytracer.hpp): it builds, its probe and its grid are
    the yardstick's for the same scene, and the PGM has the grid's size"""
    import re
    import subprocess
    exe = rt.build.build_sweep_example()
    W, H, rad = 40, 32, np.float32(0.05)
    pgm = tmp_path / "rest.pgm"
    r = subprocess.run([exe, models_dir, str(W), str(H), "0.05", str(pgm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    objs = [("obj", "low_poly_monkey.obj", [("enlarge", 0.3), ("rotate", 0, 2.3, 0), ("translate", 0.1, -0.1, 1.6)], ("standard", (1, 1, 1), 0.0))]
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    down = np.array([[0, -1, 0]], np.float32)
    want = R.sweep(flat, np.array([[0.1, 1.5, 1.6]], np.float32), down, rad, np.float32(np.inf))[0]
    m = re.search(r"probe: object (-?\d+) triangle (-?\d+) feature (-?\d+) t (\S+) centre (\S+) (\S+) (\S+) point (\S+) (\S+) (\S+)", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (want["object"], want["triangle"], want["feature"]) and want["object"] == 0, (r.stdout, want)
    assert np.float32(m.group(4)) == want["t"] and [np.float32(m.group(k)) for k in (5, 6, 7)] == list(want["centre"]), (r.stdout, want)
    assert [np.float32(m.group(k)) for k in (8, 9, 10)] == list(want["point"]), (r.stdout, want)
    xs = (np.float32(0.1) - np.float32(0.6) + np.float32(1.2) * np.arange(W, dtype=np.float32) / np.float32(W - 1)).astype(np.float32)
    zs = (np.float32(1.6) - np.float32(0.6) + np.float32(1.2) * np.arange(H, dtype=np.float32) / np.float32(H - 1)).astype(np.float32)
    grid = np.stack([np.broadcast_to(xs[None, :], (H, W)), np.full((H, W), 1.5, np.float32), np.broadcast_to(zs[:, None], (H, W))], axis=-1).reshape(-1, 3)
    rest = R.sweep(flat, grid, np.broadcast_to(down, grid.shape), rad, np.float32(3.0))
    landed = rest["object"] >= 0
    m = re.search(r"grid: (\d+) balls, (\d+) land, lowest rest (\S+) highest rest (\S+)", r.stdout)
    assert m and int(m.group(1)) == W * H and int(m.group(2)) == int(landed.sum()) and landed.sum() > 100, (r.stdout, landed.sum())
    assert np.float32(m.group(3)) == rest["centre"][landed, 1].min() and np.float32(m.group(4)) == rest["centre"][landed, 1].max(), r.stdout
    data = pgm.read_bytes()
    assert data.startswith(b"P5\n%d %d\n255\n" % (W, H)) and len(data) == len(b"P5\n%d %d\n255\n" % (W, H)) + W * H
