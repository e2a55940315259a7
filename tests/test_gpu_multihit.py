"""The multi-hit ray queries on the GPU (rt_trace_rays_multi[_device]) against tests/multihit_ref.py, the NumPy binary32 yardstick that
evaluates and sorts every candidate of every ray: every record and every count compared as BYTES.  The one thing the yardstick does not
restate - the u, v of a sphere whose material needs them - is taken from the device for the comparison and held to the oracle instead.

Scenes (tests/multihit_scenes.py): three-sphere, cube, monkey, reference scenes 0 and 4, the two richest seeds of tests/random_scenes.py,
nine meshes of 1 to 9 triangles, a 3,000-triangle mesh read from global memory, soup6k on the hybrid and on the global placement - the
placement asserted from scene.info().  Every shape of RT_SHAPES is forced the way tests/test_gpu_shapes.py forces it, on the smallest scene
that reaches it.  k: the values listed per scene (each overflowed by a tenth of its rays), 8 and count-only.  Limits: per ray, in turn, the
key of one of its candidates, that one ulp down, one ulp up, 0, a negative one, NaN and +Inf - and no limit array at all.
The yardstick's answers are computed once per scene and shared.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import multihit_ref as R
import multihit_scenes as S
from test_gpu_shapes import SHAPES, _id, commit_as, plan, spheres_beyond_lds

pytestmark = pytest.mark.gpu

_WANT = {}
EXTRA = {"spheres_beyond_lds": (1200, 11, (1, 2, 3))}      # reference scene 4 with as many spheres as leave LDS: the one scene of the no-mesh global shape


def objects_of(rt, name):
    if name == "spheres_beyond_lds":
        return rt.scenes.reference_scene4(num_spheres=spheres_beyond_lds(rt))[0]
    return S.objects_of(rt, name)


def ks_of(name):
    return (S.SCENES.get(name) or EXTRA[name])[2]


def reference(rt, models_dir, name):
    if name in EXTRA and name not in S._REFS:
        n, seed, _ = EXTRA[name]
        flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
        o, d = R.query_rays(flat, seed, n)
        S._REFS[name] = {"flat": flat, "o": o, "d": d, "cand": R.candidates(flat, o, d)}
    return S.reference(rt, models_dir, name)


def limits_for(cand):
    """per ray, in turn: the key of one of its candidates (1 where it has none), one ulp down, one ulp up, 0, negative, NaN, +Inf"""
    n = cand.total.shape[0]
    col = (np.arange(n) // 7) % np.maximum(cand.total, 1)
    key = np.where(cand.total > 0, np.take_along_axis(cand.key, col[:, None].astype(np.int64), axis=1)[:, 0], np.float32(1)).astype(np.float32)
    lim = key.copy()
    k = np.arange(n) % 7
    lim[k == 1] = np.nextafter(key[k == 1], np.float32(0))
    lim[k == 2] = np.nextafter(key[k == 2], np.float32(np.inf))
    lim[k == 3] = 0.0
    lim[k == 4] = -0.5
    lim[k == 5] = np.nan
    lim[k == 6] = np.inf
    return lim


def want(rt, models_dir, name, k, limited=False):
    """(hits, counts, sphere_uv) of the yardstick for the scene's rays, kept"""
    key = (name, k, limited)
    if key not in _WANT:
        ref = reference(rt, models_dir, name)
        if limited and "lim" not in ref:
            ref["lim"] = limits_for(ref["cand"])
            ref["cand_lim"] = R.candidates(ref["flat"], ref["o"], ref["d"], ref["lim"])
        _WANT[key] = R.records(ref["flat"], ref["o"], ref["d"], k, ref["cand_lim"] if limited else ref["cand"])
    return _WANT[key]


def same(got, wanted, what):
    hits, counts = got
    w_hits, w_counts, sphere_uv = wanted
    assert counts.dtype == np.int32 and counts.tobytes() == w_counts.tobytes(), (what, "counts differ at", np.nonzero(counts != w_counts)[0][:5])
    w = w_hits.copy()
    w["u"][sphere_uv], w["v"][sphere_uv] = hits["u"][sphere_uv], hits["v"][sphere_uv]
    assert hits.dtype == w.dtype and hits.shape == w.shape and hits.tobytes() == w.tobytes(), (what, "%d of %d records differ, first at %s" % (
        int((hits != w).sum()), hits.size, np.argwhere(hits != w)[:5].tolist()))


def check_scene(rt, ctx, scene, models_dir, name, what, ks=None):
    ref = reference(rt, models_dir, name)
    o, d = ref["o"], ref["d"]
    for k in (ks if ks is not None else tuple(ks_of(name)) + (8, 0)):
        same(rt.trace_rays_multi(ctx, scene, o, d, k), want(rt, models_dir, name, k), "%s, k=%d, no limits" % (what, k))
    k_lim = ks_of(name)[-1]
    for k in (k_lim, 0):
        wanted = want(rt, models_dir, name, k, True)                 # (makes the scene's limits on its first call)
        same(rt.trace_rays_multi(ctx, scene, o, d, k, ref["lim"]), wanted, "%s, k=%d, limits" % (what, k))
    same(rt.trace_rays_multi(ctx, scene, o, d, k_lim, np.float32(np.inf)), want(rt, models_dir, name, k_lim), what + ", +Inf everywhere")
    assert rt.count_hits(ctx, scene, o, d).tobytes() == ref["cand"].total.tobytes(), what + ", count_hits"


# ---- scenes on the placement they pick or are given ---------------------------------------------------------------------------------
PLACED = [("three_sphere", {}, 1), ("cube", {}, 1), ("monkey", {}, 1), ("reference_scene0", {}, 1), ("reference_scene4", {}, 1), ("random13", {}, 1),
          ("random15", {}, 1), ("tiny_meshes", {}, 1), ("soup3000", {"RT_AMD_SCENE_MODE": "0"}, 0), ("soup6k", {}, 2), ("soup6k", {"RT_AMD_SCENE_MODE": "0"}, 0)]


@pytest.mark.parametrize("name,env,mode", PLACED, ids=["%s-%s" % (n, {0: "global", 1: "lds", 2: "hybrid"}[m]) for n, _, m in PLACED])
def test_records_equal_the_yardstick(rt, ctx, models_dir, monkeypatch, name, env, mode):
    scene = commit_as(rt, ctx, monkeypatch, objects_of(rt, name), models_dir, env)
    info = scene.info()
    assert info["scene_in_lds"] == mode, (name, info)
    check_scene(rt, ctx, scene, models_dir, name, "%s %s" % (name, info))


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
    check_scene(rt, ctx, scene, models_dir, name, "%s on %s" % (name, _id(shape)), ks=(ks_of(name)[-1], 8, 0))


# ---- counts around a wave and a chunk -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["monkey", "reference_scene4"])
def test_ray_counts(rt, ctx, models_dir, name):
    flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
    o, d = R.query_rays(flat, 99, 4097)
    cand = R.candidates(flat, o, d)
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    for k in (3, 0):
        w = R.records(flat, o, d, k, cand)
        for n in (1, 63, 64, 65, 4097):
            same(rt.trace_rays_multi(ctx, scene, o[:n], d[:n], k), (w[0][:n], w[1][:n], w[2][:n]), "%s n=%d k=%d" % (name, n, k))
    hits, counts = rt.trace_rays_multi(ctx, scene, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 4)
    assert hits.shape == (0, 4) and counts.shape == (0,)
    assert ctx.last_kernel_ms() > 0.0


# ---- identities on the device's own answers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["monkey", "random13", "reference_scene0", "soup6k"])
def test_prefixes_and_the_closest_hit(rt, orc, ctx, models_dir, name):
    ref = reference(rt, models_dir, name)
    o, d = ref["o"], ref["d"]
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    by_k = {k: rt.trace_rays_multi(ctx, scene, o, d, k) for k in (1, 2, 3, 8)}
    for k1, k2 in ((1, 2), (2, 3), (3, 8), (1, 8)):
        assert by_k[k2][0][:, :k1].tobytes() == by_k[k1][0].tobytes(), (name, k1, k2)
        assert np.array_equal(np.minimum(by_k[k2][1], k1), by_k[k1][1]), (name, k1, k2)
    assert np.array_equal(np.minimum(rt.count_hits(ctx, scene, o, d), 8), by_k[8][1])
    # record 0 under k = 1 is rt_trace_rays' record, outside D
    D = R.set_d(ref["flat"], orc.Scene(objects_of(rt, name), orc.MATH_DET, models_dir), o, d, ref["cand"])
    assert D.mean() <= 0.01, (name, D.mean())
    first, closest = by_k[1][0][:, 0], rt.trace_rays(ctx, scene, o, d)
    assert first[~D].tobytes() == closest[~D].tobytes(), (name, np.nonzero(first != closest)[0][:5])


@pytest.mark.parametrize("name", ["random13", "random15", "soup6k"])
def test_texture_coordinates_equal_the_oracle(rt, orc, ctx, models_dir, name):
    """the u, v of every record that is the first of its object along its ray: trace_one_uv on the oracle scene holding that object alone"""
    ref = reference(rt, models_dir, name)
    o, d, flat = ref["o"], ref["d"], ref["flat"]
    objs = objects_of(rt, name)
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    hits, counts = rt.trace_rays_multi(ctx, scene, o, d, 8)
    checked = 0
    for i in np.nonzero(flat["objects"]["need_uv"] != 0)[0]:
        alone = orc.Scene([objs[i]], orc.MATH_DET, models_dir)
        on = hits["object"] == i
        rays = np.nonzero(on.any(axis=1))[0][:400]
        for r in rays:
            h = hits[r, int(np.argmax(on[r]))]
            hit, out = alone.trace_one_uv(o[r], d[r])
            if not hit or out[0:1].view(np.uint32)[0] != h["t"].view(np.uint32):
                continue                                            # (a tie inside the object: the oracle kept another of its triangles)
            assert np.array([h["u"], h["v"]], np.float32).view(np.uint32).tolist() == out[8:10].view(np.uint32).tolist(), (name, i, r, h, out)
            checked += 1
    assert checked >= 100, (name, checked)


# ---- directions with NaN and zero components -------------------------------------------------------------------------------------------
def test_nan_and_zero_direction_components(rt, ctx, models_dir):
    name = "reference_scene0"
    ref = reference(rt, models_dir, name)
    flat = ref["flat"]
    o, d = ref["o"][:600].copy(), ref["d"][:600].copy()
    d[0::6, 0] = 0.0
    d[1::6, 1] = -0.0
    d[2::6, 2] = 0.0
    d[3::6, 0:2] = 0.0
    d[4::12, 1] = np.nan
    d[10::12] = np.nan
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    cand = R.candidates(flat, o, d)
    assert (cand.total[4::12] == 0).all() and (cand.total[0::6] > 0).any()
    for k in (2, 8, 0):
        same(rt.trace_rays_multi(ctx, scene, o, d, k), R.records(flat, o, d, k, cand), "zero and NaN components, k=%d" % k)


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
    flat = fresh_objs.debug_flatten()
    o, d = R.query_rays(flat, 3, 1500)
    before = rt.trace_rays_multi(ctx, scene, o, d, 4)
    scene.update_mesh_device(1, torch.from_numpy(new).to("cuda:0"))
    after = rt.trace_rays_multi(ctx, scene, o, d, 4)
    fresh = rt.trace_rays_multi(ctx, ctx.commit(fresh_objs), o, d, 4)
    assert after[0].tobytes() == fresh[0].tobytes() and after[1].tobytes() == fresh[1].tobytes(), "updated against a fresh commit"
    same(after, R.records(scene.debug_read(), o, d, 4, R.candidates(scene.debug_read(), o, d)), "updated against the yardstick on the device's scene")
    assert before[0].tobytes() != after[0].tobytes()


# ---- device form: tensors, pointers, a sleeping stream ----------------------------------------------------------------------------------
def test_device_form(rt, ctx, models_dir):
    import torch
    name = "monkey"
    ref = reference(rt, models_dir, name)
    o, d = ref["o"], ref["d"]
    n = o.shape[0]
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    d_o, d_d = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
    hits, counts = rt.trace_rays_multi_device(ctx, scene, d_o, d_d, 3)
    same((hits.cpu().numpy().view(rt.HIT_DTYPE)[..., 0], counts.cpu().numpy()), want(rt, models_dir, name, 3), "tensors")
    want(rt, models_dir, name, 3, True)
    d_lim = torch.from_numpy(ref["lim"]).to("cuda:0")
    buf = torch.full((n, 3, 48), 0xA5, dtype=torch.uint8, device="cuda:0")
    got = rt.trace_rays_multi_device(ctx, scene, d_o, d_d, 3, d_lim, hits=buf)
    assert got[0] is buf
    same((buf.cpu().numpy().view(rt.HIT_DTYPE)[..., 0], got[1].cpu().numpy()), want(rt, models_dir, name, 3, True), "tensors, limits, a buffer of the caller's")
    none, total = rt.trace_rays_multi_device(ctx, scene, d_o, d_d, 0)
    assert none is None and total.cpu().numpy().tobytes() == ref["cand"].total.tobytes()
    buf.fill_(0x5A)
    rt.trace_rays_multi_device(ctx, scene, d_o.data_ptr(), d_d.data_ptr(), 3, hits=buf.data_ptr(), counts=None, n=n)       # no counts: allowed with k > 0
    torch.cuda.synchronize()
    w = want(rt, models_dir, name, 3)
    same((buf.cpu().numpy().view(rt.HIT_DTYPE)[..., 0], w[1]), w, "pointers, no counts")


def test_rays_produced_on_the_stream_just_ahead_of_the_call(rt, models_dir):
    """In the manner of tests/test_gpu_nearest.py: on a sleeping stream the rays are copied into place, the call is queued, the records are
    copied out - the host waits for nothing in between - and the records are those of a synchronised call on a fresh context."""
    import torch
    name = "monkey"
    ref = reference(rt, models_dir, name)
    o, d = ref["o"], ref["d"]
    n, k = o.shape[0], 4
    dev = torch.device("cuda:0")
    fresh = rt.Context(0)
    wanted = rt.trace_rays_multi(fresh, fresh.commit(rt.SceneObjects(objects_of(rt, name), models_dir)), o, d, k)
    same(wanted, want(rt, models_dir, name, k), "the synchronised call")
    c = rt.Context(0)
    scene = c.commit(rt.SceneObjects(objects_of(rt, name), models_dir))
    src_o, src_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    buf_o, buf_d = torch.empty_like(src_o), torch.empty_like(src_d)
    out = torch.empty((n, k, 48), dtype=torch.uint8, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    res, res_cnt = torch.empty_like(out), torch.empty_like(cnt)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rt.trace_rays_multi_device(c, scene, src_o, src_d, k, hits=out, counts=cnt, stream=stream.cuda_stream)      # warm: the kernel is loaded, the stream has its queue
    torch.cuda.synchronize()
    buf_o.fill_(float("nan"))
    buf_d.fill_(float("nan"))
    out.fill_(0xEE)
    cnt.fill_(-7)
    res.fill_(0xEE)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(60000000)
        buf_o.copy_(src_o, non_blocking=True)
        buf_d.copy_(src_d, non_blocking=True)
        rt.trace_rays_multi_device(c, scene, buf_o, buf_d, k, hits=out, counts=cnt, stream=stream.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(stream)
        pending = not ev.query()
        res.copy_(out, non_blocking=True)
        res_cnt.copy_(cnt, non_blocking=True)
    torch.cuda.synchronize()
    assert pending, "the stream had run dry before the call returned: the window was not open"
    got = res.cpu().numpy().view(rt.HIT_DTYPE)[..., 0]
    assert got.tobytes() == wanted[0].tobytes() and res_cnt.cpu().numpy().tobytes() == wanted[1].tobytes(), "queued behind the producer of its rays"


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(rt, ctx, models_dir):
    import torch
    L = rt.lib()
    scene = ctx.commit(rt.SceneObjects(objects_of(rt, "three_sphere"), models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objects_of(rt, "three_sphere"), models_dir))
    rays = torch.zeros((4, 3), dtype=torch.float32, device="cuda:0")
    out = torch.full((4 * 2 * 48 + 16,), 0x77, dtype=torch.uint8, device="cuda:0")
    cnt = torch.full((4,), -3, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p, h, c = C.c_void_p(rays.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr())
    dev = L.rt_trace_rays_multi_device
    bad = rt.RT_ERR_INVALID
    assert dev(ctx._h, scene._h, p, p, None, -1, 2, h, c, None) == bad and dev(ctx._h, scene._h, p, p, None, (1 << 30) + 1, 2, h, c, None) == bad
    assert dev(ctx._h, scene._h, p, p, None, 4, -1, h, c, None) == bad and dev(ctx._h, scene._h, p, p, None, 4, 9, h, c, None) == bad
    assert dev(ctx._h, scene._h, None, p, None, 4, 2, h, c, None) == bad and dev(ctx._h, scene._h, p, None, None, 4, 2, h, c, None) == bad
    assert dev(ctx._h, scene._h, p, p, None, 4, 2, None, c, None) == bad
    assert dev(ctx._h, scene._h, p, p, None, 4, 2, C.c_void_p(out.data_ptr() + 4), c, None) == bad and "16-byte aligned" in ctx.last_error()
    assert dev(ctx._h, scene._h, p, p, None, 4, 0, h, None, None) == bad and "null counts" in ctx.last_error()
    assert dev(ctx._h, foreign._h, p, p, None, 4, 2, h, c, None) == bad and "another context" in ctx.last_error()
    assert dev(None, scene._h, p, p, None, 4, 2, h, c, None) == bad and dev(ctx._h, None, p, p, None, 4, 2, h, c, None) == bad
    assert dev(ctx._h, scene._h, None, None, None, 0, 2, None, None, None) == rt.RT_OK
    torch.cuda.synchronize()
    assert bool((out == 0x77).all()) and bool((cnt == -3).all()), "a refused call wrote"
    with pytest.raises(ValueError):
        rt.trace_rays_multi(ctx, scene, np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32), 9)
    with pytest.raises(ValueError):
        rt.trace_rays_multi_device(ctx, scene, rays.double(), rays, 2)


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_example_xray_program(rt, ctx, models_dir, tmp_path):
    """host/example_xray.cpp (Renderer::count_hits, Renderer::trace_rays_multi of host/raytracer.hpp): it builds, its centre ray and its
    totals are the yardstick's for the same scene and rays, and the PGM holds min(count, 8) * 32 per pixel"""
    import re
    import subprocess
    exe = rt.build.build_xray_example()
    W, H = 48, 40
    pgm = tmp_path / "xray.pgm"
    r = subprocess.run([exe, models_dir, str(W), str(H), str(pgm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    objs = [("obj", "low_poly_monkey.obj", [("enlarge", 0.3), ("rotate", 0, 2.3, 0), ("translate", 0.1, -0.1, 1.6)], ("standard", (1, 1, 1), 0.0))]
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    cam = rt.Camera(W, H)
    d = rt.render_aov(ctx, ctx.commit(rt.SceneObjects(objs, models_dir)), cam, planes=("ray",))["ray"].reshape(-1, 3)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(cam.floats()[0:3], np.float32), d.shape))
    cand = R.candidates(flat, o, d)
    hits, counts, _ = R.records(flat, o, d, 4, cand)
    centre = (H // 2) * W + W // 2
    m = re.search(r"centre: (\d+) hits:((?: \S+ \(triangle -?\d+\))*)", r.stdout)
    assert m and int(m.group(1)) == cand.total[centre], (r.stdout, cand.total[centre])
    listed = re.findall(r" (\S+) \(triangle (-?\d+)\)", m.group(2))
    assert [(np.float32(t), int(tri)) for t, tri in listed] == [(hits["t"][centre, q], int(hits["triangle"][centre, q])) for q in range(counts[centre])], (r.stdout, hits[centre])
    m = re.search(r"view: (\d+) rays, (\d+) meet nothing, most surfaces (\d+), (\d+) surfaces in all", r.stdout)
    assert m and [int(x) for x in m.groups()] == [W * H, int((cand.total == 0).sum()), int(cand.total.max()), int(cand.total.sum())], (r.stdout,)
    data = pgm.read_bytes()
    head = b"P5\n%d %d\n255\n" % (W, H)
    assert data.startswith(head) and data[len(head):] == bytes(255 if c >= 8 else c * 32 for c in cand.total.tolist())
