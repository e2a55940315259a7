"""Closest-hit ray queries (rt_trace_rays) and the first-hit AOV planes (rt_render_aov) against the CPU oracle's orc_trace_one and
render: equal bits (uint32 views), never a tolerance.  Run with -m gpu on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISS_T = np.float32(1073741824.0)
SCENES = ["three_sphere", "cube", "monkey", "reference_scene0", "reference_scene1", "reference_scene2", "reference_scene3", "soup6k", "sphere50k"]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rays(n, seed, target=(0.0, 0.0, 2.0), spread=3.0):
    """tests/test_host.py::_rays' construction: half the origins at 0, half scattered around the target (inside and outside the
    scene), every ray aimed at a point scattered around the target"""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), np.float32)
    o[n // 2:] = (rng.normal(size=(n - n // 2, 3)) * 0.8 + np.array(target)).astype(np.float32)
    t = (rng.normal(size=(n, 3)) * spread * 0.4 + np.array(target)).astype(np.float32)
    d = (t - o).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def primaries(cam_floats, W, H):
    """the renderer's primary rays with antialiasing off, in float32 with the kernel's operation order:
    normalised((tl + (du * px + dv * py)) - cam_pos), normalised = a * (1 / sqrt((x*x + y*y) + z*z))"""
    F = np.float32
    c = np.asarray(cam_floats, F)
    pos, tl, du, dv = c[0:3], c[3:6], c[6:9], c[9:12]
    px = np.arange(W, dtype=np.int32)[None, :, None].astype(F)
    py = np.arange(H, dtype=np.int32)[:, None, None].astype(F)
    plane_point = (du[None, None, :] * px).astype(F) + (dv[None, None, :] * py).astype(F)
    a = ((tl[None, None, :] + plane_point).astype(F) - pos[None, None, :]).astype(F)
    sq = (a * a).astype(F)
    m = ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)
    inv = (F(1.0) / np.sqrt(m).astype(F)).astype(F)
    return (a * inv[..., None]).astype(F)


def oracle_records(oracle, origins, dirs):
    n = len(origins)
    hit = np.zeros(n, bool)
    out = np.zeros((n, 8), np.float32)
    for i in range(n):
        hit[i], out[i] = oracle.trace_one(origins[i], dirs[i])
    return hit, out


def assert_equal_to_oracle(hits, ohit, oout, what=""):
    """every ray is compared: the hit flag; for hits distance, point, normal as uint32 and the object index; misses the miss record"""
    got_hit = hits["object"] >= 0
    assert np.array_equal(got_hit, ohit), (what, int((got_hit != ohit).sum()))
    h = ohit
    assert np.array_equal(u32(hits["t"][h]), u32(oout[h, 0])), what
    assert np.array_equal(u32(hits["point"][h]), u32(oout[h, 1:4])), what
    assert np.array_equal(u32(hits["normal"][h]), u32(oout[h, 4:7])), what
    assert np.array_equal(hits["object"][h], oout[h, 7].astype(np.int32)), what
    assert_miss_records(hits[~h], what)


def assert_miss_records(m, what=""):
    assert np.all(u32(m["t"]) == u32(MISS_T)) and not u32(m["point"]).any() and not u32(m["normal"]).any(), what
    assert np.all(m["object"] == -1) and np.all(m["triangle"] == -1), what
    assert not u32(m["u"]).any() and not u32(m["v"]).any() and not m["reserved"].any(), what


def assert_triangles_and_uv(rt, objs, models_dir, o, d, hits, what="", sample=600):
    """rt_hit.triangle, u, v of the hits against the flattened layout (rt_debug_flatten), independently of the kernel: the index is -1 iff the object
    is a sphere, else it names a triangle of that object, and the emulator's triangle test (tests/flat_emulator.py) on that very triangle hits at
    the record's distance, bit for bit; u, v are 0 unless the object's material needs them, and for a triangle that does they are the
    barycentric blend of its texture coordinates (Triangle::assign_texture_coords, float32, the kernel's operation order)"""
    from flat_emulator import FlatScene, tri_test, _cross, _dot
    F = np.float32
    flat = rt.SceneObjects(objs, models_dir).debug_flatten()
    fs = FlatScene(flat)
    ob = flat["objects"]
    hit = hits["object"] >= 0
    typ = np.where(hit, ob["type"][np.maximum(hits["object"], 0)], -1)
    assert np.array_equal(hits["triangle"][hit] == -1, typ[hit] == 0), what                       # 0: RT_OBJ_SPHERE
    assert np.all((hits["triangle"][hit] >= -1) & (hits["triangle"][hit] < flat["num_triangles"])), what
    need = np.where(hit, ob["need_uv"][np.maximum(hits["object"], 0)], 0) != 0
    assert not u32(hits["u"][~need]).any() and not u32(hits["v"][~need]).any(), what
    span = {1: 1, 2: 2, 3: 2, 4: 12}                                                              # triangle, quad, one-way quad, cuboid
    idx = np.flatnonzero(hit & (typ != 0))
    if len(idx) > sample:
        idx = np.random.default_rng(8).choice(idx, sample, replace=False)
    for i in idx:
        t = int(hits["triangle"][i])
        k = int(hits["object"][i])
        if int(typ[i]) in span:
            assert ob["prim_start"][k] <= t < ob["prim_start"][k] + span[int(typ[i])], (what, i)
        ok, dist = tri_test(fs.tris, t, o[i].astype(F), d[i].astype(F))
        assert ok and u32(F(dist)) == u32(hits["t"][i]), (what, i, t)
        if need[i]:
            q = fs.tris[3 * t:3 * t + 3].reshape(12)
            p0, s1, s2 = q[0:3], q[3:6], q[6:9]
            pv = _cross(d[i], s2)
            inv_det = F(F(1) / _dot(s1, pv))
            tv = (o[i] - p0).astype(F)
            bu = F(_dot(tv, pv) * inv_det)
            bv = F(_dot(d[i], _cross(tv, s1)) * inv_det)
            bw = F(F(F(1) - bu) - bv)
            uv = flat["tri_uv"][t]
            want_u = F(F(F(uv[0] * bw) + F(uv[2] * bu)) + F(uv[4] * bv))
            want_v = F(F(F(uv[1] * bw) + F(uv[3] * bu)) + F(uv[5] * bv))
            assert u32(want_u) == u32(hits["u"][i]) and u32(want_v) == u32(hits["v"][i]), (what, i)
    return len(idx)


def scene_rays(rt, n=2000, W=40, H=30):
    o, d = _rays(n, 5)
    cam = rt.Camera(W, H).floats()
    p = primaries(cam, W, H).reshape(-1, 3)
    return np.concatenate([o, np.broadcast_to(np.asarray(cam[0:3], np.float32), p.shape)]).astype(np.float32), np.concatenate([d, p]).astype(np.float32), n


def check_scene(rt, orc, ctx, models_dir, name):
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    o, d, n_random = scene_rays(rt)
    hits = rt.trace_rays(ctx, scene, o, d)
    ohit, oout = oracle_records(oracle, o, d)
    # conditions on the generator, from the oracle alone: a batch that is nearly all hits or all misses would test little
    frac = ohit[:n_random].mean()
    print("%s: %d rays, oracle hits %.1f %% of the random ones, placement %d" % (name, len(o), 100 * frac, scene.info()["scene_in_lds"]))
    assert 0.25 <= frac <= 0.90, (name, frac)
    assert_equal_to_oracle(hits, ohit, oout, name)
    checked = assert_triangles_and_uv(rt, objs, models_dir, o, d, hits, name)
    assert checked > 0 or name == "three_sphere", name                  # (a scene of spheres alone has no triangle to name)
    return scene.info()["scene_in_lds"]


@pytest.mark.parametrize("name", [s for s in SCENES if s not in ("soup6k", "sphere50k")])
def test_queries_equal_the_oracle(rt, orc, ctx, models_dir, name):
    assert check_scene(rt, orc, ctx, models_dir, name) == 1          # the whole scene in LDS


def test_queries_equal_the_oracle_beyond_lds(rt, orc, ctx, models_dir):
    """soup6k and sphere50k: the placements beyond LDS.  Between them HYBRID (2) and GLOBAL (0) must both run; a placement the committed
    shapes do not pick is forced with RT_AMD_SCENE_MODE in a child process (the knob is read when a scene is committed)."""
    modes = {name: check_scene(rt, orc, ctx, models_dir, name) for name in ("soup6k", "sphere50k")}
    assert all(m in (0, 2) for m in modes.values()), modes
    missing = {0, 2} - set(modes.values())
    assert 2 not in missing, ("no scene runs the hybrid placement", modes)
    if 0 in missing:
        env = dict(os.environ, RT_AMD_SCENE_MODE="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "soup6k"], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "placement 0" in r.stdout and "child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


TIE_SCENE = [
    ("quad", (-1, -0.5, 1), (1, -0.5, 1), (1, -0.5, 3), (-1, -0.5, 3), ("checkerboard", (0.9, 0.9, 0.9), (0.2, 0.2, 0.2), 6, 0.1)),
    ("one_way_quad", (-1, 1, 0.5), (1, 1, 0.5), (1, -1, 0.5), (-1, -1, 0.5), False, ("standard", (1, 1, 1), 0)),
    ("one_way_quad", (-1, 1, 3.2), (1, 1, 3.2), (1, -1, 3.2), (-1, -1, 3.2), True, ("standard", (0.4, 0.8, 0.4), 0)),
    ("cuboid", (-0.3, 0.3, 1.6), 0.6, 0.5, 0.4, ("standard", (0.8, 0.3, 0.3), 0.5)),
    ("triangle_uv", [(-0.9, 0.9, 2.5), (0.9, 0.9, 2.5), (0.0, -0.2, 2.0)], [(0, 0), (1, 0), (0.5, 1)], ("gradient", 0)),
    ("triangle", (-0.9, 0.9, 2.5), (0.9, 0.9, 2.5), (0.0, -0.2, 2.0), ("standard", (0.2, 0.2, 0.9), 0)),    # coincident: wins the tie
    ("sphere", (0.5, -0.2, 1.4), 0.2, ("emissive", (1, 0.9, 0.8), 4)),
    ("sphere", (0.5, -0.2, 1.4), 0.2, ("standard", (0.5, 0.5, 0.5), 1)),                                      # coincident sphere: wins
]


@pytest.mark.parametrize("name", ["monkey", "reference_scene1"])
def test_edge_rays(rt, orc, ctx, models_dir, name):
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    nan = np.float32(np.nan)
    sub = np.float32(1e-41)          # subnormal
    rays = [
        ((0, 0, 0), (0, 0.3, 1)), ((0.1, -0.1, 0), (0, 0, 1)), ((0.1, 0, 0), (0, 0, 1)), ((0, 0, 1.7), (1, 0, 0)), ((0, 0, 1.7), (0, -1, 0)),   # one / two zero components
        ((0.1, -0.1, 0), (sub, 0.05, 1)), ((0, 0, 0), (0.1, sub, 1)),                                                                        # a subnormal component
        ((0, 0, 0), (nan, nan, nan)), ((0.1, -0.1, 1.0), (nan, nan, nan)),                                                                    # all NaN: a miss
        ((0, 0, 0), (0.3, -0.3, 3 * 0.9055385)), ((0, 0, 0), (0.1, -0.1, 1)),                                                                 # length ~3 and the same direction shorter
        ((0.2, -0.5, 1.9), (0.1, 1, 0.2)), ((0.2, -0.5, 1.9), (0.1, -1, 0.2)), ((-0.5, 0.1, 1.5), (1, 0.2, 0.3)),                             # origins lying on the floor / the left wall (quads)
    ]
    o = np.array([r[0] for r in rays], np.float32)
    d = np.array([r[1] for r in rays], np.float32)
    hits = rt.trace_rays(ctx, scene, o, d)
    ohit, oout = oracle_records(oracle, o, d)
    assert_equal_to_oracle(hits, ohit, oout, name)
    assert not ohit[7] and not ohit[8]                               # NaN directions
    assert ohit[:5].any() and ohit[9] and ohit[10]
    # an un-normalised direction: the same object, the distance scales with 1 / length
    u = (d[9] / np.float32(3.0)).astype(np.float32)
    h3, h1 = rt.trace_rays(ctx, scene, o[9:10], d[9:10])[0], rt.trace_rays(ctx, scene, o[9:10], u[None])[0]
    assert h3["object"] == h1["object"] and abs(float(h3["t"]) * 3.0 / float(h1["t"]) - 1.0) < 1e-5


def test_tie_rules(rt, orc, ctx, models_dir):
    """coincident objects (the later one wins, `<=`), one-way quads, the cuboid's strict <: rays through every part of the tie scene"""
    scene = ctx.commit(rt.SceneObjects(TIE_SCENE, models_dir))
    oracle = orc.Scene(TIE_SCENE, orc.MATH_DET, models_dir)
    cam = rt.Camera(96, 72).floats()
    d = primaries(cam, 96, 72).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(cam[0:3], np.float32), d.shape).copy()
    o2, d2 = _rays(1500, 7, target=(0.0, 0.2, 2.0), spread=2.0)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    hits = rt.trace_rays(ctx, scene, o, d)
    ohit, oout = oracle_records(oracle, o, d)
    assert_equal_to_oracle(hits, ohit, oout, "tie scene")
    assert assert_triangles_and_uv(rt, TIE_SCENE, models_dir, o, d, hits, "tie scene", sample=2000) > 500
    assert (hits["object"] == 4).sum() == 0 and ((hits["object"] == 0) & (hits["u"] != 0)).any()       # the textured quad's coordinates are there
    won = set(hits["object"].tolist())
    assert 5 in won and 7 in won and 4 not in won and 6 not in won           # the later of two coincident objects, never the earlier


def test_batch_shape_does_not_matter(rt, orc, ctx, models_dir):
    objs, _ = rt.scenes.monkey()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    n = 2 ** 20 + 17
    o, d = _rays(n, 11)
    big = rt.trace_rays(ctx, scene, o, d)
    perm = np.random.default_rng(3).permutation(n)
    shuffled = rt.trace_rays(ctx, scene, o[perm], d[perm])
    back = np.empty_like(shuffled)
    back[perm] = shuffled
    assert big.tobytes() == back.tobytes()
    for k in (1, 63, 64, 65):
        assert rt.trace_rays(ctx, scene, o[:k], d[:k]).tobytes() == big[:k].tobytes(), k
    pick = np.random.default_rng(4).choice(n, 4096, replace=False)
    ohit, oout = oracle_records(orc.Scene(objs, orc.MATH_DET, models_dir), o[pick], d[pick])
    assert_equal_to_oracle(big[pick], ohit, oout, "subsample")
    assert rt.trace_rays(ctx, scene, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0,)


@pytest.mark.parametrize("name", ["monkey", "reference_scene0", "reference_scene2"])
@pytest.mark.parametrize("W,H", [(160, 120), (67, 45)])
def test_aov_planes(rt, orc, ctx, models_dir, name, W, H):
    import torch
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    cam = rt.Camera(W, H)
    sky = (0.25, 0.5, 0.75)
    aov = rt.render_aov(ctx, scene, cam, sky)
    assert sorted(aov) == sorted(rt.AOV_PLANES)
    # (a) the ray plane is the primary-ray expression
    assert np.array_equal(u32(aov["ray"]), u32(primaries(cam.floats(), W, H)))
    # (b) the oracle on exactly these rays
    d = aov["ray"].reshape(-1, 3)
    o = np.broadcast_to(np.asarray(cam.floats()[0:3], np.float32), d.shape)
    ohit, oout = oracle_records(oracle, o, d)
    obj = aov["object"].reshape(-1)
    assert np.array_equal(obj >= 0, ohit) and np.array_equal(obj[ohit], oout[ohit, 7].astype(np.int32))
    depth, normal, albedo = aov["depth"].reshape(-1), aov["normal"].reshape(-1, 3), aov["albedo"].reshape(-1, 3)
    assert np.array_equal(u32(depth[ohit]), u32(oout[ohit, 0])) and np.all(u32(depth[~ohit]) == u32(MISS_T))
    assert np.array_equal(u32(normal[ohit]), u32(oout[ohit, 4:7])) and not u32(normal[~ohit]).any()
    assert np.all(obj[~ohit] == -1) and np.array_equal(u32(albedo[~ohit]), u32(np.broadcast_to(np.float32(sky), albedo[~ohit].shape)))
    # ... and the query entry point on them gives the same records
    hits = rt.trace_rays(ctx, scene, o, d)
    assert np.array_equal(u32(hits["t"]), u32(depth)) and np.array_equal(hits["object"], obj) and np.array_equal(u32(hits["normal"]), u32(normal))
    # (c) a subset of planes: the same bits
    part = rt.render_aov(ctx, scene, cam, sky, planes=("depth", "object"))
    assert sorted(part) == ["depth", "object"] and part["depth"].tobytes() == aov["depth"].tobytes() and part["object"].tobytes() == aov["object"].tobytes()
    one = rt.render_aov(ctx, scene, cam, sky, planes=("albedo",))
    assert list(one) == ["albedo"] and one["albedo"].tobytes() == aov["albedo"].tobytes()
    # (d) the device form into torch tensors
    dev = torch.device("cuda:0")
    t = {"depth": torch.full((H, W), -1.0, device=dev), "normal": torch.full((H, W, 3), -1.0, device=dev), "albedo": torch.full((H, W, 3), -1.0, device=dev),
         "object": torch.full((H, W), -7, dtype=torch.int32, device=dev), "ray": torch.full((H, W, 3), -1.0, device=dev)}
    torch.cuda.synchronize()
    rt.render_aov_device(ctx, scene, cam, sky, **{"d_" + k: v.data_ptr() for k, v in t.items()})
    ctx.synchronize()
    for k, v in t.items():
        assert v.cpu().numpy().tobytes() == aov[k].tobytes(), k
    assert ctx.last_kernel_ms() > 0
    # trace_rays_device on device tensors
    n = d.shape[0]
    t_o, t_d = torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev)
    t_h = torch.zeros(n * rt.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rt.trace_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), n, t_h.data_ptr())
    ctx.synchronize()
    assert t_h.cpu().numpy().tobytes() == hits.tobytes()


@pytest.mark.parametrize("name", ["monkey", "reference_scene0", "reference_scene2", "reference_scene3"])
def test_albedo_is_the_one_bounce_render(rt, ctx, models_dir, name):
    """sky (1,1,1), 1 spp, reflection limit 1, antialias off, frame 0: trace_ray adds sky * 1 on a miss, emitted * 1 on an emissive hit and
    nothing else, so the frame equals the albedo plane there and is 0 elsewhere"""
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    W, H = 160, 120
    cam = rt.Camera(W, H)
    data = rt.VariableRenderData(W, H)
    rt.render(ctx, scene, cam, rt.RenderData(1, 1, False, (1.0, 1.0, 1.0)), data, 4242)
    frame = data.previous_render.reshape(H, W, 3)
    aov = rt.render_aov(ctx, scene, cam, (1.0, 1.0, 1.0), planes=("albedo", "object"))
    emissive = np.array([o[-1][0] == "emissive" for o in objs] + [False])
    lit = (aov["object"] < 0) | emissive[aov["object"]]
    assert lit.any() and (~lit).any()
    assert np.array_equal(u32(frame[lit]), u32(aov["albedo"][lit])) and not u32(frame[~lit]).any()


LONE = {"sphere": ("sphere", (0, 0, 1.5), 0.5), "quad": ("quad", (-0.5, 0.5, 1.5), (0.5, 0.5, 1.5), (0.5, -0.5, 1.7), (-0.5, -0.5, 1.7))}


@pytest.mark.parametrize("shape", ["sphere", "quad"])
@pytest.mark.parametrize("material", ["checkerboard", "gradient", "image"])
def test_albedo_of_a_lone_convex_object_is_the_oracle_frame(rt, orc, ctx, models_dir, shape, material):
    """one convex object alone: the second ray always escapes to the sky (1,1,1), so the oracle's 1-spp, limit-2 frame is 1 * c * 1 = the
    texture colour at the first hit, on every pixel"""
    img = np.random.default_rng(1).random((5, 7, 3)).astype(np.float32)
    mat = {"checkerboard": ("checkerboard", (0.9, 0.8, 0.1), (0.1, 0.2, 0.3), 8, 0.0), "gradient": ("gradient", 0.5), "image": ("image", img, 0.2)}[material]
    objs = [LONE[shape] + (mat,)]
    W, H = 160, 120
    cam = rt.Camera(W, H)
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    frames = [oracle.render(cam.floats(), W, H, 1, 2, (1, 1, 1), time_ms=t, antialias=False) for t in (12345, 999)]
    # the three facts about the oracle frame this test rests on
    assert np.array_equal(u32(frames[0]), u32(frames[1]))                      # no second ray ever lands
    flat = frames[0].reshape(-1, 3)
    sky = (flat == 1).all(axis=1)
    assert 0.3 < sky.mean() < 0.9
    colours = len(np.unique(flat[~sky], axis=0))
    assert colours == 2 if material == "checkerboard" else (colours > 1000 if material == "gradient" else 2 <= colours <= 35), colours
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    aov = rt.render_aov(ctx, scene, cam, (1.0, 1.0, 1.0), planes=("albedo", "object"))
    assert np.array_equal(aov["object"].reshape(-1) < 0, sky)
    assert np.array_equal(u32(aov["albedo"]), u32(frames[0]))


def test_errors_leave_the_context_usable(rt, ctx, models_dir):
    import ctypes as C
    L = rt.lib()
    objs, _ = rt.scenes.three_sphere()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objs, models_dir))
    o, d = _rays(64, 1)
    hits = np.zeros(64, rt.HIT_DTYPE)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
    good = rt.trace_rays(ctx, scene, o, d)

    def usable():
        assert rt.trace_rays(ctx, scene, o, d).tobytes() == good.tobytes()

    for args, msg in [((ctx._h, scene._h, fp(o), fp(d), -1, C.c_void_p(hits.ctypes.data)), "ray count"),
                      ((ctx._h, scene._h, None, fp(d), 64, C.c_void_p(hits.ctypes.data)), "null"),
                      ((ctx._h, scene._h, fp(o), None, 64, C.c_void_p(hits.ctypes.data)), "null"),
                      ((ctx._h, scene._h, fp(o), fp(d), 64, None), "null"),
                      ((ctx._h, foreign._h, fp(o), fp(d), 64, C.c_void_p(hits.ctypes.data)), "another context"),
                      ((ctx._h, None, fp(o), fp(d), 64, C.c_void_p(hits.ctypes.data)), "null")]:
        assert L.rt_trace_rays(*args) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        usable()
    assert L.rt_trace_rays_device(ctx._h, scene._h, None, None, 5, None, None) == rt.RT_ERR_INVALID
    assert L.rt_trace_rays_device(ctx._h, scene._h, None, None, -5, None, None) == rt.RT_ERR_INVALID
    # n == 0 succeeds and touches nothing, null pointers included
    assert L.rt_trace_rays(ctx._h, scene._h, None, None, 0, None) == rt.RT_OK
    assert L.rt_trace_rays_device(ctx._h, scene._h, None, None, 0, None, None) == rt.RT_OK
    usable()
    cam = rt.Camera(32, 24)
    sky = np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="no plane"):
        rt.render_aov(ctx, scene, cam, planes=())
    assert L.rt_render_aov_device(ctx._h, scene._h, C.byref(cam.c), fp(sky), None, None, None, None, None, None) == rt.RT_ERR_INVALID
    with pytest.raises(ValueError, match="another context"):
        rt.render_aov(ctx, foreign, cam)
    depth = np.zeros((24, 32), np.float32)
    assert L.rt_render_aov(ctx._h, scene._h, None, fp(sky), fp(depth), None, None, None, None) == rt.RT_ERR_INVALID
    with pytest.raises(ValueError):
        rt.render_aov(ctx, scene, cam, planes=("depth", "colour"))
    usable()
    assert rt.render_aov(ctx, scene, cam, planes=("depth",))["depth"].shape == (24, 32)
    # the render entry points still work on this context after all of the above
    data = rt.VariableRenderData(32, 24)
    rt.render(ctx, scene, cam, rt.RenderData(2, 3, True, (0.8, 1.0, 1.0)), data, 1)
    assert data.frame_num == 1


def test_cpp_query_example(rt, orc, models_dir, tmp_path):
    """host/raytracer.hpp's trace_ray / trace_rays / render_aov through host/example_query.cpp, against the oracle"""
    import re
    bmod = __import__("importlib").import_module("ray-tracer_amd.build")
    exe = bmod.build_query_example()
    W, H = 80, 64
    for scene_num, name in ((0, "reference_scene0"), (1, "reference_scene1"), (3, "reference_scene3")):
        out = tmp_path / ("depth%d.pgm" % scene_num)
        text = subprocess.check_output([exe, models_dir, str(scene_num), str(W), str(H), str(out)], timeout=300, cwd=str(tmp_path), text=True)
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
        cam = rt.Camera(W, H).floats()
        d = primaries(cam, W, H)
        origin = np.asarray(cam[0:3], np.float32)
        hit, want = oracle.trace_one(origin, d[H // 2, W // 2])
        m = re.search(r"centre ray: object (-?\d+) triangle (-?\d+) t (\S+) point (\S+) (\S+) (\S+) normal (\S+) (\S+) (\S+)", text)
        assert m and hit and int(m.group(1)) == int(want[7])
        got = np.array([float(x) for x in m.groups()[2:]], np.float32)          # %.9g round-trips a binary32
        assert np.array_equal(u32(got), u32(want[:7]))
        phit, pwant = oracle.trace_one((0, 0, 0), (0, 0, 2))
        m = re.search(r"probe: object (-?\d+) t (\S+)", text)
        assert m and phit and int(m.group(1)) == int(pwant[7]) and u32(np.float32(float(m.group(2)))) == u32(pwant[0])
        ohit, oout = oracle_records(oracle, np.broadcast_to(origin, (W * H, 3)), d.reshape(-1, 3))
        m = re.search(r"planes: (\d+) of (\d+) pixels hit, nearest (\S+) farthest (\S+)", text)
        assert m and int(m.group(1)) == int(ohit.sum()) and int(m.group(2)) == W * H
        assert u32(np.float32(float(m.group(3)))) == u32(oout[ohit, 0].min()) and u32(np.float32(float(m.group(4)))) == u32(oout[ohit, 0].max())
        raw = out.read_bytes()
        header = ("P5\n%d %d\n255\n" % (W, H)).encode()
        assert raw.startswith(header) and len(raw) == len(header) + W * H
        grey = np.frombuffer(raw[len(header):], np.uint8)
        assert not grey[~ohit].any() and grey[int(np.argmin(np.where(ohit, oout[:, 0], np.inf)))] == 255


if __name__ == "__main__":
    # child of test_queries_equal_the_oracle_beyond_lds: one scene under the environment's placement knob
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    _rt = importlib.import_module("ray-tracer_amd")
    from oracle import binding as _orc
    _orc.build()
    check_scene(_rt, _orc, _rt.Context(0), _rt.scenes.models_dir(), sys.argv[1])
    print("child ok")
