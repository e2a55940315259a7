"""Occlusion (any-hit) ray queries (rt_occluded_rays) and the light-visibility plane (rt_render_visibility) against the CPU oracle's
orc_trace_one: expected = `hit and t <= tmax` in float32 for EVERY ray and pixel, compared as bytes, never to a tolerance and never on a
sample.  The limits are built from the oracle's own distances, so the boundary t == tmax is hit exactly.  Run with -m gpu on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_query import SCENES, _rays, primaries, u32

pytestmark = pytest.mark.gpu

F = np.float32
MISS_T = F(1073741824.0)
N_BASE = 1999                      # not a multiple of 64
# per scene: where test_gpu_query._rays aims and how widely, chosen so that the oracle answers "occluded" for 10-90 % of the base batch
# (asserted below from the oracle alone); the default is that file's
AIM = {}


def oracle_hits(oracle, o, d):
    """(hit flags, distances) of orc_trace_one for every ray"""
    n = len(o)
    hit, t, obj = np.zeros(n, bool), np.zeros(n, F), np.full(n, -1, np.int32)
    for i in range(n):
        h, out = oracle.trace_one(o[i], d[i])
        hit[i], t[i] = h, out[0]
        if h:
            obj[i] = int(out[7])
    return hit, t, obj


def expected(hit, t, tmax):
    """occluded := the oracle finds a hit AND its distance t <= tmax, in float32 (a NaN limit compares false)"""
    with np.errstate(invalid="ignore"):
        return (hit & (t.astype(F) <= np.asarray(tmax, F))).astype(np.uint8)


def limit_sets(hit, t):
    """the per-ray limits, from the oracle's own distances (a miss gets limits around 1)"""
    base = np.where(hit, t, F(1.0)).astype(F)
    n = len(base)
    return {
        "t": base,                                                     # equality: occluded
        "below t": np.nextafter(base, F(0.0)).astype(F),               # not occluded
        "above t": np.nextafter(base, F(np.inf)).astype(F),
        "t / 2": (base / F(2.0)).astype(F),
        "MISS_T": np.full(n, MISS_T, F),
        "+inf": np.full(n, np.inf, F),
        "NaN": np.full(n, np.nan, F),
        "0": np.zeros(n, F),
        "negative": np.full(n, -1.5, F),
    }


def check_batch(rt, ctx, scene, o, d, hit, t, what):
    """every limit set and NULL on one batch; returns the number of bytes compared"""
    compared = 0
    got = rt.occluded_rays(ctx, scene, o, d)                           # tmax = NULL: any hit at all
    assert got.dtype == np.uint8 and got.shape == (len(o),)
    assert got.tobytes() == hit.astype(np.uint8).tobytes(), (what, "NULL", int((got != hit).sum()))
    compared += len(o)
    for name, tmax in limit_sets(hit, t).items():
        got = rt.occluded_rays(ctx, scene, o, d, tmax)
        want = expected(hit, t, tmax)
        assert got.tobytes() == want.tobytes(), (what, name, int((got != want).sum()))
        compared += len(o)
    # the sets are what they claim to be
    sets = limit_sets(hit, t)
    assert np.array_equal(expected(hit, t, sets["t"]), hit.astype(np.uint8)) and not expected(hit, t, sets["below t"]).any()
    assert not expected(hit, t, sets["NaN"]).any() and np.array_equal(expected(hit, t, sets["+inf"]), hit.astype(np.uint8))
    return compared


def check_scene(rt, orc, ctx, models_dir, name):
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    o, d = _rays(N_BASE, 5, **AIM.get(name, {}))
    hit, t, _ = oracle_hits(oracle, o, d)
    # condition on the inputs, from the oracle alone: a batch that is nearly all occluded or all free would test little
    frac = hit.mean()
    print("%s: %d rays, oracle: %.1f %% occluded with no limit, placement %d" % (name, len(o), 100 * frac, scene.info()["scene_in_lds"]))
    assert 0.10 <= frac <= 0.90, (name, frac)
    compared = check_batch(rt, ctx, scene, o, d, hit, t, name)
    for k in (1, 63, 64, 65):
        compared += check_batch(rt, ctx, scene, o[:k], d[:k], hit[:k], t[:k], "%s n=%d" % (name, k))
    # the library's own closest-hit query on the same rays agrees: occluded == (a hit and hits.t <= tmax)
    hits = rt.trace_rays(ctx, scene, o, d)
    for lname, tmax in limit_sets(hit, t).items():
        with np.errstate(invalid="ignore"):
            own = ((hits["object"] >= 0) & (hits["t"] <= tmax)).astype(np.uint8)
        assert rt.occluded_rays(ctx, scene, o, d, tmax).tobytes() == own.tobytes(), (name, lname)
    assert rt.occluded_rays(ctx, scene, o, d).tobytes() == (hits["object"] >= 0).astype(np.uint8).tobytes(), name
    print("%s: %d bytes compared, 0 differ" % (name, compared))
    return scene.info()["scene_in_lds"]


@pytest.mark.parametrize("name", [s for s in SCENES if s not in ("soup6k", "sphere50k")])
def test_occlusion_equals_the_oracle(rt, orc, ctx, models_dir, name):
    assert check_scene(rt, orc, ctx, models_dir, name) == 1          # the whole scene in LDS


def test_occlusion_equals_the_oracle_beyond_lds(rt, orc, ctx, models_dir):
    """soup6k and sphere50k: the placements beyond LDS.  HYBRID (2) and GLOBAL (0) must both run; a placement the committed shapes do not
    pick is forced with RT_AMD_SCENE_MODE in a fresh child process, as tests/test_gpu_query.py does it."""
    modes = {name: check_scene(rt, orc, ctx, models_dir, name) for name in ("soup6k", "sphere50k")}
    assert all(m in (0, 2) for m in modes.values()), modes
    missing = {0, 2} - set(modes.values())
    assert 2 not in missing, ("no scene runs the hybrid placement", modes)
    if 0 in missing:
        env = dict(os.environ, RT_AMD_SCENE_MODE="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "soup6k"], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "placement 0" in r.stdout and "child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def _square(x0, x1, z0, z1):
    """two triangles over x in [x0, x1], y in [-0.5, 0.5], tilted in z (a flat axis-aligned box is dropped by the strict slab test)"""
    a, b, c, e = (x0, -0.5, z0), (x1, -0.5, z0), (x1, 0.5, z1), (x0, 0.5, z1)
    return np.asarray([[a, b, c], [a, c, e]], np.float32)


GREY = ("standard", (0.5, 0.5, 0.5), 0)
TWO_MESHES = [
    ("mesh", _square(-0.6, -0.05, 2.0, 2.2), GREY),                 # 0: the first mesh, left
    ("sphere", (-0.15, 0.0, 1.0), 0.08, GREY),                      # 1: a simple object in front of it
    ("mesh", _square(-0.6, 1.0, 3.0, 3.3), GREY),                   # 2: the second mesh, behind and wider
]


def test_blockers_simple_object_first_mesh_second_mesh(rt, orc, ctx, models_dir):
    scene = ctx.commit(rt.SceneObjects(TWO_MESHES, models_dir))
    oracle = orc.Scene(TWO_MESHES, orc.MATH_DET, models_dir)
    o = np.zeros((4, 3), F)
    d = np.array([(-0.3, 0.0, 2.0),        # sphere, then mesh 0, then mesh 2
                  (-0.5, 0.3, 2.0),        # mesh 0, then mesh 2
                  (0.5, 0.0, 3.0),         # only mesh 2, the second of the two meshes
                  (0.0, 2.0, 1.0)], F)     # nothing
    hit, t, obj = oracle_hits(oracle, o, d)
    assert obj.tolist() == [1, 0, 2, -1], obj                        # the construction does what it says (oracle alone)
    h0, t0 = oracle.trace_one(o[0], d[0])[0], F(oracle.trace_one(o[0], d[0])[1][0])
    check_batch(rt, ctx, scene, o, d, hit, t, "two meshes")
    # ray 0 with a limit between the sphere and the mesh behind it: blocked by the simple object, no mesh needed
    between = F(t0 * F(1.5))
    assert h0 and between < F(1.0)                                   # (mesh 0 lies at t ~ 1 in units of this direction)
    assert rt.occluded_rays(ctx, scene, o[:1], d[:1], between).tolist() == [1]
    # ray 2 with limits around the second mesh's distance
    assert rt.occluded_rays(ctx, scene, o[2:3], d[2:3], t[2]).tolist() == [1]
    assert rt.occluded_rays(ctx, scene, o[2:3], d[2:3], np.nextafter(t[2], F(0))).tolist() == [0]
    # more rays over the same scene, every one compared
    o2, d2 = _rays(1500, 21, target=(0.0, 0.0, 2.5), spread=2.0)
    hit2, t2, obj2 = oracle_hits(oracle, o2, d2)
    assert set(obj2.tolist()) >= {-1, 0, 2}
    check_batch(rt, ctx, scene, o2, d2, hit2, t2, "two meshes, random")


ONE_WAY = [
    ("one_way_quad", (-1, 1, 1.0), (1, 1, 1.0), (1, -1, 1.0), (-1, -1, 1.0), False, GREY),
    ("one_way_quad", (-1, 1, 3.0), (1, 1, 3.0), (1, -1, 3.0), (-1, -1, 3.0), True, GREY),
]


def test_one_way_quads_from_both_sides(rt, orc, ctx, models_dir):
    scene = ctx.commit(rt.SceneObjects(ONE_WAY, models_dir))
    oracle = orc.Scene(ONE_WAY, orc.MATH_DET, models_dir)
    # through each quad along +z and along -z, limits short of the second quad
    o = np.array([(0.1, 0.2, 0.0), (0.1, 0.2, 2.0), (0.1, 0.2, 2.0), (0.1, 0.2, 4.0)], F)
    d = np.array([(0, 0, 1), (0, 0, -1), (0, 0, 1), (0, 0, -1)], F)
    hit, t, obj = oracle_hits(oracle, o, d)
    near = np.full(4, 1.5, F)
    want = expected(hit, t, near)
    assert want[0] != want[1] and want[2] != want[3], (hit, t, obj)   # each quad stops one direction only (oracle alone)
    assert rt.occluded_rays(ctx, scene, o, d, near).tobytes() == want.tobytes()
    check_batch(rt, ctx, scene, o, d, hit, t, "one-way quads")


@pytest.mark.parametrize("name", ["monkey", "reference_scene1"])
def test_nan_and_zero_direction_components(rt, orc, ctx, models_dir, name):
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    nan = F(np.nan)
    sub = F(1e-41)
    rays = [
        ((0, 0, 0), (0, 0.3, 1)), ((0.1, -0.1, 0), (0, 0, 1)), ((0.1, 0, 0), (0, 0, 1)), ((0, 0, 1.7), (1, 0, 0)), ((0, 0, 1.7), (0, -1, 0)),
        ((0.1, -0.1, 0), (sub, 0.05, 1)), ((0, 0, 0), (0.1, sub, 1)),
        ((0, 0, 0), (nan, nan, nan)), ((0.1, -0.1, 1.0), (nan, nan, nan)), ((0, 0, 0), (nan, 0, 1)), ((0, 0, 0), (0.1, -0.1, nan)),
        ((0, 0, 0), (0.3, -0.3, 3 * 0.9055385)), ((0, 0, 0), (0.1, -0.1, 1)), ((0, 0, 0), (0, 0, 0)),
    ]
    o = np.array([r[0] for r in rays], F)
    d = np.array([r[1] for r in rays], F)
    hit, t, _ = oracle_hits(oracle, o, d)
    assert not hit[7:11].any() and hit[:5].any() and hit[11] and hit[12]
    check_batch(rt, ctx, scene, o, d, hit, t, name)
    assert not rt.occluded_rays(ctx, scene, o[7:11], d[7:11]).any()                # a NaN component: not occluded


def oracle_visibility(oracle, cam_floats, W, H, light, bias):
    """the plane by two oracle calls per pixel, chained in float32: o' = (N * bias) + P (two roundings), d' = light - o', limit 1"""
    d = primaries(cam_floats, W, H).reshape(-1, 3)
    origin = np.asarray(cam_floats[0:3], F)
    light, bias = np.asarray(light, F), F(bias)
    out = np.zeros(W * H, np.uint8)
    for i in range(W * H):
        hit, rec = oracle.trace_one(origin, d[i])
        if not hit:
            out[i] = 2
            continue
        P, N = rec[1:4].astype(F), rec[4:7].astype(F)
        o2 = ((N * bias).astype(F) + P).astype(F)
        d2 = (light - o2).astype(F)
        hit2, rec2 = oracle.trace_one(o2, d2)
        out[i] = 0 if (hit2 and F(rec2[0]) <= F(1.0)) else 1
    return out.reshape(H, W)


VIS_CODES = set()


@pytest.mark.parametrize("name", ["three_sphere", "monkey", "soup6k"])            # no mesh, a mesh in LDS, the hybrid placement
def test_visibility_plane(rt, orc, ctx, models_dir, name):
    import torch
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    assert scene.info()["scene_in_lds"] == (2 if name == "soup6k" else 1)
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    W, H = 67, 45                                                                 # ragged: neither is a multiple of 8
    cam = rt.Camera(W, H)
    for light in ((1.5, 2.0, 0.2), (0.0, -3.0, 1.5)):                             # in the open; inside the ground sphere
        for bias in (1e-3, 0.0):
            want = oracle_visibility(oracle, cam.floats(), W, H, light, bias)
            got = rt.render_visibility(ctx, scene, cam, light, bias)
            assert got.shape == (H, W) and got.dtype == np.uint8
            assert got.tobytes() == want.tobytes(), (name, light, bias, int((got != want).sum()))
            VIS_CODES.update(np.unique(want).tolist())
            print("%s light %s bias %g: blocked %d lit %d no surface %d" % (name, light, bias, (want == 0).sum(), (want == 1).sum(), (want == 2).sum()))
            # the device form into a torch tensor gives the same bytes
            t = torch.full((H, W), 9, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            rt.render_visibility_device(ctx, scene, cam, light, bias, t.data_ptr())
            ctx.synchronize()
            assert t.cpu().numpy().tobytes() == want.tobytes()
            assert ctx.last_kernel_ms() > 0


def test_visibility_codes_all_occur():
    """(after the planes above) blocked, lit and no-surface each occur in at least one case"""
    assert VIS_CODES == {0, 1, 2}, VIS_CODES


def test_host_and_device_forms_agree_and_streams_order(rt, orc, ctx, models_dir):
    import torch
    objs, _ = rt.scenes.monkey()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    n = 2 ** 18 + 17
    o, d = _rays(n, 11)
    hits = rt.trace_rays(ctx, scene, o, d)
    tmax = np.where(hits["object"] >= 0, hits["t"], F(1.0)).astype(F)
    tmax[::3] = np.nextafter(tmax[::3], F(0))
    host = rt.occluded_rays(ctx, scene, o, d, tmax)
    with np.errstate(invalid="ignore"):
        assert host.tobytes() == ((hits["object"] >= 0) & (hits["t"] <= tmax)).astype(np.uint8).tobytes()
    assert 0.1 < host.mean() < 0.9
    dev = torch.device("cuda:0")
    t_o, t_d, t_t = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (o, d, tmax))
    t_out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rt.occluded_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), t_t.data_ptr(), n, t_out.data_ptr())
    ctx.synchronize()
    assert t_out.cpu().numpy().tobytes() == host.tobytes()
    assert ctx.last_kernel_ms() > 0
    # NULL limits, device form
    rt.occluded_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), None, n, t_out.data_ptr())
    ctx.synchronize()
    assert t_out.cpu().numpy().tobytes() == (hits["object"] >= 0).astype(np.uint8).tobytes()
    # on a stream of the caller, ordered against a following copy on that stream
    s = torch.cuda.Stream(device=dev)
    t_out.fill_(7)
    t_copy = torch.zeros_like(t_out)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rt.occluded_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), t_t.data_ptr(), n, t_out.data_ptr(), stream=s.cuda_stream)
        t_copy.copy_(t_out, non_blocking=True)
    s.synchronize()
    assert t_copy.cpu().numpy().tobytes() == host.tobytes()
    # a shuffled batch gives the shuffled answers
    perm = np.random.default_rng(3).permutation(n)
    assert rt.occluded_rays(ctx, scene, o[perm], d[perm], tmax[perm]).tobytes() == host[perm].tobytes()
    # line of sight: visible_between is occluded_rays on (a, b - a) with the limit 1 - shrink
    a, b = o[:4096], (o[:4096] + d[:4096] * F(2.5)).astype(F)
    vis = rt.visible_between(ctx, scene, a, b, shrink=1e-4)
    want = rt.occluded_rays(ctx, scene, a, (b - a).astype(F), F(1.0) - F(1e-4)) == 0
    assert vis.dtype == bool and np.array_equal(vis, want) and vis.any() and (~vis).any()
    assert rt.occluded_rays(ctx, scene, np.zeros((0, 3), F), np.zeros((0, 3), F)).shape == (0,)


def test_frames_and_records_unchanged_by_occlusion_calls(rt, ctx, models_dir):
    """the context's scratch (ray counter, query buffers, events) is shared: frames and closest-hit records before and after"""
    objs, _ = rt.scenes.monkey()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    W, H = 96, 72
    cam = rt.Camera(W, H)
    o, d = _rays(5000, 2)

    def frame():
        data = rt.VariableRenderData(W, H)
        for k in range(2):
            rt.render(ctx, scene, cam, rt.RenderData(4, 4, True, (0.8, 1.0, 1.0)), data, 100 + k)
        return data.previous_render.copy()

    f0, h0 = frame(), rt.trace_rays(ctx, scene, o, d)
    aov0 = rt.render_aov(ctx, scene, cam, planes=("depth",))["depth"]
    occ0 = rt.occluded_rays(ctx, scene, o, d, 2.0)
    vis0 = rt.render_visibility(ctx, scene, cam, (0.5, 1.0, 0.0), 1e-3)
    f1, h1 = frame(), rt.trace_rays(ctx, scene, o, d)
    assert np.array_equal(u32(f0), u32(f1)) and h0.tobytes() == h1.tobytes()
    assert rt.render_aov(ctx, scene, cam, planes=("depth",))["depth"].tobytes() == aov0.tobytes()
    assert rt.occluded_rays(ctx, scene, o, d, 2.0).tobytes() == occ0.tobytes()
    assert rt.render_visibility(ctx, scene, cam, (0.5, 1.0, 0.0), 1e-3).tobytes() == vis0.tobytes()


def test_errors_leave_the_context_usable(rt, ctx, models_dir):
    import ctypes as C
    L = rt.lib()
    objs, _ = rt.scenes.three_sphere()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    other = rt.Context(0)
    foreign = other.commit(rt.SceneObjects(objs, models_dir))
    o, d = _rays(64, 1)
    out = np.zeros(64, np.uint8)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
    vp = lambda a: C.c_void_p(a.ctypes.data)                    # noqa: E731
    good = rt.occluded_rays(ctx, scene, o, d)
    for args, msg in [((ctx._h, scene._h, fp(o), fp(d), None, -1, vp(out)), "ray count"),
                      ((ctx._h, scene._h, fp(o), fp(d), None, 2 ** 30 + 1, vp(out)), "ray count"),
                      ((ctx._h, scene._h, None, fp(d), None, 64, vp(out)), "null"),
                      ((ctx._h, scene._h, fp(o), None, None, 64, vp(out)), "null"),
                      ((ctx._h, scene._h, fp(o), fp(d), None, 64, None), "null"),
                      ((ctx._h, foreign._h, fp(o), fp(d), None, 64, vp(out)), "another context"),
                      ((ctx._h, None, fp(o), fp(d), None, 64, vp(out)), "null")]:
        assert L.rt_occluded_rays(*args) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        assert rt.occluded_rays(ctx, scene, o, d).tobytes() == good.tobytes()
    assert L.rt_occluded_rays_device(ctx._h, scene._h, None, None, None, 5, None, None) == rt.RT_ERR_INVALID
    assert L.rt_occluded_rays_device(ctx._h, scene._h, None, None, None, -5, None, None) == rt.RT_ERR_INVALID
    # n == 0 succeeds and touches nothing, null pointers included
    assert L.rt_occluded_rays(ctx._h, scene._h, None, None, None, 0, None) == rt.RT_OK
    assert L.rt_occluded_rays_device(ctx._h, scene._h, None, None, None, 0, None, None) == rt.RT_OK
    cam = rt.Camera(32, 24)
    light = np.zeros(3, F)
    plane = np.zeros((24, 32), np.uint8)
    assert L.rt_render_visibility(ctx._h, scene._h, None, fp(light), 0.0, vp(plane)) == rt.RT_ERR_INVALID
    assert L.rt_render_visibility(ctx._h, scene._h, C.byref(cam.c), None, 0.0, vp(plane)) == rt.RT_ERR_INVALID
    assert L.rt_render_visibility(ctx._h, scene._h, C.byref(cam.c), fp(light), 0.0, None) == rt.RT_ERR_INVALID
    assert L.rt_render_visibility_device(ctx._h, foreign._h, C.byref(cam.c), fp(light), 0.0, vp(plane), None) == rt.RT_ERR_INVALID
    assert "another context" in ctx.last_error()
    assert rt.render_visibility(ctx, scene, cam, (0, 2, 0), 1e-3).shape == (24, 32)
    assert rt.occluded_rays(ctx, scene, o, d).tobytes() == good.tobytes()


def test_cpp_occlusion_example(rt, orc, models_dir, tmp_path):
    """host/raytracer.hpp's occluded / occluded_rays / render_visibility through host/example_query.cpp, against the oracle"""
    import re
    bmod = __import__("importlib").import_module("ray-tracer_amd.build")
    exe = bmod.build_query_example()
    W, H = 80, 64
    objs, _ = rt.scenes.CONFIG_SCENES["reference_scene0"]()
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    text = subprocess.check_output([exe, models_dir, "0", str(W), str(H), str(tmp_path / "depth.pgm")], timeout=300, cwd=str(tmp_path), text=True)
    # line of sight from the origin to (0, 0, 2) and to half that way
    hit, rec = oracle.trace_one((0, 0, 0), (0, 0, 2))
    m = re.search(r"line of sight: whole (\d) half (\d)", text)
    assert m, text
    assert int(m.group(1)) == int(hit and F(rec[0]) <= F(1.0)) and int(m.group(2)) == int(hit and F(rec[0]) <= F(0.5))
    want = oracle_visibility(oracle, rt.Camera(W, H).floats(), W, H, (0.0, 0.3, 1.7), 1e-3)
    m = re.search(r"shadow mask: blocked (\d+) lit (\d+) no surface (\d+)", text)
    assert m and [int(x) for x in m.groups()] == [int((want == k).sum()) for k in (0, 1, 2)], (text, [(want == k).sum() for k in (0, 1, 2)])


if __name__ == "__main__":
    # child of test_occlusion_equals_the_oracle_beyond_lds: one scene under the environment's placement knob
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    _rt = importlib.import_module("ray-tracer_amd")
    from oracle import binding as _orc
    _orc.build()
    check_scene(_rt, _orc, _rt.Context(0), _rt.scenes.models_dir(), sys.argv[1])
    print("child ok")
