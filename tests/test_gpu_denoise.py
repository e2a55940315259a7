"""rt_denoise / rt_denoise_device on the GPU against the yardstick (tests/denoise_ref.py, the definition in NumPy float32): equal as
uint32 for EVERY pixel, never on a sample - frames and planes rendered by the library itself, ragged sizes, steps larger than the image,
every level count, with and without the optional planes, in place, on a caller's stream, non-finite pixels."""
import subprocess

import numpy as np
import pytest

from denoise_ref import denoise_ref

pytestmark = pytest.mark.gpu

F = np.float32
# the scenes of tests/test_gpu_query.py that render in a moment at these sizes (all of them do)
SCENES = ["three_sphere", "cube", "monkey", "reference_scene0", "reference_scene1", "reference_scene2", "reference_scene3", "soup6k", "sphere50k"]
SIZES = [(1, 1), (5, 3), (64, 64), (67, 45), (333, 200), (5, 40)]          # (W, H); the last one has W < 8 < H


def u32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same_bits(got, want, what=""):
    bad = (u32(got) != u32(want)).any(axis=2)
    assert got.shape == want.shape and not bad.any(), "%s: %d of %d pixels differ, first at (y, x) = %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


_rendered = {}


def rendered(rt, ctx, models_dir, name, W, H, spp=4):
    """a noisy frame of the scene (spp samples, 8 bounces, one frame) and its first-hit planes, both from the library"""
    key = (name, W, H, spp)
    if key not in _rendered:
        objs, sky = rt.scenes.CONFIG_SCENES[name]()
        scene = ctx.commit(rt.SceneObjects(objs, models_dir))
        cam = rt.Camera(W, H)
        data = rt.VariableRenderData(W, H)
        rt.render(ctx, scene, cam, rt.RenderData(spp, 8, True, sky), data, 4321)
        aov = rt.render_aov(ctx, scene, cam, sky, planes=("depth", "normal", "albedo", "object"))
        _rendered[key] = (data.previous_render.copy(), aov["normal"], aov["depth"], aov["object"], aov["albedo"])
    return _rendered[key]


def check(rt, ctx, planes, what, use_object=True, use_albedo=True, rendered_case=True, **fields):
    c, n, z, o, a = planes
    o, a = (o if use_object else None), (a if use_albedo else None)
    p = rt.DenoiseParams(**fields)
    want = denoise_ref(c, n, z, o, a, **p.as_dict())
    if rendered_case and not fields and c.shape[0] >= 64 and c.shape[1] >= 64:
        # asserted from the yardstick alone, before the GPU is asked: with the default parameters the filter changes at least 10 % of a
        # rendered frame's pixels, so an entry point that copied its input could not pass (sky pixels never change)
        changed = float((u32(want) != u32(c)).any(axis=2).mean())
        print("%s: %.0f %% of the pixels change" % (what, 100 * changed))
        assert changed >= 0.10, (what, changed)
    got = rt.denoise(ctx, c, n, z, o, a, p)
    assert_same_bits(got, want, what)
    return want


@pytest.mark.parametrize("name", SCENES)
def test_rendered_scenes_equal_the_yardstick(rt, ctx, models_dir, name):
    for W, H in ((64, 64), (96, 80)):
        planes = rendered(rt, ctx, models_dir, name, W, H)
        for use_albedo in (True, False):          # (check() asserts the 10 % precondition on these: default parameters, 64 x 64 or more)
            check(rt, ctx, planes, "%s %dx%d albedo %d" % (name, W, H, use_albedo), use_albedo=use_albedo)
        assert ctx.last_kernel_ms() > 0


@pytest.mark.parametrize("W,H", SIZES)
def test_sizes(rt, ctx, models_dir, W, H):
    """ragged tiles, halos wider than the image, steps larger than the image (iterations = 8 is step 128)"""
    planes = rendered(rt, ctx, models_dir, "monkey", W, H)
    for iterations in (1, 5, 8):
        check(rt, ctx, planes, "%dx%d, %d levels" % (W, H, iterations), iterations=iterations)
    check(rt, ctx, planes, "%dx%d, bare" % (W, H), use_object=False, use_albedo=False, iterations=8)
    check(rt, ctx, planes, "%dx%d, defaults" % (W, H))


@pytest.mark.parametrize("iterations", range(1, 9))
def test_parameter_matrix(rt, ctx, models_dir, iterations):
    planes = rendered(rt, ctx, models_dir, "reference_scene0", 67, 45)
    for power in (0, 5, 8):
        for use_object in (True, False):
            for use_albedo in (True, False):
                check(rt, ctx, planes, "levels %d power %d object %d albedo %d" % (iterations, power, use_object, use_albedo),
                      use_object=use_object, use_albedo=use_albedo, iterations=iterations, normal_power_log2=power)


@pytest.mark.parametrize("name", ["three_sphere", "monkey"])
def test_extreme_colour_tolerances(rt, ctx, models_dir, name):
    planes = rendered(rt, ctx, models_dir, name, 67, 45)
    for sigma in (1e6, 1e-6, 3e38, 1e-30):
        for use_albedo in (True, False):
            check(rt, ctx, planes, "sigma_colour %g albedo %d" % (sigma, use_albedo), use_albedo=use_albedo, sigma_colour=sigma)
    check(rt, ctx, planes, "loose depth", sigma_depth=10.0, sigma_colour=8.0)
    check(rt, ctx, planes, "tight depth", sigma_depth=1e-4, albedo_floor=0.5)


def test_non_finite_pixels(rt, ctx):
    """synthetic planes with a NaN and an Inf colour pixel: the device result equals the yardstick there too, and nothing spreads"""
    H, W = 40, 56
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    n = np.stack([0.2 * np.sin(x / 6.0), 0.2 * np.cos(y / 4.0), -np.ones_like(x)], axis=2).astype(F)
    n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    z = (2.0 + 0.01 * x + 0.015 * y).astype(F)
    o = (x * 2 // W).astype(np.int32)
    a = (0.2 + 0.7 * rng.random((H, W, 3))).astype(F)
    c = rng.random((H, W, 3)).astype(F)
    c[10, 10, 0] = np.nan
    c[20, 30, 2] = np.inf
    c[21, 30, 1] = -np.inf
    c[H - 1, W - 1, :] = np.nan
    for use_albedo in (False, True):
        want = check(rt, ctx, (c, n, z, o, a), "non-finite, albedo %d" % use_albedo, use_albedo=use_albedo, rendered_case=False, iterations=6)
        assert (~np.isfinite(want).all(axis=2)).sum() == 4
    # guide planes of a miss everywhere: every pixel keeps its colour
    got = rt.denoise(ctx, c, np.zeros_like(n), np.full((H, W), 2.0 ** 30, F), np.full((H, W), -1, np.int32))
    assert_same_bits(got, c, "all misses")


def test_device_form_in_place_and_on_a_stream(rt, ctx, models_dir):
    import torch
    dev = torch.device("cuda:0")
    W, H = 96, 80
    c, n, z, o, a = rendered(rt, ctx, models_dir, "monkey", W, H)
    p = rt.DenoiseParams(iterations=6)
    host = rt.denoise(ctx, c, n, z, o, a, p)
    assert_same_bits(host, denoise_ref(c, n, z, o, a, **p.as_dict()), "host form")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in (("c", c), ("n", n), ("z", z), ("o", o), ("a", a))}
    out = torch.full((H, W, 3), -1.0, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    # on a caller's stream, into a buffer of its own
    rt.denoise_device(ctx, W, H, t["c"].data_ptr(), t["n"].data_ptr(), t["z"].data_ptr(), t["o"].data_ptr(), t["a"].data_ptr(), out.data_ptr(), p,
                      stream=stream.cuda_stream)
    ctx.synchronize()
    assert_same_bits(out.cpu().numpy(), host, "device form on a stream")
    assert ctx.last_kernel_ms() > 0
    assert t["c"].cpu().numpy().tobytes() == np.ascontiguousarray(c).tobytes()          # the input is not touched
    # d_out == d_colour, on the default stream, without the optional planes
    rt.denoise_device(ctx, W, H, t["c"].data_ptr(), t["n"].data_ptr(), t["z"].data_ptr(), None, None, t["c"].data_ptr(), p)
    ctx.synchronize()
    assert_same_bits(t["c"].cpu().numpy(), denoise_ref(c, n, z, None, None, **p.as_dict()), "in place")


def test_two_calls_of_different_sizes(rt, ctx, models_dir):
    """the context's scratch regrows between calls and a smaller call after a larger one uses the larger buffer"""
    small = rendered(rt, ctx, models_dir, "cube", 64, 64)
    large = rendered(rt, ctx, models_dir, "cube", 333, 200)
    for planes, what in ((small, "small"), (large, "large"), (small, "small again"), (large, "large again")):
        check(rt, ctx, planes, what)
    fresh = rt.Context(0)
    check(rt, fresh, large, "large first on a fresh context")
    check(rt, fresh, small, "then small")


def test_a_denoise_call_disturbs_no_render_state(rt, ctx, models_dir):
    objs, sky = rt.scenes.monkey()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    W, H = 96, 80
    cam, rs = rt.Camera(W, H), rt.RenderData(4, 8, True, sky)
    before = rt.VariableRenderData(W, H)
    rt.render_frames(ctx, scene, cam, rs, before, [11, 12])
    planes = rendered(rt, ctx, models_dir, "monkey", W, H)
    check(rt, ctx, planes, "between the frames")
    after = rt.VariableRenderData(W, H)
    rt.render_frames(ctx, scene, cam, rs, after, [11, 12])
    assert after.previous_render.tobytes() == before.previous_render.tobytes()
    aov = rt.render_aov(ctx, scene, cam, sky, planes=("depth", "normal", "albedo", "object"))
    assert all(aov[k].tobytes() == v.tobytes() for k, v in zip(("normal", "depth", "object", "albedo"), planes[1:]))


def test_render_denoised(rt, ctx, models_dir):
    objs, sky = rt.scenes.three_sphere()
    scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    W, H = 96, 64
    cam, rs = rt.Camera(W, H), rt.RenderData(4, 8, True, sky)
    noisy, out = rt.render_denoised(ctx, scene, cam, rs, [5, 6])
    data = rt.VariableRenderData(W, H)
    rt.render_frames(ctx, scene, cam, rs, data, [5, 6])
    assert_same_bits(noisy, data.previous_render, "the noisy frame is render_frames'")
    aov = rt.render_aov(ctx, scene, cam, sky, planes=("depth", "normal", "albedo", "object"))
    p = rt.DenoiseParams()
    assert_same_bits(out, denoise_ref(noisy, aov["normal"], aov["depth"], aov["object"], aov["albedo"], **p.as_dict()), "render_denoised")
    tight = rt.render_denoised(ctx, scene, cam, rs, [5, 6], rt.DenoiseParams(iterations=2))[1]
    assert_same_bits(tight, denoise_ref(noisy, aov["normal"], aov["depth"], aov["object"], aov["albedo"], **rt.DenoiseParams(iterations=2).as_dict()), "two levels")


def test_errors_leave_the_context_usable(rt, ctx, models_dir):
    import ctypes as C
    L = rt.lib()
    planes = rendered(rt, ctx, models_dir, "cube", 64, 64)
    c, n, z, o, a = [np.ascontiguousarray(v) for v in planes]
    good = rt.denoise(ctx, c, n, z, o, a)
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
    ip = o.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros_like(c)
    ok = rt.DenoiseParams()

    def params(**kw):
        p = rt.DenoiseParams()
        for k, v in kw.items():
            setattr(p.c, k, v)
        return p

    r = params()
    r.c.reserved[1] = 7
    for args, msg in [((ctx._h, 64, 64, None, fp(n), fp(z), ip, fp(a), C.byref(ok.c), fp(out)), "null"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), None, fp(out)), "null"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(ok.c), None), "null"),
                      ((ctx._h, 0, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(ok.c), fp(out)), "image size"),
                      ((ctx._h, 64, -3, fp(c), fp(n), fp(z), ip, fp(a), C.byref(ok.c), fp(out)), "image size"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(params(iterations=9).c), fp(out)), "iterations"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(params(iterations=0).c), fp(out)), "iterations"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(params(sigma_colour=0.0).c), fp(out)), "sigma"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(params(sigma_depth=float("nan")).c), fp(out)), "sigma"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(params(normal_power_log2=9).c), fp(out)), "normal_power_log2"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(params(albedo_floor=0.0).c), fp(out)), "albedo_floor"),
                      ((ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, fp(a), C.byref(r.c), fp(out)), "reserved")]:
        assert L.rt_denoise(*args) == rt.RT_ERR_INVALID, msg
        assert msg in ctx.last_error(), (msg, ctx.last_error())
        assert not out.any()
        assert rt.denoise(ctx, c, n, z, o, a).tobytes() == good.tobytes()
    # albedo_floor is only read when an albedo plane is given
    assert L.rt_denoise(ctx._h, 64, 64, fp(c), fp(n), fp(z), ip, None, C.byref(params(albedo_floor=0.0).c), fp(out)) == rt.RT_OK
    assert_same_bits(out, denoise_ref(c, n, z, o, None, **ok.as_dict()), "no albedo, floor 0")
    with pytest.raises(ValueError, match="shape"):
        rt.denoise(ctx, c, n[:-1], z)


def test_cpp_denoise_example(rt, models_dir, tmp_path):
    """host/raytracer.hpp's Renderer::denoise through host/example_denoise.cpp: the picture it writes holds the noisy frame on the left
    and, on the right, what the yardstick makes of that frame and the library's planes"""
    import re
    bmod = __import__("importlib").import_module("ray-tracer_amd.build")
    exe = bmod.build_denoise_example()
    W, H, spp = 96, 80, 4
    png = tmp_path / "pair.png"
    raw = tmp_path / "pair.f32"
    text = subprocess.check_output([exe, models_dir, str(W), str(H), str(spp), str(png), str(raw)], timeout=300, cwd=str(tmp_path), text=True)
    assert re.search(r"denoised %d x %d" % (W, H), text), text
    assert png.read_bytes().startswith(b"\x89PNG")
    both = np.fromfile(str(raw), F).reshape(2, H, W, 3)
    objs, sky = rt.scenes.reference_scene0()          # the reference's monkey_test_scene (the monkey and a sphere in a Cornell box; no sky): the mirror's scene 0
    ctx2 = rt.Context(0)
    scene = ctx2.commit(rt.SceneObjects(objs, models_dir))
    aov = rt.render_aov(ctx2, scene, rt.Camera(W, H), sky, planes=("depth", "normal", "albedo", "object"))
    want = denoise_ref(both[0], aov["normal"], aov["depth"], aov["object"], aov["albedo"], **rt.DenoiseParams().as_dict())
    assert (u32(both[0]) != u32(both[1])).any(axis=2).mean() >= 0.10
    assert_same_bits(both[1], want, "the example's denoised frame")
