"""rt_traits_kernel, the render kernel's variant for scenes of known traits (rt_render_kernel.h), against rt_render_kernel on the
same scene (RT_AMD_KERNEL_VARIANT=generic at commit) and against the CPU oracle in det mode: two progressive frames in one launch
(render_device_batch), every frame compared as uint32.  The variant leaves out control flow only, so nothing has a tolerance.

Scenes: the three config scenes that have all three traits and a random spheres-plus-one-mesh scene drawn by tests/random_scenes.py; bounce
limits 1 and 8; 64 x 48 and, ragged against the 8 x 8 tiles, 70 x 50.  A camera whose rays have direction components of exactly zero reaches
the min / max copy of the descend loop; RT_AMD_DESCEND_KEEP 20 and 63 move the loop's exit.  Scenes that lack a trait must report the
generic kernel and still render the oracle's frame.  The oracle's frames are computed once per case and shared.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from random_scenes import random_scene
from test_kernel_variant_choice import scenes as choice_scenes

pytestmark = pytest.mark.gpu

F = np.float32
SPP, TIMES = 4, [4242, 4243]
SIZES = [(64, 48), (70, 50)]
LIMITS = [1, 8]
SKY = (0.5, 0.7, 1.0)
_REFS = {}


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def random_spheres_and_mesh(seed=13):
    """the spheres of random_scene(seed) and the first of its triangle soups, each with a plain material: the generator's own where that is
    standard or emissive, else a standard one of the colour it drew"""
    def plain(m):
        return m if m[0] in ("standard", "emissive") else ("standard", tuple(m[1]) if m[0] in ("checkerboard", "refractive") else (0.7, 0.6, 0.5), 0.3)
    objs, _ = random_scene(seed)
    spheres = [("sphere", o[1], o[2], plain(o[3])) for o in objs if o[0] == "sphere"]
    mesh = next(("mesh", o[1], plain(o[2])) for o in objs if o[0] == "mesh")
    assert len(spheres) >= 2
    return spheres[:1] + [mesh] + spheres[1:] + [("sphere", (0, 1.6, 2.0), 0.5, ("emissive", (1, 1, 1), 4.0))]


def zero_direction_scene():
    """tests/test_gpu_parity.py test_rays_with_a_zero_direction_component with spheres for its quad and its second mesh: many vertices in the
    planes x == 0 and y == 0, a mirror-like ground, and a camera at the origin whose pixel column 32 has x == 0 and whose row 24 has y == 0"""
    rng = np.random.default_rng(5)
    n = 160
    tris = (rng.normal(0, 0.9, (n, 1, 3)) + rng.normal(0, 0.35, (n, 3, 3))).astype(F)
    tris[..., 2] -= 4.0
    tris[rng.random((n, 3)) < 0.35, 0] = 0.0
    tris[rng.random((n, 3)) < 0.35, 1] = 0.0
    objs = [("mesh", tris.reshape(n, 9), ("standard", (0.8, 0.6, 0.4), 0.9)),
            ("sphere", (3.0, 4.0, -4.0), 1.5, ("emissive", (1.0, 1.0, 1.0), 6)),
            ("sphere", (0.0, -102.0, -4.0), 100, ("standard", (0.6, 0.6, 0.6), 1.0))]
    cam = np.array([0, 0, 0, -4.0, 3.0, -8.0, 0.125, 0, 0, 0, -0.125, 0], F)
    return objs, cam


def scene_objs(rt, name):
    if name == "random":
        return random_spheres_and_mesh(), SKY
    return rt.scenes.CONFIG_SCENES[name]()


def oracle_frames(orc, models_dir, key, objs, cam, W, H, limit, sky, aa=True):
    """the two progressive frames of the oracle, once per case"""
    if key not in _REFS:
        o = orc.Scene(objs, orc.MATH_DET, models_dir)
        first = o.render(cam, W, H, SPP, limit, sky, time_ms=TIMES[0], antialias=aa)
        _REFS[key] = o.render(cam, W, H, SPP, limit, sky, time_ms=TIMES[1], frame_num=1, prev=first, antialias=aa)
    return _REFS[key]


def commit(rt, ctx, monkeypatch, objs, models_dir, variant, override=None):
    """the scene committed with RT_AMD_KERNEL_VARIANT=generic in the environment (override; by default: when that is the variant asked for) or
    without, and the variant it then reports"""
    with monkeypatch.context() as m:
        m.delenv("RT_AMD_KERNEL_VARIANT", raising=False)
        if (variant == "generic") if override is None else override:
            m.setenv("RT_AMD_KERNEL_VARIANT", "generic")
        scene = ctx.commit(rt.SceneObjects(objs, models_dir))
    assert scene.info()["kernel_variant"] == variant, scene.info()
    return scene


def two_frames(rt, ctx, scene, cam, W, H, limit, sky, aa=True):
    import torch
    out = torch.full((H, W, 3), 7.0, device="cuda:0")            # garbage: frame 0 ignores it
    st = torch.cuda.current_stream().cuda_stream
    rt.render_device_batch(ctx, scene, cam, rt.RenderData(SPP, limit, aa, sky), TIMES, 0, out.data_ptr(), stream=st)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_same(got, want, what):
    bad = (u32(got) != u32(want)).any(axis=2)
    assert not bad.any(), (what, "%d of %d pixels differ, first at (y, x) = %s" % (int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0])))


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["monkey", "cube", "three_sphere", "random"])
def test_variant_generic_and_oracle_agree(rt, orc, ctx, models_dir, monkeypatch, name, size, limit):
    W, H = size
    objs, sky = scene_objs(rt, name)
    cam = rt.Camera(W, H)
    want = oracle_frames(orc, models_dir, (name, W, H, limit), objs, cam.floats(), W, H, limit, sky)
    frames = {v: two_frames(rt, ctx, commit(rt, ctx, monkeypatch, objs, models_dir, v), cam, W, H, limit, sky) for v in ("traits", "generic")}
    assert_same(frames["traits"], frames["generic"], (name, size, limit, "traits kernel against generic kernel"))
    assert_same(frames["traits"], want, (name, size, limit, "traits kernel against the oracle"))
    assert_same(frames["generic"], want, (name, size, limit, "generic kernel against the oracle"))


@pytest.mark.parametrize("aa", [False, True])
def test_rays_with_a_zero_direction_component(rt, orc, ctx, models_dir, monkeypatch, aa):
    objs, camf = zero_direction_scene()
    W, H, limit = 64, 48, 5
    cam = rt.Camera(W, H, floats=camf)
    want = oracle_frames(orc, models_dir, ("zero", aa), objs, camf, W, H, limit, SKY, aa)
    for v in ("traits", "generic"):
        scene = commit(rt, ctx, monkeypatch, objs, models_dir, v)
        assert_same(two_frames(rt, ctx, scene, cam, W, H, limit, SKY, aa), want, ("zero direction components", v, aa))


@pytest.mark.parametrize("keep", [20, 63])
def test_descend_keep(rt, orc, models_dir, monkeypatch, keep):
    """the descend loop's exit rule at two settings, on the 1024-thread shape that pops inside the loop (a context reads the knob when it is made)"""
    W, H, limit = 64, 48, 8
    objs, sky = scene_objs(rt, "monkey")
    cam = rt.Camera(W, H)
    want = oracle_frames(orc, models_dir, ("monkey", W, H, limit), objs, cam.floats(), W, H, limit, sky)
    with monkeypatch.context() as m:
        m.setenv("RT_AMD_DESCEND_KEEP", str(keep))
        own = rt.Context(0)
    for v in ("traits", "generic"):
        scene = commit(rt, own, monkeypatch, objs, models_dir, v)
        assert scene.info()["threads_per_block"] == 1024, scene.info()
        assert_same(two_frames(rt, own, scene, cam, W, H, limit, sky), want, ("descend_keep", keep, v))


@pytest.mark.parametrize("name", ["reference_scene0", "reference_scene3", "checkerboard_sphere", "two_meshes"])
def test_a_scene_without_a_trait_runs_the_generic_kernel(rt, orc, ctx, models_dir, monkeypatch, name):
    objs, want_traits = choice_scenes(rt)[name]
    sky = rt.scenes.CONFIG_SCENES[name]()[1] if name in rt.scenes.CONFIG_SCENES else SKY
    W, H, limit = 64, 48, 8
    cam = rt.Camera(W, H)
    assert want_traits is None or len(want_traits) == 2
    scene = commit(rt, ctx, monkeypatch, objs, models_dir, "generic", override=False)          # no override: the scene's own choice
    want = oracle_frames(orc, models_dir, (name, W, H, limit), objs, cam.floats(), W, H, limit, sky)
    assert_same(two_frames(rt, ctx, scene, cam, W, H, limit, sky), want, (name, "generic kernel against the oracle"))
