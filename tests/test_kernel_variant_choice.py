"""Which render kernel a scene runs is decided on the host when the scene is flattened, from three traits of the object list (rt_device_scene.h
RT_TRAIT_*, rt_scene_traits in rt_host.cpp, rt_sched::choose_variant): every object besides the meshes is a sphere, there is at most one mesh,
no material needs texture coordinates, refracts or carries a texture.  A scene with all three asks for rt_traits_kernel, every other one for
rt_render_kernel, and RT_AMD_KERNEL_VARIANT=generic keeps rt_render_kernel for all.  CPU test: SceneObjects.debug_flatten() needs no device."""
import numpy as np
import pytest

ALL = {"SPHERES_ONLY", "ONE_MESH", "PLAIN_MATERIALS"}
_RNG = np.random.default_rng(3)


def _soup(n, centre):
    return (np.asarray(centre) + _RNG.normal(0, 0.2, (n, 1, 3)) + _RNG.normal(0, 0.06, (n, 3, 3))).astype(np.float32).reshape(n, 9)


def scenes(rt):
    """name -> (objects, the traits expected to be ON)"""
    cfg = rt.scenes.CONFIG_SCENES
    ground = ("sphere", (0, -100.5, 1.5), 100, ("standard", (0.5, 0.5, 0.5), 0.2))
    light = ("sphere", (0, 1.3, 1.5), 0.5, ("emissive", (1, 1, 1), 5.0))
    return {
        "three_sphere": (cfg["three_sphere"]()[0], ALL),
        "cube": (cfg["cube"]()[0], ALL),
        "monkey": (cfg["monkey"]()[0], ALL),
        "reference_scene0": (cfg["reference_scene0"]()[0], None),       # quads and cuboids: asserted below to lack SPHERES_ONLY
        "reference_scene3": (cfg["reference_scene3"]()[0], None),       # refractive: lacks PLAIN_MATERIALS
        "checkerboard_sphere": ([ground, light, ("sphere", (0, 0, 2), 0.4, ("checkerboard", (0.9, 0.9, 0.9), (0.1, 0.1, 0.1), 6, 0.1))], ALL - {"PLAIN_MATERIALS"}),
        "two_meshes": ([ground, light, ("mesh", _soup(30, (-0.5, 0, 2)), ("standard", (0.8, 0.3, 0.3), 0.2)),
                        ("mesh", _soup(30, (0.5, 0, 2)), ("standard", (0.3, 0.3, 0.8), 0.2))], ALL - {"ONE_MESH"}),
    }


def flatten(rt, objs):
    return rt.SceneObjects(objs).debug_flatten()


def test_traits_and_variant_of_each_scene(rt, monkeypatch):
    monkeypatch.delenv("RT_AMD_KERNEL_VARIANT", raising=False)
    seen_on, seen_off = set(), set()
    for name, (objs, want) in scenes(rt).items():
        f = flatten(rt, objs)
        got = f["traits"]
        assert got <= ALL, (name, got)
        if want is not None:
            assert got == want, (name, got)
        assert f["kernel_variant"] == ("traits" if got == ALL else "generic"), (name, got, f["kernel_variant"])
        seen_on |= got
        seen_off |= ALL - got
    f0, f3 = flatten(rt, scenes(rt)["reference_scene0"][0]), flatten(rt, scenes(rt)["reference_scene3"][0])
    assert "SPHERES_ONLY" not in f0["traits"] and f0["kernel_variant"] == "generic"
    assert "PLAIN_MATERIALS" not in f3["traits"] and f3["kernel_variant"] == "generic"
    # every trait is seen both ways: none is stuck
    assert seen_on == ALL and seen_off == ALL, (seen_on, seen_off)


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey"])
def test_each_trait_falls_alone(rt, monkeypatch, name):
    """one more object takes exactly its trait from a scene that has all three"""
    monkeypatch.delenv("RT_AMD_KERNEL_VARIANT", raising=False)
    objs = scenes(rt)[name][0]
    extra = {"SPHERES_ONLY": ("quad", (-1, -0.4, 1), (1, -0.4, 1), (1, -0.4, 3), (-1, -0.4, 3), ("standard", (0.6, 0.6, 0.6), 0.3)),
             "PLAIN_MATERIALS": ("sphere", (0.3, 0.2, 1.5), 0.1, ("refractive", (1.0, 1.0, 1.0), 1.5))}
    for trait, o in extra.items():
        f = flatten(rt, list(objs) + [o])
        assert f["traits"] == ALL - {trait} and f["kernel_variant"] == "generic", (name, trait, f["traits"])
    meshes = [("mesh", _soup(5, (0, 0, 2)), ("standard", (0.5, 0.5, 0.5), 0.1))] * (1 if flatten(rt, objs)["num_meshes"] else 2)
    f = flatten(rt, list(objs) + meshes)
    assert f["num_meshes"] == 2 and f["traits"] == ALL - {"ONE_MESH"} and f["kernel_variant"] == "generic"


def test_override_keeps_the_generic_kernel(rt, monkeypatch):
    monkeypatch.setenv("RT_AMD_KERNEL_VARIANT", "generic")
    for name, (objs, _) in scenes(rt).items():
        assert flatten(rt, objs)["kernel_variant"] == "generic", name
    # only that word does it
    monkeypatch.setenv("RT_AMD_KERNEL_VARIANT", "generics")
    assert flatten(rt, scenes(rt)["monkey"][0])["kernel_variant"] == "traits"


def test_image_and_gradient_textures_are_not_plain(rt, monkeypatch):
    monkeypatch.delenv("RT_AMD_KERNEL_VARIANT", raising=False)
    img = np.full((2, 2, 3), 0.5, np.float32)
    for mat in (("gradient", 0.1), ("image", img, 0.0)):
        f = flatten(rt, [("sphere", (0, 0, 2), 0.4, mat)])
        assert f["traits"] == ALL - {"PLAIN_MATERIALS"}, mat[0]
