"""The conditions on the inputs of tests/test_gpu_random_scenes.py, from the generators and the CPU oracle alone (no GPU): a batch of rays that
nearly all hit or nearly all miss, a seed list without a second mesh or without a textured mesh would let that file pass while testing
little.  A seed that fails a condition is replaced in that file's list; the condition stays."""
import numpy as np
import pytest

import ao_ref
import random_scenes as RS
from test_gpu_occlusion import oracle_visibility
from test_gpu_parity import _random_scene
from test_gpu_random_scenes import (AO, AO_RADII, LIGHTS, PLACED_SEEDS, SCENE_CASES, SEEDS, SOUP_CASES, SOUPS, SPP, H, W, Case, budget_planes, oracle_of,
                                    plane_records, ray_records, view_frames)

F = np.float32
OWN = [c for c in SCENE_CASES if c.placement == "own"]
TEXTURED = ("checkerboard", "gradient", "image")


def same(a, b):
    """two neutral scene descriptions, compared value by value"""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def test_the_moved_generator_makes_the_scenes_it_made():
    """tests/test_gpu_parity.py re-exports the generator; a seed gives one scene whoever asks, twice over; seed 13's first draws are pinned
    (14 objects, five of them meshes, the third object an image-textured cube.obj), so that a reordered draw cannot go unnoticed"""
    assert _random_scene is RS.random_scene
    for seed in (11, 13, 22):
        assert same(RS.random_scene(seed), RS.random_scene(seed)) and same(RS.random_soup_scene(seed), RS.random_soup_scene(seed))
    objs, sky = RS.random_scene(13)
    assert [o[0] for o in objs] == ["mesh", "obj", "obj", "cuboid", "obj", "sphere", "one_way_quad", "quad", "one_way_quad", "cuboid", "mesh", "cuboid",
                                    "triangle_uv", "sphere"]
    assert objs[2][-1][0] == "image" and objs[2][-1][1].shape[2] == 3 and RS.num_meshes(objs) == 5
    assert not same(RS.random_scene(13), RS.random_scene(14))


@pytest.mark.parametrize("case", SCENE_CASES + SOUP_CASES, ids=[c.id for c in SCENE_CASES + SOUP_CASES])
def test_each_scene_is_worth_tracing(rt, orc, models_dir, case):
    """per scene: the oracle answers "hit" for 10 to 90 % of the random rays; its frame at the GPU file's size and settings is finite, and
    light reaches more than half its pixels (a pixel that is 0 whatever the path does compares nothing)"""
    q = ray_records(orc, models_dir, case)
    frac = q["hit"][:q["n"]].mean()
    frame = oracle_of(orc, models_dir, case).render(rt.Camera(W, H).floats(), W, H, SPP, case.limit, case.sky, time_ms=case.time_ms)
    print("%s: %d objects, %d meshes, oracle hits %.1f %% of the %d random rays and %.1f %% of the primary grid" %
          (case.id, len(case.objs), RS.num_meshes(case.objs), 100 * frac, q["n"], 100 * q["hit"][q["n"]:].mean()))
    assert 0.10 <= frac <= 0.90, (case.id, frac)
    assert np.isfinite(frame).all(), case.id
    assert (frame != 0).any(axis=2).sum() > W * H // 2 and frame.std() > 0.05, case.id


def winners(orc, models_dir, case, rt=None):
    """the objects that are some ray's closest hit: of the scene's rays, or (rt given) of the W x H view's primary rays"""
    q = ray_records(orc, models_dir, case) if rt is None else plane_records(rt, orc, models_dir, case)
    hit = q["hit"]
    return set(np.unique(q["rec" if rt is not None else "out"][hit, 7].astype(np.int32)).tolist())


def test_the_seed_list_holds_what_the_config_scenes_lack(rt, orc, models_dir):
    """over the list: at least two thirds of the scenes have two meshes or more; a mesh of each of the six material kinds, and each
    primitive kind, is some ray's closest hit; a one-way quad of either orientation is; and, for the two yardsticks that are new in the
    GPU file, a textured sphere is some ray's closest hit and the W x H view sees a textured mesh, a textured cuboid or quad and a
    refractive and an emissive mesh"""
    assert sum(RS.num_meshes(c.objs) >= 2 for c in OWN) * 3 >= 2 * len(OWN)
    mesh_materials, primitives, one_way, sphere_textures, seen = set(), set(), set(), set(), set()
    for c in OWN:
        kinds = RS.kinds_of(c.objs)
        for k in winners(orc, models_dir, c):
            prim, mat = kinds[k]
            primitives.add(prim)
            if prim in RS.MESH_KINDS:
                mesh_materials.add(mat)
            if prim == "one_way_quad":
                one_way.add(bool(c.objs[k][5]))
            if prim == "sphere" and mat in TEXTURED:
                sphere_textures.add(mat)
        for k in winners(orc, models_dir, c, rt):
            prim, mat = kinds[k]
            seen.add(("mesh" if prim in RS.MESH_KINDS else prim, mat))
    assert mesh_materials == set(RS.MATERIAL_KINDS), mesh_materials
    assert primitives == set(RS.PRIMITIVE_KINDS), primitives
    assert one_way == {False, True}
    assert sphere_textures == set(TEXTURED), sphere_textures
    assert {("mesh", m) for m in RS.MATERIAL_KINDS} <= seen, seen
    assert any(p in ("cuboid", "quad", "one_way_quad") and m in TEXTURED for p, m in seen)


def test_the_placed_seeds_are_the_rich_ones(rt, orc, models_dir):
    """13 and 15 have five and six meshes; meshes with an image, a gradient and a checkerboard texture win hits in them; the filler of the
    global cases comes after every object of the seed and the soups are what their placements need"""
    textures = set()
    for seed, n in zip(PLACED_SEEDS, (5, 6)):
        case = Case("random", seed)
        assert RS.num_meshes(case.objs) == n
        kinds = RS.kinds_of(case.objs)
        textures |= {kinds[k][1] for k in winners(orc, models_dir, case) if kinds[k][0] in RS.MESH_KINDS}
        filled = Case("random", seed, "global")
        assert len(filled.objs) == len(case.objs) + 1 and same(filled.objs[:-1], case.objs) and filled.name != case.name
        assert len(case.objs) in winners(orc, models_dir, filled)                       # the filler is part of the scene, not out of sight
    assert set(TEXTURED) <= textures, textures
    for placement, seed in SOUPS.items():
        objs, _ = RS.random_soup_scene(seed)
        flat = rt.SceneObjects(objs, models_dir).debug_flatten()
        assert flat["num_meshes"] == 2 and "refractive" in [o[-1][0] for o in objs if o[0] == "mesh"], placement
        assert flat["num_triangles"] > 2 * 1024                                          # more triangles than a depth-10 tree has leaves: leaves of several


@pytest.mark.parametrize("case", OWN + SOUP_CASES, ids=[c.id for c in OWN + SOUP_CASES])
def test_each_plane_decides_something(rt, orc, models_dir, case):
    """per scene, from the yardsticks alone: the ambient-occlusion planes have surface pixels and, with the unlimited radius, partly occluded
    ones; blocked and lit pixels both occur in the visibility planes; the budget planes are what their docstring says; the three views'
    frames differ from one another and from the frame they fold into; some ray's closest hit is a triangle"""
    r = {radius: ao_ref.scene_reference(rt, orc, models_dir, case.name, W, H, AO["samples"], radius, AO["bias"], case.time_ms, objs=case.objs) for radius in AO_RADII}
    count = r[np.inf]["count"][r[np.inf]["surface"]]
    partly = int(((count > 0) & (count < AO["samples"])).sum())
    near = r[0.5]["count"][r[0.5]["surface"]]
    oracle = oracle_of(orc, models_dir, case)
    codes = np.concatenate([oracle_visibility(oracle, rt.Camera(W, H).floats(), W, H, light, bias).ravel() for light, bias in LIGHTS])
    print("%s: %d surface pixels, %d partly occluded without a limit, %d occluded at all within 0.5; visibility: blocked %d lit %d no surface %d" %
          (case.id, len(count), partly, int((near < AO["samples"]).sum()), (codes == 0).sum(), (codes == 1).sum(), (codes == 2).sum()))
    assert len(count) >= W * H // 10 and partly >= 10 and (near < AO["samples"]).any(), case.id
    assert (codes == 0).any() and (codes == 1).any(), case.id
    b1, b2 = budget_planes(case)
    for b in (b1, b2):
        assert b.dtype == np.uint16 and sorted(np.unique(b).tolist()) == [0, 1, 2, 3, 4, 5] and (b == 0).sum() > W * H // 10
    assert ((b1 > 0) & (b2 > 0) & (b1 != b2)).sum() > W * H // 3 and ((b1 == 0) & (b2 > 0)).any() and ((b1 > 0) & (b2 == 0)).any()
    if case.kind == "random":
        want, chain = view_frames(rt, orc, models_dir, case)
        assert len({want[i].tobytes() for i in range(len(want))}) == len(want) == 3 and not any(np.array_equal(chain, w) for w in want), case.id
    assert any(o[0] != "sphere" for o in (case.objs[k] for k in winners(orc, models_dir, case))), case.id            # a triangle to name


def test_seed_lists():
    assert len(SEEDS) == len(set(SEEDS)) >= 12 and set(PLACED_SEEDS) <= set(SEEDS)
