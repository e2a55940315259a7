"""The scenes and rays the multi-hit tests share (tests/test_multihit_ref.py on the CPU, tests/test_gpu_multihit.py on the GPU): each scene's
object list, its seeded rays (multihit_ref.query_rays) and the k values tested on it.  Answers of the yardstick are computed once per
scene and kept (`reference`)."""
import os

import numpy as np

import multihit_ref as R
from random_scenes import random_scene

# name -> (rays, seed of the rays, the k tested there beside count-only).  At most 2,048 rays on the large scenes.  A k is listed where at
# least a tenth of the scene's rays have MORE candidates than it (test_multihit_ref.py asserts that from the yardstick alone), so that the
# threshold prunes and a full buffer overflows; k = 8 is run everywhere on top, for the miss pattern behind a ray's last hit.
SCENES = {
    "three_sphere": (3000, 1, (1,)),
    "cube": (3000, 2, (1, 2)),
    "monkey": (3000, 3, (1, 2, 3)),
    "reference_scene0": (3000, 4, (1, 2, 3)),
    "reference_scene4": (3000, 5, (1, 2, 3)),
    "random13": (3000, 6, (1, 2, 3)),
    "random15": (3000, 7, (1, 2, 3)),
    "tiny_meshes": (3000, 8, (1,)),
    "soup3000": (2048, 9, (1, 2, 3, 8)),
    "soup6k": (2048, 10, (1, 2, 3, 8)),
}
SOUPS = ("soup3000", "soup6k")
# soup6k's triangles are small and spread evenly: a ray of the seeded kind meets more than 8 of them about once in twenty.  Its rays are
# therefore a committed choice (soup6k_rays below made it, from the yardstick alone): of four times as many seeded rays, the first 320
# with more than 8 candidates and the first 1,728 of the others.
SOUP6K_RAYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multihit_rays_soup6k.npy")
_REFS = {}


def soup6k_rays(rt, models_dir):
    """-> [2048, 6] float32: what tests/golden/multihit_rays_soup6k.npy holds (python tests/multihit_ref.py writes it)"""
    n, seed, _ = SCENES["soup6k"]
    flat = rt.SceneObjects(objects_of(rt, "soup6k"), models_dir).debug_flatten()
    o, d = R.query_rays(flat, seed, 4 * n)
    total = R.candidates(flat, o, d).total
    rich, rest = np.nonzero(total > R.MULTIHIT_MAX)[0][:320], np.nonzero(total <= R.MULTIHIT_MAX)[0][:n - 320]
    pick = np.sort(np.concatenate([rich, rest]))
    assert pick.shape[0] == n
    return np.concatenate([o[pick], d[pick]], axis=1).astype(np.float32)


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
    tris = (np.array([0.0, 0.0, 2.2]) + rng.normal(0, 0.4, (3000, 1, 3)) + rng.normal(0, 0.1, (3000, 3, 3))).astype(np.float32).reshape(3000, 9)
    return [("mesh", tris, ("standard", (0.6, 0.6, 0.6), 0.1)), ("sphere", (0.0, 1.3, 1.5), 0.5, ("emissive", (1, 1, 1), 5.0))]


def objects_of(rt, name):
    if name.startswith("random"):
        return random_scene(int(name[6:]))[0]
    if name == "tiny_meshes":
        return tiny_meshes()
    if name == "soup3000":
        return soup3000()
    return rt.scenes.CONFIG_SCENES[name]()[0]


def reference(rt, models_dir, name):
    """dict(flat, o, d, cand) of the scene: its flattened form, its rays and every candidate of every ray in order, from the yardstick alone"""
    if name not in _REFS:
        n, seed, _ = SCENES[name]
        flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
        if name == "soup6k":
            rays = np.load(SOUP6K_RAYS)
            assert rays.shape == (n, 6) and rays.dtype == np.float32
            o, d = np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 3:6])
        else:
            o, d = R.query_rays(flat, seed, n)
        _REFS[name] = {"flat": flat, "o": o, "d": d, "cand": R.candidates(flat, o, d)}
    return _REFS[name]
