"""The scenes and balls the sphere-cast tests share (tests/test_sweep_ref.py on the CPU, tests/test_gpu_sweep.py on the GPU): each scene's
object list and its seeded balls (sweep_ref.query_sweeps, then a few inputs that are not valid).  Answers of the yardstick - without
limits, and under the per-ball limits of limits_for - are computed once per scene and kept (`reference`)."""
import numpy as np

import multihit_scenes as MS
import sweep_ref as R

# name -> (balls, seed of the balls).  At most 3,000 per scene and 2,048 on the large ones, so that the yardstick stays within seconds.
SCENES = {
    "three_sphere": (3000, 1),
    "cube": (3000, 2),
    "monkey": (3000, 3),
    "reference_scene0": (3000, 4),
    "reference_scene4": (3000, 5),
    "random13": (3000, 6),
    "random15": (3000, 7),
    "tiny_meshes": (3000, 8),
    "soup3000": (2048, 9),
    "soup6k": (2048, 10),
    "spheres_beyond_lds": (1024, 11),         # (needs a GPU to be sized: the shapes test alone uses it)
}
MESH_SCENES = ("cube", "monkey", "reference_scene0", "random13", "random15", "tiny_meshes", "soup3000", "soup6k")
ONE_WAY_FREE = ("three_sphere", "monkey", "tiny_meshes", "soup3000", "soup6k")       # scenes without one-way quads: the r = 0 comparison with the oracle
_REFS = {}


def objects_of(rt, name):
    if name == "spheres_beyond_lds":
        from test_gpu_shapes import spheres_beyond_lds
        return rt.scenes.reference_scene4(num_spheres=spheres_beyond_lds(rt))[0]
    return MS.objects_of(rt, name)


def invalid_balls():
    """(origins, directions, radius) that give a miss whatever the scene: origins and directions that are not finite, zero directions, radii
    that are NaN, negative or infinite"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    o = np.array([[nan, 0, 0], [0, inf, 1], [1, 2, -inf], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [nan, 0, 1], [0, inf, 0], [1, 1, -inf], [0, 0, 0], [-0.0, 0, -0.0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], np.float32)
    r = np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, nan, -0.25, inf, -inf], np.float32)
    return o, d, r


def limits_for(key):
    """per ball, in turn: the winner's key (1 where there is none), one ulp below it, one ulp above it, 0, negative, NaN, +Inf"""
    lim = np.where(np.isnan(key), np.float32(1), key).astype(np.float32)
    k = np.arange(lim.shape[0]) % 7
    lim[k == 1] = np.nextafter(lim[k == 1], np.float32(-np.inf))
    lim[k == 2] = np.nextafter(lim[k == 2], np.float32(np.inf))
    lim[k == 3] = 0.0
    lim[k == 4] = -0.5
    lim[k == 5] = np.nan
    lim[k == 6] = np.inf
    return lim


def reference(rt, models_dir, name):
    """dict of the scene: flat, o, d, r, free and detail (the records without a limit array and what sweep_ref says about them), lim and
    limited (the per-ball limits and the records under them), n_seeded (the balls ahead of the invalid ones)"""
    if name not in _REFS:
        n, seed = SCENES[name]
        flat = rt.SceneObjects(objects_of(rt, name), models_dir).debug_flatten()
        io, id_, ir = invalid_balls()
        o, d, r = R.query_sweeps(flat, seed, n - io.shape[0])
        o, d, r = np.concatenate([o, io]), np.concatenate([d, id_]), np.concatenate([r, ir])
        (free, detail), = R.sweep_many(flat, o, d, r, [None])
        lim = limits_for(detail["key"])
        (limited, limited_detail), = R.sweep_many(flat, o, d, r, [lim])
        assert (free["object"][n - io.shape[0]:] == -1).all() and not detail["valid"][n - io.shape[0]:].any(), name
        _REFS[name] = {"flat": flat, "o": o, "d": d, "r": r, "free": free, "detail": detail, "lim": lim, "limited": limited,
                       "limited_detail": limited_detail, "n_seeded": n - io.shape[0]}
    return _REFS[name]
