"""The seeded scene generators of the suite and of the hand-run soaks, in one place, and the rays that go with them.  No product code and no
oracle: a seed gives a neutral scene description (ray-tracer_amd/scenes.py) that both sides consume.  The draws of random_scene are those
tests/test_gpu_parity.py has always made: a seed gives the scene it gave when the soaks under tests/soak/ ran it."""
import numpy as np

MATERIAL_KINDS = ("standard", "emissive", "checkerboard", "gradient", "image", "refractive")
PRIMITIVE_KINDS = ("sphere", "triangle_uv", "quad", "one_way_quad", "cuboid", "obj", "mesh")
MESH_KINDS = ("obj", "mesh")
# where random_scene puts its objects' centres: the box the rays below are aimed around
OBJECT_BOX = ((-1.2, -0.7, 1.0), (1.2, 0.9, 3.5))


def random_scene(seed):
    """a seeded mix of every primitive and material kind, in random list order"""
    rng = np.random.default_rng(seed)

    def vec(lo, hi):
        return tuple(float(x) for x in rng.uniform(lo, hi, 3))

    def material():
        k = rng.integers(0, 7)
        col = vec(0.1, 1.0)
        if k == 0:
            return ("standard", col, float(rng.uniform(0, 1)))
        if k == 1:
            return ("standard", col, 0.0)
        if k == 2:
            return ("emissive", col, float(rng.uniform(0.5, 5)))
        if k == 3:
            return ("checkerboard", col, vec(0, 0.5), int(rng.integers(1, 12)), float(rng.uniform(0, 0.5)))
        if k == 4:
            return ("gradient", float(rng.uniform(0, 0.3)))
        if k == 5:
            return ("refractive", col, float(rng.uniform(1.05, 2.2)))
        return ("image", rng.uniform(0, 1, (int(rng.integers(2, 9)), int(rng.integers(2, 9)), 3)).astype(np.float32), 0.0)

    objs = []
    for _ in range(int(rng.integers(6, 14))):
        kind = rng.integers(0, 7)
        c = np.array(vec([-1.2, -0.7, 1.0], [1.2, 0.9, 3.5]))
        if kind == 0:
            objs.append(("sphere", tuple(c), float(rng.uniform(0.08, 0.45)), material()))
        elif kind == 1:
            p = [tuple(c + rng.normal(0, 0.35, 3)) for _ in range(3)]
            objs.append(("triangle_uv", p, [tuple(rng.uniform(0, 1, 2)) for _ in range(3)], material()))
        elif kind == 2:
            a, b = rng.normal(0, 0.4, 3), rng.normal(0, 0.4, 3)
            objs.append(("quad", tuple(c), tuple(c + a), tuple(c + a + b), tuple(c + b), material()))
        elif kind == 3:
            a, b = rng.normal(0, 0.5, 3), rng.normal(0, 0.5, 3)
            objs.append(("one_way_quad", tuple(c), tuple(c + a), tuple(c + a + b), tuple(c + b), bool(rng.integers(0, 2)), material()))
        elif kind == 4:
            objs.append(("cuboid", tuple(c), float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.1, 0.5)), float(rng.uniform(0.1, 0.5)), material()))
        elif kind == 5:
            objs.append(("obj", "cube.obj", [("enlarge", float(rng.uniform(0.08, 0.25))), ("rotate", *[float(x) for x in rng.uniform(-3, 3, 3)]),
                                             ("translate", *[float(x) for x in c])], material()))
        else:
            n = int(rng.integers(1, 60))
            tris = (c + rng.normal(0, 0.25, (n, 1, 3)) + rng.normal(0, 0.08, (n, 3, 3))).astype(np.float32).reshape(n, 9)
            objs.append(("mesh", tris, material()))
    if rng.integers(0, 2):
        objs.append(("sphere", (0, -100.5, 1.5), 100, ("standard", (0.5, 0.5, 0.5), float(rng.uniform(0, 0.4)))))
    sky = (0.8, 1.0, 1.0) if rng.integers(0, 2) else (0.0, 0.0, 0.0)
    return objs, sky


def random_soup_scene(seed):
    """one or two random triangle soups of 100..3,000 triangles (leaves of the fixed-depth-10 tree then hold several triangles; the larger
    ones do not fit LDS), standard or refractive, an emissive sphere above and, for half the seeds, the ground sphere"""
    rng = np.random.default_rng(seed)
    objs = []
    for _ in range(int(rng.integers(1, 3))):
        n = int(rng.integers(100, 3000))
        c = rng.uniform([-0.8, -0.5, 1.4], [0.8, 0.6, 3.0])
        tris = (c + rng.normal(0, 0.35, (n, 1, 3)) + rng.normal(0, 0.06, (n, 3, 3))).astype(np.float32).reshape(n, 9)
        mat = ("standard", tuple(float(x) for x in rng.uniform(0.2, 1, 3)), float(rng.uniform(0, 0.6))) if rng.integers(0, 3) else ("refractive", (1.0, 1.0, 1.0), 1.5)
        objs.append(("mesh", tris, mat))
    objs.append(("sphere", (0, 1.3, 1.5), 0.5, ("emissive", (1, 1, 1), 5.0)))
    if rng.integers(0, 2):
        objs.append(("sphere", (0, -100.5, 1.5), 100, ("standard", (0.5, 0.5, 0.5), 0.2)))
    sky = (0.8, 1.0, 1.0) if rng.integers(0, 2) else (0.0, 0.0, 0.0)
    return objs, sky


def scene_rays_for(seed, n, W=40, H=30, cam=None):
    """-> origins [n + W*H, 3], directions [n + W*H, 3], n: n random rays whose draws depend on the seed - tests/test_gpu_query._rays with its
    default target (0, 0, 2), which lies in OBJECT_BOX: half the origins at 0, half scattered around the target, inside and outside the
    scene, every ray aimed at a point scattered around it - followed by the W x H primary rays (antialias off) of the camera `cam` (12
    floats; the default camera's unless given)"""
    from test_gpu_query import _rays, primaries
    lo, hi = OBJECT_BOX
    assert all(a <= t <= b for a, t, b in zip(lo, (0.0, 0.0, 2.0), hi))
    o, d = _rays(n, seed)
    if cam is None:
        cam = default_camera(W, H)
    cam = np.asarray(cam, np.float32)
    p = primaries(cam, W, H).reshape(-1, 3)
    return (np.concatenate([o, np.broadcast_to(cam[0:3], p.shape)]).astype(np.float32), np.concatenate([d, p]).astype(np.float32), n)


def default_camera(W, H):
    """the twelve floats of the product's default camera (rt.Camera(W, H).floats(): plain Python over the image size, no device)"""
    import importlib
    return np.asarray(importlib.import_module("ray-tracer_amd").Camera(W, H).floats(), np.float32)


def kinds_of(objs):
    """per object: (primitive kind, material kind)"""
    return [(o[0], o[-1][0]) for o in objs]


def num_meshes(objs):
    return sum(o[0] in MESH_KINDS for o in objs)
