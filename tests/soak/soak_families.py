"""One-off soak of every kernel family (test infrastructure, run by hand on the GPU box, not part of -m gpu): the comparisons of
tests/test_gpu_random_scenes.py - closest-hit queries with the oracle's texture coordinates, the first-hit planes with the albedo yardstick,
occlusion queries, the visibility plane, the ambient-occlusion plane, sample budgets, camera sequences - over a range of seeds of
tests/random_scenes.py, every ray and pixel compared bit for bit.  Seed s runs on the shape its scene picks (s % 3 == 0), forced to 1024
threads (1) or from global memory with the filler mesh (2); every tenth seed also runs a triangle soup through the ray families on whatever
placement it gets.  Exits non-zero on a mismatch and prints the seed, the family and the assertion; an error of the runtime ends the run at once.
    python tests/soak/soak_families.py <first seed> <count>"""
import importlib, os, sys, time, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
rt = importlib.import_module("ray-tracer_amd")
from oracle import binding as orc
import ao_ref
import test_gpu_random_scenes as T

first, count = int(sys.argv[1]), int(sys.argv[2])
orc.build()
ctx = rt.Context(0)
md = rt.scenes.models_dir()
KNOBS = ("RT_AMD_THREADS", "RT_AMD_SCENE_MODE", "RT_AMD_BLOCKS_PER_CU")
PLACEMENTS = ("own", "threads1024", "global")


def commit(case):
    """the scene committed under its placement's environment (read by rt_scene_commit), the environment put back"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(T.ENVS[case.placement] if case.kind == "random" else {})
    try:
        return ctx.commit(rt.SceneObjects(case.objs, md))
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


bad, ran, shapes, t0 = 0, 0, {}, time.time()
for seed in range(first, first + count):
    cases = [(T.Case("random", seed, PLACEMENTS[seed % 3]), T.FAMILIES)]
    if seed % 10 == 0:
        cases.append((T.Case("soup", seed), T.SOUP_FAMILIES))
    for case, families in cases:
        scene = commit(case)
        info = scene.info()
        shape = "%s %s-%d" % (case.kind, {0: "global", 1: "lds", 2: "hybrid"}[info["scene_in_lds"]], info["threads_per_block"])
        shapes[shape] = shapes.get(shape, 0) + 1
        for family in families:
            try:
                T.FAMILIES[family](rt, orc, ctx, md, case, scene)
                ran += 1
            except AssertionError:
                bad += 1
                print("MISMATCH seed %d (%s, %s) family %s\n%s" % (seed, case.id, shape, family, traceback.format_exc(limit=-2)), flush=True)
            except Exception:
                print("ERROR seed %d (%s, %s) family %s: stopping\n%s" % (seed, case.id, shape, family, traceback.format_exc()), flush=True)
                sys.exit(2)
        del scene
    T._REFS.clear()
    ao_ref._CACHE.clear()
    if (seed - first + 1) % 50 == 0:
        print("... %d seeds, %d family runs, %d mismatches so far, %.0f s" % (seed - first + 1, ran + bad, bad, time.time() - t0), flush=True)     # a long run must not look hung
print("soak: seeds %d..%d, %d family runs, %d mismatches, %.0f s; scenes per shape: %s" % (first, first + count - 1, ran + bad, bad, time.time() - t0,
                                                                                          ", ".join("%s: %d" % kv for kv in sorted(shapes.items()))), flush=True)
sys.exit(1 if bad else 0)
