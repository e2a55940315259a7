"""Properties of the adaptive sampling yardstick alone (tests/adaptive_ref.py: the definitions of rt_render_budget, rt_adaptive_plan_device and
rt_render_adaptive in NumPy float32 over the CPU oracle's renderer), and one quality measurement made with it.  CPU tests: the library is
not called."""
import numpy as np
import pytest

import adaptive_ref as R

F = np.float32
W, H, LIMIT = 37, 21, 5


def u32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def three_sphere(rt, orc, models_dir):
    objs, sky = rt.scenes.three_sphere()
    return orc.Scene(objs, orc.MATH_DET, models_dir), orc.camera_default(W, H), sky


def test_a_uniform_budget_from_nothing_is_the_oracles_frame(three_sphere):
    oracle, cam, sky = three_sphere
    for n, seed in ((1, 12345), (5, -7)):
        want = oracle.render(cam, W, H, n, LIMIT, sky, time_ms=seed)
        frame, count = R.budget_render(oracle, cam, W, H, np.full((H, W), n, np.uint16), LIMIT, sky, seed)
        assert np.array_equal(u32(frame), u32(want)) and np.all(count == n)
        # zero counts given explicitly, over a frame of garbage: the same
        frame, count = R.budget_render(oracle, cam, W, H, np.full((H, W), n, np.uint16), LIMIT, sky, seed, np.full((H, W, 3), 7.0, F), np.zeros((H, W), np.uint32))
        assert np.array_equal(u32(frame), u32(want)) and np.all(count == n)


def test_mixed_budgets_select_per_pixel_and_zero_touches_nothing(three_sphere):
    oracle, cam, sky = three_sphere
    rng = np.random.default_rng(3)
    budget = rng.choice(np.array([0, 0, 1, 2, 5], np.uint16), size=(H, W))
    old = np.full((H, W, 3), 7.0, F)
    frame, count = R.budget_render(oracle, cam, W, H, budget, LIMIT, sky, 99, old, np.zeros((H, W), np.uint32))
    for n in (1, 2, 5):
        want = oracle.render(cam, W, H, n, LIMIT, sky, time_ms=99)
        assert np.array_equal(u32(frame[budget == n]), u32(want[budget == n]))
    assert np.all(frame[budget == 0] == 7.0) and np.array_equal(count, budget.astype(np.uint32))
    # a second call folds by sample counts: (c * n + frame * m) / (n + m), each operation rounded once
    again, count2 = R.budget_render(oracle, cam, W, H, budget, LIMIT, sky, 100, frame, count)
    c = R.pixel_means(oracle, cam, W, H, budget, LIMIT, sky, 100)
    y, x = np.argwhere(budget == 5)[0]
    want = F(F(F(c[y, x, 1] * F(5)) + F(frame[y, x, 1] * F(5))) / F(10))
    assert u32(again[y, x, 1]) == u32(want) and count2[y, x] == 10 and np.all(again[budget == 0] == 7.0)


def test_an_infinite_threshold_is_the_pilot_only(three_sphere):
    oracle, cam, sky = three_sphere
    frame, count, stats, (A, B, c) = R.render_adaptive(oracle, cam, W, H, LIMIT, sky, 12345, dict(pilot_spp=3, step_spp=2, max_spp=9, max_passes=4, threshold=np.inf))
    a = oracle.render(cam, W, H, 3, LIMIT, sky, time_ms=12345)
    b = oracle.render(cam, W, H, 3, LIMIT, sky, time_ms=12346)
    assert np.array_equal(u32(A), u32(a)) and np.array_equal(u32(B), u32(b)) and np.array_equal(u32(frame), u32((a + b) * F(0.5)))
    assert np.all(count == 6) and stats == {"passes": 0, "active_tiles": [], "total_samples": 6 * W * H}
    # ... and so is max_passes = 0 with any threshold
    frame0, count0, stats0, _ = R.render_adaptive(oracle, cam, W, H, LIMIT, sky, 12345, dict(pilot_spp=3, step_spp=2, max_spp=9, max_passes=0, threshold=1e-9))
    assert np.array_equal(u32(frame0), u32(frame)) and np.array_equal(count0, count) and stats0 == stats


def test_a_tiny_threshold_ends_every_pixel_at_max_spp(three_sphere):
    oracle, cam, sky = three_sphere
    p = dict(pilot_spp=2, step_spp=3, max_spp=9, max_passes=8, threshold=1e-30, pixel_threshold=1e-30)
    _, count, stats, (A, B, c) = R.render_adaptive(oracle, cam, W, H, LIMIT, sky, 5, p)
    # 2, 5, 8, then the remaining 1: three passes over every tile, and the fourth plan finds nothing active.  Tiles whose two half
    # buffers agree to the bit (the sky: every sample is the sky colour) have no error at all and stop at the pilot
    e = R.pixel_error(A, B, R.DEFAULTS["floor"])
    noisy = (R.tiles_of(e) > 0).any(axis=1)
    tile_count = R.tiles_of(c, 9)
    assert np.all(tile_count[noisy] == 9) and noisy.sum() >= 4
    assert stats["passes"] == 3 and stats["active_tiles"][0] >= noisy.sum() and np.all(count == 2 * c) and count.max() == 18
    assert stats["total_samples"] == int(count.sum())


def test_the_butterfly_is_the_pairwise_tree():
    rng = np.random.default_rng(1)
    v = (rng.random((500, 64), dtype=F) * F(10.0)) ** 3
    v[::7, rng.integers(0, 64, 72)] = 0.0
    b = R.butterfly_sum(v)
    assert np.all(u32(b) == u32(b[:, :1]))                           # every slot ends with the same bits
    assert np.array_equal(u32(b[:, 0]), u32(R.tree_sum(v)))
    # it is a particular order: the running sum differs from it somewhere
    running = v[:, 0].copy()
    for k in range(1, 64):
        running = running + v[:, k]
    assert not np.array_equal(u32(running), u32(b[:, 0]))
    # infinities go through, and a tile of one pixel is that pixel
    v[3, 17] = np.inf
    assert np.isinf(R.butterfly_sum(v)[3, 0]) and np.isinf(R.tree_sum(v)[3])
    one = np.zeros((1, 64), F)
    one[0, 0] = 0.3
    assert u32(R.butterfly_sum(one)[0, 0]) == u32(F(0.3))


def test_plan_by_hand():
    """two tiles side by side (12 x 8: the second is ragged), errors placed by hand"""
    A = np.full((8, 12, 3), 1.0, F)
    B = A.copy()
    B[2, 3] = 0.0                                                   # one noisy pixel in tile 0: num = 3, I = 0.5, s = 1.5
    A[0, 9, 0] = np.nan                                             # a NaN pixel in tile 1: e = 0
    count = np.full((8, 12), 4, np.uint32)
    count[5, 5] = 10                                                # at max_spp: never active
    count[7, 0] = 9
    p = dict(step_spp=4, max_spp=10, threshold=0.02, pixel_threshold=np.inf, floor=0.01)
    budget, E, active, e = R.plan(A, B, count, **p)
    e0 = F(3.0) / np.sqrt(F(1.5))
    assert u32(e[2, 3]) == u32(e0) and e[0, 9] == 0 and np.count_nonzero(e) == 1
    assert u32(E[0]) == u32(e0 / F(64)) and E[1] == 0 and E[0] > p["threshold"]
    assert active.tolist() == [63, 0] and not budget[:, 8:].any()
    assert budget[5, 5] == 0 and budget[7, 0] == 1 and budget[0, 0] == 4 and (budget[:, :8] == 4).sum() == 62
    # the pixel rule alone: a high tile threshold, a pixel threshold below e0
    budget, E, active, _ = R.plan(A, B, count, **dict(p, threshold=1.0, pixel_threshold=1.0))
    assert active.tolist() == [1, 0] and budget[2, 3] == 4 and budget.sum() == 4
    assert R.tile_list_of(np.array([0.5, 0.5, 0.7, 0.1], F), np.array([1, 2, 3, 0])) == [2, 0, 1]


# scene -> (RMSE of the adaptive frame) / (RMSE of a uniform frame with the same number of samples, rounded up), as measured
MEASURED = {"cube": 0.881, "monkey": 0.743}


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_adaptive_against_uniform_at_equal_samples(rt, orc, models_dir, name):
    """The one quality figure, from the CPU oracle alone (deterministic): 128 x 128, default camera, 8 bounces, target 1024 spp (seed 777); the
    adaptive loop with the library's defaults (seed 12345) against a uniform render (seed 4242) at its mean samples per pixel, rounded up.
        cube:    16 passes, 60.8 samples per pixel on average (uniform: 61); RMSE 0.00858 against 0.00974: ratio 0.881
        monkey:  16 passes, 223.4 (224); RMSE 0.03570 against 0.04803: ratio 0.743
    (three-sphere, not asserted: 142.5 (143), 0.01077 against 0.01166: 0.924.)  Adaptive wins on both, by the gap 1 - ratio; asserted is the
    measured ratio to within a tenth of that gap, both ways, so the yardstick cannot drift unseen."""
    S = 128
    objs, sky = rt.scenes.CONFIG_SCENES[name]()
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    cam = orc.camera_default(S, S)
    target = oracle.render(cam, S, S, 1024, 8, sky, time_ms=777)
    frame, count, stats, _ = R.render_adaptive(oracle, cam, S, S, 8, sky, 12345, {})
    spp = -(-stats["total_samples"] // (S * S))
    uniform = oracle.render(cam, S, S, spp, 8, sky, time_ms=4242)
    ra, ru = R.rmse(frame, target), R.rmse(uniform, target)
    print("%s: %d passes, %.1f samples per pixel (uniform %d), RMSE %.5f against %.5f: ratio %.4f" % (name, stats["passes"], stats["total_samples"] / (S * S), spp, ra, ru, ra / ru))
    gap = 1.0 - MEASURED[name]
    assert abs(ra / ru - MEASURED[name]) <= gap / 10, (name, ra, ru, ra / ru)
