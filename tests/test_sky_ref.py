"""Pins tests/sky_ref.py, the yardstick of the cube-map sky, without a GPU and without the feature's device code.  Its bounce loop against
the oracle's own renderer: under a constant map c with tint s every miss adds fl(c * s) times the throughput, so the yardstick's frames
must be oracle.render(sky = fl(c * s)) as uint32, on the scenes of tests/test_gpu_views.py and on the random scenes that hold refractive
and textured objects.  The mapping: the lookup of every texel's direction (rt_sky_texel_direction's restatement) is the texel again - also
normalised, also scaled by 1e-3f - exhaustively for the face sizes include/rt_amd.h's definition was checked on.  And sky_from_equirect,
the NumPy convenience of the binding, on images whose cube map is known."""
import numpy as np
import pytest

import sky_ref as S
from random_scenes import kinds_of, random_scene
from test_gpu_shapes import scene_of
from test_gpu_views import SCENES

F = np.float32
W, H, SPP, LIMIT = 23, 13, 2, 5                     # 3 x 2 tiles' worth of pixels, ragged; the loop is Python per sample
TIMES = [12345, -99]
MAP, TINT = (0.7, 1.3, 0.05), (0.9, 0.5, 3.0)      # fl(c * s) is rounded in two of the channels
TEXTURED = {"checkerboard", "gradient", "image"}
RANDOM_SEEDS = [s for s in range(11, 23) if "refractive" in {m for _, m in kinds_of(random_scene(s)[0])} and TEXTURED & {m for _, m in kinds_of(random_scene(s)[0])}]
ROUND_TRIP_SIZES = list(range(1, 66)) + [100, 255, 256, 1000, 1023, 1024, 2047, 2048]


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def cameras(rt):
    return [rt.Camera(W, H).floats(), rt.Camera(W, H, pos=(0.2, 0.0, 0.1), rot=(0.05, -0.2, 0.1)).floats()]


def check_against_the_oracle(rt, orc, models_dir, objs, what):
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    faces = np.broadcast_to(np.asarray(MAP, F), (6, 2, 2, 3))
    sky = np.asarray(MAP, F) * np.asarray(TINT, F)
    means, reads = zip(*[S.view_means(orc, oracle, objs, c, W, H, SPP, LIMIT, TINT, t, True, faces) for c, t in zip(cameras(rt), TIMES)])
    want = [oracle.render(c, W, H, SPP, LIMIT, sky, time_ms=t, frame_num=0) for c, t in zip(cameras(rt), TIMES)]
    got = S.separate(means)
    for i in range(len(want)):
        diff = (u32(got[i]) != u32(want[i])).any(axis=2)
        assert not diff.any(), (what, "view", i, "pixels that differ", int(diff.sum()), np.argwhere(diff)[:5].tolist())
    chain = oracle.render(cameras(rt)[1], W, H, SPP, LIMIT, sky, time_ms=TIMES[1], frame_num=1, prev=want[0])
    assert np.array_equal(u32(S.accumulated(means)), u32(chain)), (what, "accumulated")
    five = oracle.render(cameras(rt)[1], W, H, SPP, LIMIT, sky, time_ms=TIMES[1], frame_num=5, prev=want[0])
    assert np.array_equal(u32(S.accumulated(means[1:], frame_num=5, prev=want[0])), u32(five)), (what, "frame 5 over a previous frame")
    return np.concatenate([r.reshape(-1, 3) for r in reads])


@pytest.mark.parametrize("name", SCENES)
def test_yardstick_equals_the_oracle_under_a_constant_map(rt, orc, models_dir, name):
    objs, _ = scene_of(rt, name)
    reads = check_against_the_oracle(rt, orc, models_dir, objs, name)
    assert (reads[:, 0] >= 0).any(), (name, "no sample reached the sky")


def test_the_random_seeds_hold_what_they_are_chosen_for():
    assert len(RANDOM_SEEDS) >= 3, RANDOM_SEEDS


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_yardstick_equals_the_oracle_on_random_scenes(rt, orc, models_dir, seed):
    check_against_the_oracle(rt, orc, models_dir, random_scene(seed)[0], seed)


def test_a_wrong_loop_does_not_pass(rt, orc, models_dir):
    """the pin tells: the same comparison with the draws of the jitter left out differs"""
    objs, _ = scene_of(rt, "three_sphere")
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    faces = np.broadcast_to(np.asarray(MAP, F), (6, 1, 1, 3))
    sky = np.asarray(MAP, F) * np.asarray(TINT, F)
    cam = cameras(rt)[0]
    mean, _ = S.view_means(orc, oracle, objs, cam, W, H, SPP, LIMIT, TINT, TIMES[0], False, faces)
    assert not np.array_equal(u32(S.fold(None, mean, 0)), u32(oracle.render(cam, W, H, SPP, LIMIT, sky, time_ms=TIMES[0])))
    assert np.array_equal(u32(S.fold(None, mean, 0)), u32(oracle.render(cam, W, H, SPP, LIMIT, sky, time_ms=TIMES[0], antialias=False)))


# ---- the mapping ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROUND_TRIP_SIZES)
def test_the_lookup_of_a_texels_direction_is_the_texel(n):
    """every texel, face by face: as rt_sky_texel_direction gives the direction, normalised as rt_vec.h normalises, and scaled by 1e-3f"""
    directions = S.texel_directions(n)
    rows, cols = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for face in range(6):
        d = directions[face]
        for what, v in (("as given", d), ("normalised", S.normalised_rows(d)), ("scaled", d * F(1e-3))):
            f, r, c = S.lookup(v, n)
            ok = (f == face) & (r == rows) & (c == cols)
            assert ok.all(), (n, face, what, np.argwhere(~ok)[:5].tolist())


def test_the_lookup_on_special_directions():
    nan, inf = F(np.nan), F(np.inf)
    # ties go to the earlier axis; -0 is the positive face; a NaN compares false
    cases = [((1, 1, 1), 0), ((-1, 1, 1), 1), ((0.5, 1, 1), 2), ((0.5, -1, 1), 3), ((0.5, 0.5, 1), 4), ((0, 0, -1), 5), ((-0.0, 0, 0), 0), ((0, 0, 0), 0),
             ((nan, 1, 0), 2), ((nan, nan, nan), 4), ((1, nan, 0), 4), ((inf, 1, 1), 0), ((-inf, inf, 0), 1)]
    for n in (1, 2, 7, 2048):
        for d, face in cases:
            f, r, c = S.lookup(np.asarray(d, F), n)
            assert int(f) == face and 0 <= int(r) < n and 0 <= int(c) < n, (n, d, int(f), int(r), int(c))
    assert [int(v) for v in S.lookup(np.asarray((1, -1, 1), F), 4)] == [0, 3, 0]            # X: (a, b) = (y, z): col from y, row from z
    assert [int(v) for v in S.lookup(np.asarray((0.5, 1, -1), F), 4)] == [2, 3, 0]            # Y: (z, x)
    assert [int(v) for v in S.lookup(np.asarray((-1, 0.9, 2), F), 4)] == [4, 2, 1]          # Z: (x, y)


# ---- sky_from_equirect ------------------------------------------------------------------------------------------------------------------------
def test_equirect_of_a_constant_image_is_constant(rt):
    image = np.broadcast_to(np.asarray((0.25, 2.0, 7.5), F), (5, 9, 3))
    for n in (1, 3, 16):
        faces = rt.sky_from_equirect(image, n)
        assert faces.shape == (6, n, n, 3) and faces.dtype == np.float32 and (faces == np.asarray((0.25, 2.0, 7.5), F)).all()


def test_equirect_of_a_white_top_and_black_bottom(rt):
    """the +Y face white, the -Y face black, the side faces split along y = 0: on +-Z between two rows (y is the row's coordinate there), on +-X
    between two columns (y is the column's)"""
    n = 8
    image = np.zeros((4, 6, 3), F)
    image[:2] = 1.0
    faces = rt.sky_from_equirect(image, n)
    assert (faces[2] == 1.0).all() and (faces[3] == 0.0).all()
    for face in (4, 5):
        assert (faces[face, n // 2:] == 1.0).all() and (faces[face, :n // 2] == 0.0).all(), face
    for face in (0, 1):
        assert (faces[face, :, n // 2:] == 1.0).all() and (faces[face, :, :n // 2] == 0.0).all(), face
    with pytest.raises(ValueError):
        rt.sky_from_equirect(np.zeros((4, 6)), n)
    with pytest.raises(ValueError):
        rt.sky_texel_directions(0)
    assert np.array_equal(u32(rt.sky_texel_directions(5)), u32(S.texel_directions(5)))
