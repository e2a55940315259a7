"""The ambient-occlusion yardstick (tests/ao_ref.py) held to the oracle's own renderer, without a GPU: with one sample, no bias and an
unlimited radius the count is the oracle's 1 spp frame of the all-white scene (reflection limit 2, antialiasing off, sky 1) - the first
bounce ray escapes or it does not - bit for bit on every pixel.  Then the properties the definition promises: the seed, the prefix
property of the per-pixel stream, a closed box."""
import numpy as np
import pytest

import ao_ref
from test_gpu_query import SCENES

F = np.float32
BIG = ("soup6k", "sphere50k")
CORNELL = ("reference_scene0", "reference_scene1", "reference_scene2", "reference_scene3")


def size_of(name):
    return (32, 24) if name in BIG else (64, 48)


@pytest.mark.parametrize("name", SCENES)
def test_yardstick_equals_the_oracles_renderer(rt, orc, models_dir, name):
    W, H = size_of(name)
    objs, _ = rt.scenes.CONFIG_SCENES[name]()
    white = orc.Scene(ao_ref.whitened(objs), orc.MATH_DET, models_dir)
    cam = rt.Camera(W, H).floats()
    frame = white.render(cam, W, H, 1, 2, (1, 1, 1), time_ms=12345, antialias=False)
    ref = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, 1, np.inf, 0.0, 12345)
    count = ref["count"]
    want = np.where(count == ao_ref.NO_SURFACE, 1, count).astype(F)
    assert set(np.unique(want).tolist()) <= {0.0, 1.0}
    for c in range(3):
        assert np.array_equal(frame[..., c].view(np.uint32), want.view(np.uint32)), (name, c, int((frame[..., c] != want).sum()))
    # the comparison says something: surfaces and sky, escaping and blocked bounce rays (a closed box has no sky and few escapes)
    print("%s: %d surface pixels, %d free, %d blocked" % (name, ref["surface"].sum(), (count == 1).sum(), (count == 0).sum()))
    assert ref["surface"].any() and (count == 0).any()
    assert np.array_equal(ref["ao"].view(np.uint32), want.view(np.uint32))            # one sample: ao is the count, 1 without a surface


def test_seed_changes_the_plane_and_repeats(rt, orc, models_dir):
    W, H = 32, 24
    objs, _ = rt.scenes.monkey()
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    cam = rt.Camera(W, H).floats()
    planes = {tm: ao_ref.ao_reference(orc, oracle, cam, W, H, 4, 0.5, 1e-3, tm) for tm in (12345, 12346, -7)}
    again = ao_ref.ao_reference(orc, oracle, cam, W, H, 4, 0.5, 1e-3, 12345)
    assert again["count"].tobytes() == planes[12345]["count"].tobytes() and again["ao"].tobytes() == planes[12345]["ao"].tobytes()
    assert np.array_equal(again["direction"].view(np.uint32), planes[12345]["direction"].view(np.uint32))
    for a, b in ((12345, 12346), (12345, -7), (12346, -7)):
        assert planes[a]["count"].tobytes() != planes[b]["count"].tobytes(), (a, b)
        # the first hits are the same, the directions are not
        assert np.array_equal(planes[a]["surface"], planes[b]["surface"]) and np.array_equal(planes[a]["origin"].view(np.uint32), planes[b]["origin"].view(np.uint32))
        assert not np.array_equal(planes[a]["direction"].view(np.uint32), planes[b]["direction"].view(np.uint32))
    # a negative time is its two's complement
    assert ao_ref.seed_of(3, 2, W, -7) == ((2 * W + 3) * 3 * 3145739 + (2 ** 32 - 7) * 6291469) % 2 ** 32


@pytest.mark.parametrize("name", ["three_sphere", "monkey"])
def test_prefix_property(rt, orc, models_dir, name):
    """every sample takes six draws whatever it meets: the first four samples of an eight-sample run are the four-sample run"""
    W, H = 64, 48
    eight = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, 8, 0.5, 1e-3, 12345)
    four = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, 4, 0.5, 1e-3, 12345)
    s = eight["surface"]
    assert np.array_equal(s, four["surface"]) and np.array_equal(four["count"] == ao_ref.NO_SURFACE, ~s)
    assert np.array_equal(four["count"][s], eight["free"][..., :4].sum(axis=2)[s])
    assert np.array_equal(four["free"], eight["free"][..., :4])
    assert np.array_equal(four["direction"].view(np.uint32), eight["direction"][:, :, :4].view(np.uint32))
    assert np.array_equal(eight["count"][s], eight["free"].sum(axis=2)[s])
    assert np.array_equal(eight["ao"][s].view(np.uint32), (eight["count"][s].astype(F) / F(8)).view(np.uint32)) and np.all(eight["ao"][~s] == 1)
    # within a radius a sample is free iff the oracle's blocker is beyond it
    with np.errstate(invalid="ignore"):
        assert np.array_equal(eight["free"][s] == 0, eight["hit"][s] & (eight["t"][s] <= F(0.5)))


@pytest.mark.parametrize("name", CORNELL)
def test_closed_box_is_blocked(rt, orc, models_dir, name):
    """A Cornell scene is a sealed box seen through its one-way front: from a surface inside it every direction meets a wall, so with an
    unlimited radius the count is 0.  The exceptions are first hits that do not lie inside (the box's outer faces and rim as the camera
    sees them), a thin frame of the image: at least nine surface pixels in ten are all-blocked."""
    W, H = 64, 48
    ref = ao_ref.scene_reference(rt, orc, models_dir, name, W, H, 1, np.inf, 0.0, 12345)
    s = ref["surface"]
    blocked = int((ref["count"][s] == 0).sum())
    print("%s: %d of %d surface pixels all-blocked" % (name, blocked, int(s.sum())))
    assert s.sum() > 1500 and blocked >= 0.9 * s.sum()
