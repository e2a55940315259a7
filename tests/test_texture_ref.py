"""The albedo yardstick (tests/texture_ref.py) held to the oracle's own renderer, without a GPU.  For one convex object alone the second
ray always escapes to the sky, so under sky (1,1,1) the oracle's 1-spp, limit-2, antialias-off frame is 1 * c * 1 = the texture colour c
at the first hit (oracle/rt_oracle_core.inc, trace_ray): the trick tests/test_gpu_query.py::test_albedo_of_a_lone_convex_object_is_the_
oracle_frame rests on.  Here the yardstick, fed with the (u, v) of Scene.trace_one_uv, must give that frame on every hit pixel as uint32.

What it would catch: a checkerboard parity taken before the float -> int conversion, u and v swapped in the image index, (w - 1) and
(h - 1) swapped or w used for the row stride of a non-square image (the image is 5 x 7), a texel rounded instead of truncated, a
gradient's channels permuted.  The triangle's texture coordinates are three unequal pairs, so barycentric weights given to the wrong
vertex move (u, v) too."""
import numpy as np
import pytest

import texture_ref
from test_gpu_query import primaries, u32

F = np.float32
W, H = 160, 120
LONE = {
    "sphere": ("sphere", (0, 0, 1.5), 0.5),
    "quad": ("quad", (-0.5, 0.5, 1.5), (0.5, 0.5, 1.5), (0.5, -0.5, 1.7), (-0.5, -0.5, 1.7)),
    "triangle_uv": ("triangle_uv", [(-0.7, 0.6, 1.5), (0.8, 0.4, 1.8), (0.0, -0.7, 1.6)], [(0.1, 0.2), (0.9, 0.1), (0.4, 0.95)]),
}
IMG = np.random.default_rng(1).random((5, 7, 3)).astype(np.float32)
MATERIALS = {"checkerboard": ("checkerboard", (0.9, 0.8, 0.1), (0.1, 0.2, 0.3), 8, 0.0), "gradient": ("gradient", 0.5), "image": ("image", IMG, 0.2)}


_LONE = {}


def lone_object(rt, orc, models_dir, shape, material):
    """once per (shape, material): the oracle's frame of the object alone and, for its own primary rays, trace_one_uv's hit flags and
    records; the facts about the frame that make the trick valid are asserted here"""
    key = (shape, material)
    if key not in _LONE:
        objs = [LONE[shape] + (MATERIALS[material],)]
        cam = rt.Camera(W, H).floats()
        oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
        frames = [oracle.render(cam, W, H, 1, 2, (1, 1, 1), time_ms=t, antialias=False) for t in (12345, 999)]
        assert np.array_equal(u32(frames[0]), u32(frames[1]))                      # no second ray ever lands: the frame does not depend on the seed
        flat = frames[0].reshape(-1, 3)
        assert not np.isnan(flat).any()
        sky = (flat == 1).all(axis=1)
        assert 0.3 < sky.mean() < 0.9, sky.mean()
        colours = len(np.unique(flat[~sky], axis=0))
        assert colours == 2 if material == "checkerboard" else (colours > 1000 if material == "gradient" else 8 <= colours <= 35), colours
        # the winner's texture coordinates, from the oracle's closest-hit query on the frame's own primary rays
        d = primaries(cam, W, H).reshape(-1, 3)
        origin = np.asarray(cam[0:3], F)
        hit, rec = np.zeros(W * H, bool), np.zeros((W * H, 10), F)
        for i in range(W * H):
            hit[i], rec[i] = oracle.trace_one_uv(origin, d[i])
        assert np.array_equal(hit, ~sky)                                            # a hit pixel is never white: no colour here is (1, 1, 1)
        assert np.all(rec[hit, 7] == 0)
        assert len(np.unique(rec[hit, 8])) > 80 and len(np.unique(rec[hit, 9])) > 80 and len(np.unique(rec[hit, 8:10], axis=0)) > 1000      # (the quad's v is one value per image row)
        _LONE[key] = (flat[hit], rec[hit, 8], rec[hit, 9])
    return _LONE[key]


@pytest.mark.parametrize("shape", list(LONE))
@pytest.mark.parametrize("material", list(MATERIALS))
def test_yardstick_equals_the_oracle_frame_of_a_lone_object(rt, orc, models_dir, shape, material):
    mat = MATERIALS[material]
    frame, u, v = lone_object(rt, orc, models_dir, shape, material)
    want = texture_ref.texture_colour(mat, u, v)
    assert want.dtype == np.float32 and want.shape == frame.shape
    bad = (u32(want) != u32(frame)).any(axis=1)
    assert not bad.any(), (shape, material, int(bad.sum()), np.flatnonzero(bad)[:5].tolist())
    assert np.array_equal(u32(texture_ref.albedo(mat, u, v)), u32(want))


@pytest.mark.parametrize("shape", list(LONE))
def test_the_pin_tells_wrong_lookups_apart(rt, orc, models_dir, shape):
    """the comparison above has teeth: each of these wrong lookups, fed the same (u, v), differs from the oracle's frame on some pixel of
    every lone object - u and v swapped, a coordinate rounded to the nearest cell or texel instead of truncated, an image indexed with
    (h - 1) for u and (w - 1) for v, or with its height as the row stride"""
    def differs(material, wrong):
        frame, u, v = lone_object(rt, orc, models_dir, shape, material)
        return bool((u32(wrong(MATERIALS[material], u, v)) != u32(frame)).any())

    cb, img = MATERIALS["checkerboard"], IMG
    h, w = img.shape[:2]
    assert differs("gradient", lambda m, u, v: texture_ref.texture_colour(m, v, u))
    assert differs("image", lambda m, u, v: texture_ref.texture_colour(m, v, u))
    half = F(0.5)
    assert differs("checkerboard", lambda m, u, v: texture_ref.texture_colour(m, u + half / F(cb[3]), v + half / F(cb[3])))
    assert differs("image", lambda m, u, v: texture_ref.texture_colour(m, u + half / F(w - 1), v + half / F(h - 1)))
    assert differs("image", lambda m, u, v: texture_ref.texture_colour(m, u * (F(h - 1) / F(w - 1)), v * (F(w - 1) / F(h - 1))))
    tall = ("image", np.ascontiguousarray(img.reshape(w, h, 3)), 0.0)                # the same texels read with the row stride h
    assert differs("image", lambda m, u, v: texture_ref.texture_colour(tall, u * (F(w - 1) / F(h - 1)), v * (F(h - 1) / F(w - 1))))


def test_conversions_and_clamps():
    """the corners of the definition that no lone object reaches: NaN and out-of-range coordinates (a sphere's u is NaN at its pole; a
    triangle's barycentric blend may leave [0, 1] by an ulp), the sign of C's %, constant colours and emitted light"""
    nan, inf = F(np.nan), F(np.inf)
    assert texture_ref.f2i(np.array([nan, 3e9, -3e9, -0.9, 0.9, -1.5, 2147483520.0, inf, -inf], F)).tolist() == \
        [0, 2 ** 31 - 1, -2 ** 31, 0, 0, -1, 2147483520, 2 ** 31 - 1, -2 ** 31]
    light, dark = (0.9, 0.8, 0.1), (0.1, 0.2, 0.3)
    cb = ("checkerboard", light, dark, 4, 0.0)
    u = np.array([0.1, 0.3, -0.3, -0.3, nan, 3e9, 3e9], F)
    v = np.array([0.1, 0.1, 0.1, 0.3, 0.3, 0.1, 3e9], F)
    # cells (0,0) light; (1,0) dark; (-1,0): -1 % 2 != 0, dark; (-1,1): 0, light; (0,1) dark; INT_MAX + 0 odd: dark; INT_MAX + INT_MAX wraps to -2: light
    want = [light, dark, dark, light, dark, dark, light]
    assert np.array_equal(texture_ref.texture_colour(cb, u, v), np.asarray(want, F))
    img = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)          # h = 2, w = 3: texel k holds (3k, 3k + 1, 3k + 2)
    im = ("image", img, 0.0)
    u = np.array([0.0, 0.49, 0.5, 1.0, 1.0, 0.0, -5.0, 9.0, nan, 0.9999], F)
    v = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 9.0, 1.0, 0.9999], F)
    texel = [0, 0, 1, 2, 5, 3, 0, 5, 3, 1]
    assert np.array_equal(texture_ref.texture_colour(im, u, v)[:, 0], np.asarray(texel, F) * 3)
    z = np.zeros(4, F)
    assert np.array_equal(texture_ref.texture_colour(("gradient", 0.1), u[:4], v[:4]), np.stack([u[:4], v[:4], z], axis=-1))
    for m in (("standard", (0.25, 0.5, 0.75), 0.3), ("refractive", (0.25, 0.5, 0.75), 1.5)):
        assert np.array_equal(texture_ref.albedo(m, z, z), np.broadcast_to(np.asarray((0.25, 0.5, 0.75), F), (4, 3)))
    got = texture_ref.albedo(("emissive", (0.1, 0.7, 0.3), 3.3), z, z)
    assert got.dtype == np.float32 and np.array_equal(got[0], np.asarray((0.1, 0.7, 0.3), F) * F(3.3))
    with pytest.raises(ValueError):
        texture_ref.texture_colour(("emissive", (1, 1, 1), 2), z, z)
