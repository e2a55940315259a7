"""Properties of the camera-sequence yardstick alone (tests/views_ref.py: one oracle render per view, chained for the accumulate mode; the
thin-lens camera in NumPy float32).  CPU tests: the library is not called."""
import numpy as np
import pytest

import views_ref as R

F = np.float32
W, H, SPP, LIMIT = 37, 21, 3, 5


def u32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def three_sphere(rt, orc, models_dir):
    objs, sky = rt.scenes.three_sphere()
    return orc.Scene(objs, orc.MATH_DET, models_dir), orc.camera_default(W, H), sky


def test_identical_cameras_accumulate_to_the_oracles_progressive_frames(three_sphere):
    oracle, cam, sky = three_sphere
    times = [12345, -99, 777, 31337]
    prev, frames = None, []
    for i, t in enumerate(times):
        prev = oracle.render(cam, W, H, SPP, LIMIT, sky, time_ms=t, frame_num=i, prev=prev)
        frames.append(prev.copy())
    got = R.accumulated(oracle, [cam] * 4, W, H, SPP, LIMIT, sky, times)
    assert np.array_equal(u32(got), u32(frames[3]))
    # in two calls, the second going on from the first's frame
    first = R.accumulated(oracle, [cam] * 2, W, H, SPP, LIMIT, sky, times[:2])
    assert np.array_equal(u32(first), u32(frames[1]))
    assert np.array_equal(u32(R.accumulated(oracle, [cam] * 2, W, H, SPP, LIMIT, sky, times[2:], frame_num=2, prev=first)), u32(frames[3]))
    # frame 0 does not read what it is given
    assert np.array_equal(u32(R.accumulated(oracle, [cam] * 2, W, H, SPP, LIMIT, sky, times[:2], prev=np.full((H, W, 3), 7.0, F))), u32(frames[1]))
    # separate frames are each a frame 0
    sep = R.separate(oracle, [cam] * 2, W, H, SPP, LIMIT, sky, times[:2])
    assert np.array_equal(u32(sep[0]), u32(frames[0])) and np.array_equal(u32(sep[1]), u32(oracle.render(cam, W, H, SPP, LIMIT, sky, time_ms=-99)))


def test_depth_of_field_is_sharp_in_the_focus_plane_and_nowhere_else(orc):
    """An emissive quad lies in the focus plane, a second one at twice the distance; antialias off, one bounce, eight lens cameras.  Every
    lens sample's ray of a pixel passes through one point of the focus plane, so a pixel whose point lies inside the near quad sees exactly
    its light in all eight views - no tolerance - while the far quad moves across the pixels from view to view."""
    w, h, dist, focal = 64, 48, 2.0, 0.1
    near, far = (2.0, 1.0, 0.5), (0.5, 2.0, 1.0)              # colour * strength, exact in binary32
    objs = [("quad", (-0.4, 0.3, dist), (0.4, 0.3, dist), (0.4, -0.3, dist), (-0.4, -0.3, dist), ("emissive", (1.0, 0.5, 0.25), 2.0)),
            ("quad", (1.2, 0.5, 2 * dist), (2.0, 0.5, 2 * dist), (2.0, -0.5, 2 * dist), (1.2, -0.5, 2 * dist), ("emissive", (0.25, 1.0, 0.5), 2.0))]
    oracle = orc.Scene(objs, orc.MATH_DET)
    pinhole = orc.camera_default(w, h)
    assert np.all(pinhole[0:3] == 0) and abs(float(pinhole[5]) - focal) < 1e-7     # at the origin, the image plane at z = focal_len (to an ulp)
    cams = [R.lens(pinhole, focal, dist, u, v) for u, v in R.lens_offsets(0.2, 8)]
    for c in cams:
        assert np.array_equal(u32(c[3:]), u32(cams[0][3:]))                         # one image plane for all lens samples ...
    assert abs(float(cams[0][5]) - dist) < 1e-5                                     # ... at the focus distance
    views = R.separate(oracle, cams, w, h, 1, 1, (0.0, 0.0, 0.0), [7] * 8, antialias=False)
    # the focus-plane point of every pixel (float64 from the cameras' floats), and the pixel's size there
    tl, du, dv = (cams[0][i:i + 3].astype(np.float64) for i in (3, 6, 9))
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    point = tl + px[..., None] * du + py[..., None] * dv
    step = max(np.linalg.norm(du), np.linalg.norm(dv))
    inside = (np.abs(point[..., 0]) <= 0.4 - step) & (np.abs(point[..., 1]) <= 0.3 - step)
    assert inside.sum() > 100
    for v in views:
        assert np.array_equal(u32(v[inside]), u32(np.broadcast_to(np.asarray(near, F), v[inside].shape)))
    cover = [np.all(v == np.asarray(far, F), axis=2) for v in views]
    assert all(c.sum() > 20 for c in cover) and not any((c & inside).any() for c in cover)
    assert any(not np.array_equal(cover[0], c) for c in cover[1:])
    # folded, the near quad keeps its colour (every term of the running mean is the same value) and the far quad's edge is a blend
    dof = R.accumulated(oracle, cams, w, h, 1, 1, (0.0, 0.0, 0.0), [7] * 8, antialias=False)
    assert np.allclose(dof[inside], np.asarray(near, F), rtol=1e-6)
    union, common = np.any(cover, axis=0), np.all(cover, axis=0)
    edge = union & ~common
    assert edge.any() and np.all(dof[edge][:, 1] > 0) and np.all(dof[edge][:, 1] < far[1])


def test_lens_restatement_basics():
    cam = np.array([0.5, -1.0, 2.0, 0.4, -0.9, 2.1, 0.001, 0.0, 0.0, 0.0, -0.001, 0.0], F)
    out = R.lens(cam, 0.1, 0.1, 0.0, 0.0)
    assert np.array_equal(u32(out[6:]), u32(cam[6:])) and np.array_equal(u32(out[:3]), u32(cam[:3]))
    moved = R.lens(cam, 0.1, 3.0, 0.25, -0.5)
    # the eye moves along the camera's own unit axes: +x by 0.25, and delta_v points down, so +y by 0.5
    assert np.allclose(moved[:3] - cam[:3], [0.25, 0.5, 0.0], atol=1e-6)
    assert np.allclose(moved[6:], cam[6:] * F(30.0), rtol=1e-6) and np.array_equal(u32(moved[3:]), u32(R.lens(cam, 0.1, 3.0, 0.0, 0.0)[3:]))
    off = R.lens_offsets(0.05, 16)
    assert off.dtype == F and off.shape == (16, 2) and np.all(np.hypot(off[:, 0], off[:, 1]) <= 0.05 * (1 + 1e-6))
