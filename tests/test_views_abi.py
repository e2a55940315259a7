"""The camera-sequence entry points without a GPU: the symbols and their ctypes signatures against the header, RT_VIEWS_MAX against the
binding, the refusals a call meets before it touches HIP, rt_camera_lens against its NumPy float32 restatement (tests/views_ref.py) as
uint32, lens_cameras, and the views kernels' register / scratch figures read from the code object inside the shipped library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import views_ref as R
from conftest import ROOT
from test_abi import ctypes_kind, declared_prototypes
from test_kernel_budget import LLVM, kernel_notes

F = np.float32
NEW_SYMBOLS = ("rt_render_views_device", "rt_render_views", "rt_camera_lens")


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_symbols_and_signatures_agree_with_the_header(rt):
    L = rt.lib()
    protos = {p[0]: p[1:] for p in declared_prototypes()}
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)
        assert name in rt.ABI_SYMBOLS and name in protos, name
        ret, params = protos[name]
        assert ctypes_kind(fn.restype) == ret and [ctypes_kind(a) for a in fn.argtypes] == params, name
    # read by eye from include/rt_amd.h
    assert protos["rt_render_views_device"] == ("int32", ["pointer"] * 4 + ["int32", "pointer", "int32", "int32", "pointer", "pointer"])
    assert protos["rt_render_views"] == ("int32", ["pointer"] * 4 + ["int32", "pointer", "int32", "pointer", "pointer"])
    assert protos["rt_camera_lens"] == ("int32", ["pointer"] + ["float"] * 4 + ["pointer"])
    # in the header's order: behind the frames in flight
    i = rt.ABI_SYMBOLS.index("rt_render_views_device")
    assert rt.ABI_SYMBOLS[i - 1] == "rt_frame_wait" and rt.ABI_SYMBOLS[i:i + 3] == list(NEW_SYMBOLS)
    for name in ("render_views", "render_views_device", "lens_cameras"):
        assert callable(getattr(rt, name)), name
    assert callable(rt.Camera.lens)
    hdr = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert int(re.search(r"#define RT_VIEWS_MAX (\d+)", hdr).group(1)) == rt.VIEWS_MAX == 32
    dev = open(os.path.join(ROOT, "ray-tracer_amd", "csrc", "rt_device_scene.h")).read()
    assert 1 << int(re.search(r"#define RT_FRAME_BITS (\d+)", dev).group(1)) == rt.VIEWS_MAX        # = RT_MAX_BATCH_FRAMES


def test_refusals_before_hip(rt):
    """no GPU needed: a null context is refused before every other argument, and nothing is written"""
    L = rt.lib()
    cams = (rt.rt_camera * 2)(rt.Camera(8, 8).c, rt.Camera(8, 8).c)
    times = (C.c_int32 * 2)(1, 2)
    rs = rt.RenderData(4, 8, True, (1, 1, 1))
    frames = np.full((2, 8, 8, 3), 7.0, F)
    fn = C.c_int32(3)
    fp = frames.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rt_render_views_device(None, None, cams, times, 2, C.byref(rs.c), 0, 0, fp, None) == rt.RT_ERR_INVALID
    assert L.rt_render_views_device(None, None, None, None, 0, None, 0, 0, None, None) == rt.RT_ERR_INVALID
    assert L.rt_render_views(None, None, cams, times, 2, C.byref(rs.c), 1, C.byref(fn), fp) == rt.RT_ERR_INVALID
    assert L.rt_render_views(None, None, None, None, 2, None, 0, None, None) == rt.RT_ERR_INVALID
    assert np.all(frames == 7.0) and fn.value == 3
    with pytest.raises(ValueError, match="one time_ms per camera"):
        rt.render_views(None, None, [rt.Camera(8, 8)], rs, [1, 2])
    with pytest.raises(ValueError, match="no cameras"):
        rt.render_views(None, None, [], rs, [])


def random_cameras(rt, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        pos = tuple(float(x) for x in rng.uniform(-3, 3, 3))
        rot = tuple(float(x) for x in rng.uniform(-3.1, 3.1, 3))
        focal = float(rng.choice([0.1, 0.05, 0.37, 1.0, 2.5]))
        w, h = int(rng.integers(1, 400)), int(rng.integers(1, 300))
        cam = rt.Camera(w, h, pos=pos, fov=float(rng.uniform(0.3, 2.0)), focal_len=focal, rot=rot)
        out.append((cam, focal, float(rng.uniform(0.05, 50.0)), float(rng.normal(0, 0.2)), float(rng.normal(0, 0.2))))
    return out


def test_camera_lens_equals_its_restatement(rt):
    """1,000 seeded cameras, offsets and distances: every float of the result as uint32; the image plane does not depend on the offset"""
    for cam, focal, dist, lu, lv in random_cameras(rt, 1000, 77):
        got = cam.lens(focal, dist, lu, lv)
        want = R.lens(cam.floats(), focal, dist, lu, lv)
        assert np.array_equal(u32(got.floats()), u32(want)), (cam.floats(), focal, dist, lu, lv, got.floats(), want)
        assert (got.width, got.height) == (cam.width, cam.height)
        centre = cam.lens(focal, dist, 0.0, 0.0)
        assert np.array_equal(u32(got.floats()[3:]), u32(centre.floats()[3:]))            # tl, delta_u, delta_v: bit-equal across offsets
        assert np.array_equal(u32(centre.floats()[:3] + F(0.0)), u32(cam.floats()[:3] + F(0.0)))   # no offset: the eye stays (a -0 component comes out +0)
    # focus_dist == focal_len: s == 1, the image plane stays where it is to the rounding of (tl - pos) + pos
    cam = rt.Camera(64, 48)
    same = cam.lens(0.1, 0.1, 0.0, 0.0)
    assert np.array_equal(u32(same.floats()[6:]), u32(cam.floats()[6:]))
    # out may be cam
    L = rt.lib()
    c2 = rt.Camera(64, 48)
    assert L.rt_camera_lens(C.byref(c2.c), F(0.1), F(3.0), F(0.01), F(-0.02), C.byref(c2.c)) == rt.RT_OK
    assert np.array_equal(u32(c2.floats()), u32(cam.lens(0.1, 3.0, 0.01, -0.02).floats()))


def test_camera_lens_refusals(rt):
    L = rt.lib()
    cam = rt.Camera(16, 16)
    out = rt.Camera(16, 16, floats=np.full(12, 7.0, F))
    inf, nan = float("inf"), float("nan")

    def call(c, focal, dist, lu, lv, o):
        return L.rt_camera_lens(c, F(focal), F(dist), F(lu), F(lv), o)
    good = (C.byref(cam.c), 0.1, 2.0, 0.01, 0.01, C.byref(out.c))
    bad = [(0, None), (5, None)] + [(1, v) for v in (0.0, -0.1, inf, nan)] + [(2, v) for v in (0.0, -1.0, inf, nan)] + [(3, v) for v in (inf, -inf, nan)] + \
          [(4, v) for v in (inf, nan)]
    for i, v in bad:
        assert call(*(good[:i] + (v,) + good[i + 1:])) == rt.RT_ERR_INVALID, (i, v)
    for field in ("delta_u", "delta_v"):
        flat = rt.Camera(16, 16)
        getattr(flat.c, field)[:] = [0.0, 0.0, 0.0]
        assert call(C.byref(flat.c), 0.1, 2.0, 0.0, 0.0, C.byref(out.c)) == rt.RT_ERR_INVALID, field
    assert np.all(out.floats() == 7.0)
    assert call(*good) == rt.RT_OK and not np.all(out.floats() == 7.0)
    with pytest.raises(ValueError):
        cam.lens(0.0, 1.0, 0.0, 0.0)


def test_lens_cameras_are_deterministic_and_inside_the_disc(rt):
    cam = rt.Camera(37, 21)
    aperture, n = 0.05, 64
    a = rt.lens_cameras(cam, 0.1, 2.0, aperture, n)
    b = rt.lens_cameras(cam, 0.1, 2.0, aperture, n)
    assert len(a) == n and all(np.array_equal(u32(x.floats()), u32(y.floats())) for x, y in zip(a, b))
    off = R.lens_offsets(aperture, n)
    r = np.hypot(off[:, 0].astype(np.float64), off[:, 1].astype(np.float64))
    assert np.all(r <= aperture * (1 + 1e-6)) and np.all(np.diff(r) > 0) and r[0] > 0           # the spiral: radii grow, all inside the disc
    assert len({x.floats()[:3].tobytes() for x in a}) == n
    for x, (u, v) in zip(a, off):
        assert np.array_equal(u32(x.floats()), u32(R.lens(cam.floats(), 0.1, 2.0, u, v)))
    # the eye's distance from the pinhole is the offset's length (the camera's axes are unit vectors to rounding)
    d = np.array([np.linalg.norm((x.floats()[:3] - cam.floats()[:3]).astype(np.float64)) for x in a])
    assert np.allclose(d, r, rtol=1e-4, atol=1e-7)
    assert rt.lens_cameras(cam, 0.1, 2.0, 0.0, 3)[0].floats()[:3].tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        rt.lens_cameras(cam, 0.1, 2.0, 0.05, 0)
    with pytest.raises(ValueError):
        rt.lens_cameras(cam, 0.1, 2.0, -1.0, 4)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_views_kernel_register_budget(rt, tmp_path):
    """one views kernel per shape of RT_SHAPES, without a spilled register or a byte of scratch, inside its shape's launch bounds and at the
    render kernel's waves per SIMD (a SIMD's 512 registers per lane in blocks of 8)"""
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    views = {shape_of(n): v for n, v in notes.items() if "rt_views_kernel" in n}
    render = {shape_of(n): v for n, v in notes.items() if "rt_render_kernel" in n}
    assert set(views) == set(render) and len(views) == 13 and sum("rt_views_kernel" in n for n in notes) == 13
    waves = lambda v: min(8, 512 // (-(-v["vgpr_count"] // 8) * 8))
    report = []
    for (nt, mesh, mode), v in sorted(views.items()):
        report.append("threads %4d mesh %d mode %d: %s" % (nt, mesh, mode, v))
        assert v["agpr_count"] == 0 and v["vgpr_spill_count"] == 0 and v["scratch_insts"] == 0 and v["private_segment_fixed_size"] == 0, ((nt, mesh, mode), v)
        assert v["vgpr_count"] <= (128 if nt == 1024 else 96), ((nt, mesh, mode), v)
        # (a 1024-thread workgroup is one per CU, four waves per SIMD, whatever it is allocated within its bounds)
        assert nt == 1024 or waves(v) >= waves(render[(nt, mesh, mode)]), ((nt, mesh, mode), v, render[(nt, mesh, mode)])
        assert v["sgpr_spill_count"] <= (80 if mode == 1 else 96), ((nt, mesh, mode), v)
    print("\n".join(report))
