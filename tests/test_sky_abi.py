"""The cube-map sky without a GPU: the symbols and their ctypes signatures against the header, RT_SKY_MAX_FACE against the binding, the
refusals a call meets before it touches HIP, rt_sky_texel_direction against its NumPy float32 restatement (tests/sky_ref.py) as uint32, and
the sky kernels' register / scratch figures read from the code object inside the shipped library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sky_ref as S
from conftest import ROOT
from test_abi import ctypes_kind, declared_prototypes
from test_kernel_budget import LLVM, kernel_notes

F = np.float32
NEW_SYMBOLS = ("rt_sky_create", "rt_sky_destroy", "rt_sky_texel_direction", "rt_render_sky_device", "rt_render_sky")


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
    assert protos["rt_sky_create"] == ("int32", ["pointer", "int32", "pointer", "pointer"])
    assert protos["rt_sky_destroy"] == ("void", ["pointer"])
    assert protos["rt_sky_texel_direction"] == ("int32", ["int32"] * 4 + ["pointer"])
    assert protos["rt_render_sky_device"] == ("int32", ["pointer"] * 5 + ["int32", "pointer", "int32", "int32", "pointer", "pointer"])
    assert protos["rt_render_sky"] == ("int32", ["pointer"] * 5 + ["int32", "pointer", "int32", "pointer", "pointer"])
    # in the header's order: behind the camera sequences
    i = rt.ABI_SYMBOLS.index("rt_sky_create")
    assert rt.ABI_SYMBOLS[i - 1] == "rt_camera_lens" and rt.ABI_SYMBOLS[i:i + 5] == list(NEW_SYMBOLS)
    for name in ("Sky", "render_sky", "render_sky_device", "sky_texel_directions", "sky_from_equirect"):
        assert callable(getattr(rt, name)), name
    hdr = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert int(re.search(r"#define RT_SKY_MAX_FACE (\d+)", hdr).group(1)) == rt.SKY_MAX_FACE == 2048
    assert b"0.4.1" in L.rt_version()


def test_refusals_before_hip(rt):
    """no GPU needed: a null context is refused before every other argument, and nothing is written"""
    L = rt.lib()
    cams = (rt.rt_camera * 2)(rt.Camera(8, 8).c, rt.Camera(8, 8).c)
    times = (C.c_int32 * 2)(1, 2)
    rs = rt.RenderData(4, 8, True, (1, 1, 1))
    frames = np.full((2, 8, 8, 3), 7.0, F)
    fn = C.c_int32(3)
    fp = frames.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rt_render_sky_device(None, None, None, cams, times, 2, C.byref(rs.c), 0, 0, fp, None) == rt.RT_ERR_INVALID
    assert L.rt_render_sky_device(None, None, None, None, None, 0, None, 0, 0, None, None) == rt.RT_ERR_INVALID
    assert L.rt_render_sky(None, None, None, cams, times, 2, C.byref(rs.c), 1, C.byref(fn), fp) == rt.RT_ERR_INVALID
    assert L.rt_render_sky(None, None, None, None, None, 2, None, 0, None, None) == rt.RT_ERR_INVALID
    out = C.c_void_p()
    faces = np.ones((6, 1, 1, 3), F)
    assert L.rt_sky_create(None, 1, faces.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)) == rt.RT_ERR_INVALID and not out.value
    L.rt_sky_destroy(None)
    assert np.all(frames == 7.0) and fn.value == 3
    with pytest.raises(ValueError, match="one time_ms per camera"):
        rt.render_sky(None, None, None, [rt.Camera(8, 8)], rs, [1, 2])
    with pytest.raises(ValueError, match="no cameras"):
        rt.render_sky(None, None, None, [], rs, [])


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 64, 1000, 2048])
def test_texel_direction_equals_its_restatement(rt, n):
    """every texel of a small map, the border and a seeded thousand of a large one: the three floats as uint32; the binding's NumPy form too"""
    L = rt.lib()
    want = S.texel_directions(n)
    rng = np.random.default_rng(n)
    if n <= 16:
        texels = [(f, r, c) for f in range(6) for r in range(n) for c in range(n)]
    else:
        texels = [(f, r, c) for f in range(6) for r in (0, n - 1) for c in (0, n // 2, n - 1)] + [tuple(int(v) for v in rng.integers((0, 0, 0), (6, n, n))) for _ in range(1000)]
    out = np.zeros(3, F)
    for f, r, c in texels:
        assert L.rt_sky_texel_direction(n, f, r, c, out.ctypes.data_as(C.POINTER(C.c_float))) == rt.RT_OK
        assert np.array_equal(u32(out), u32(want[f, r, c])), (n, f, r, c, out, want[f, r, c])
    assert np.array_equal(u32(rt.sky_texel_directions(n)), u32(want))


def test_texel_direction_refusals(rt):
    L = rt.lib()
    out = np.full(3, 7.0, F)
    p = out.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((0, 0, 0, 0, p), (-1, 0, 0, 0, p), (rt.SKY_MAX_FACE + 1, 0, 0, 0, p), (4, -1, 0, 0, p), (4, 6, 0, 0, p), (4, 0, -1, 0, p), (4, 0, 4, 0, p), (4, 0, 0, -1, p),
                 (4, 0, 0, 4, p), (4, 0, 0, 0, None)):
        assert L.rt_sky_texel_direction(*args) == rt.RT_ERR_INVALID, args[:4]
    assert np.all(out == 7.0)
    assert L.rt_sky_texel_direction(rt.SKY_MAX_FACE, 5, rt.SKY_MAX_FACE - 1, 0, p) == rt.RT_OK and out[2] == -1.0


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_sky_kernel_register_budget(rt, tmp_path):
    """one sky kernel per shape of RT_SHAPES, without a spilled register or a byte of scratch, inside its shape's launch bounds and at the
    views kernel's waves per SIMD (a SIMD's 512 registers per lane in blocks of 8)"""
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    sky = {shape_of(n): v for n, v in notes.items() if "rt_sky_kernel" in n}
    views = {shape_of(n): v for n, v in notes.items() if "rt_views_kernel" in n}
    assert set(sky) == set(views) and len(sky) == 13 and sum("rt_sky_kernel" in n for n in notes) == 13
    waves = lambda v: min(8, 512 // (-(-v["vgpr_count"] // 8) * 8))
    report = []
    for (nt, mesh, mode), v in sorted(sky.items()):
        report.append("threads %4d mesh %d mode %d: %s  (views: %d VGPRs)" % (nt, mesh, mode, v, views[(nt, mesh, mode)]["vgpr_count"]))
        assert v["agpr_count"] == 0 and v["vgpr_spill_count"] == 0 and v["scratch_insts"] == 0 and v["private_segment_fixed_size"] == 0, ((nt, mesh, mode), v)
        assert v["vgpr_count"] <= (128 if nt == 1024 else 96), ((nt, mesh, mode), v)
        assert waves(v) >= waves(views[(nt, mesh, mode)]), ((nt, mesh, mode), v, views[(nt, mesh, mode)])
    print("\n".join(report))
