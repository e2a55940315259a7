"""The ambient-occlusion entry points without a GPU: the symbols and their ctypes signatures, the null-context refusals, the header's
RT_AO_* against the binding, and the AO kernels' register / scratch budget read from the code object inside the shipped library."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_render_ao", "rt_render_ao_device")


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_render_ao.argtypes == [vp, vp, C.POINTER(rt.rt_camera), C.c_int32, C.c_float, C.c_float, C.c_int32, vp, fp]
    assert L.rt_render_ao_device.argtypes == [vp, vp, C.POINTER(rt.rt_camera), C.c_int32, C.c_float, C.c_float, C.c_int32, vp, vp, vp]
    assert L.rt_render_ao.restype is C.c_int32 and L.rt_render_ao_device.restype is C.c_int32
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("render_ao", "render_ao_device"):
        assert callable(getattr(rt, name)), name
    # in the header's order: behind the visibility plane, ahead of the denoiser
    i = rt.ABI_SYMBOLS.index("rt_render_ao_device")
    assert rt.ABI_SYMBOLS[i - 1:i + 3] == ["rt_render_visibility", "rt_render_ao_device", "rt_render_ao", "rt_denoise_params_default"]


def test_null_context_is_refused_before_hip(rt):
    """no GPU needed: the entry points check their context before they touch HIP, and before every other argument"""
    L = rt.lib()
    cam = rt.Camera(8, 8)
    count = (C.c_uint16 * 64)()
    ao = (C.c_float * 64)()
    assert L.rt_render_ao(None, None, C.byref(cam.c), 16, 0.5, 1e-3, 0, count, ao) == rt.RT_ERR_INVALID
    assert L.rt_render_ao_device(None, None, C.byref(cam.c), 16, 0.5, 1e-3, 0, None, None, None) == rt.RT_ERR_INVALID
    # ... with everything else invalid too: the context comes first
    assert L.rt_render_ao(None, None, None, 0, -1.0, -1.0, 0, None, None) == rt.RT_ERR_INVALID
    assert L.rt_render_ao_device(None, None, None, 5000, float("nan"), float("inf"), -1, None, None, None) == rt.RT_ERR_INVALID
    assert not any(count) and not any(ao)
    with pytest.raises(ValueError, match="unknown planes"):
        rt.render_ao(None, None, cam, planes=("ao", "depth"))


def test_ao_constants_in_header_and_binding(rt):
    hdr = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert int(re.search(r"#define RT_AO_NO_SURFACE (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == rt.AO_NO_SURFACE == 0xFFFF
    assert int(re.search(r"#define RT_AO_MAX_SAMPLES (\d+)", hdr).group(1)) == rt.AO_MAX_SAMPLES == 4096
    assert rt.AO_MAX_SAMPLES < rt.AO_NO_SURFACE                       # a count never collides with the marker


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_ao_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    ao = {}
    for n, v in notes.items():
        if "rt_ao_kernel" in n:
            # the other kernels are counted by their names: this one's must hold none of them
            assert not any(w in n for w in ("rt_render_kernel", "rt_query_kernel", "rt_occlusion_kernel", "rt_denoise")), n
            ao[tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())] = v
    render = {tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups()) for n in notes if "rt_render_kernel" in n}
    # one kernel per shape, one front: 13
    assert set(ao) == render and len(ao) == 13 and sum("rt_ao_kernel" in n for n in notes) == 13
    report = []
    for shape, v in sorted(ao.items()):
        report.append("threads %4d mesh %d mode %d: %d VGPRs" % (shape + (v["vgpr_count"],)))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (shape, v)
        assert v["agpr_count"] == 0, (shape, v)
        assert v["vgpr_count"] <= 128, (shape, v)                     # __launch_bounds__(NT, 4): four waves per SIMD
    print("\n".join(report))
