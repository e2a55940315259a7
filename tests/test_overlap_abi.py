"""The box-overlap entry points without a GPU: the symbols and their ctypes signatures against the header's prototypes, the null-context
refusals, rt_overlap_id's size and offsets in the header's order against the binding's and the yardstick's dtypes, RT_OVERLAP_MAX, and the
kernels' register / scratch budget read from the code object inside the shipped library (one kernel per shape of RT_SHAPES; no spill, no
scratch, no AGPRs, and at most 128 VGPRs, so that the four waves per SIMD the kernel is compiled for are resident)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_overlap_boxes", "rt_overlap_boxes_device")
HEADER = open(os.path.join(ROOT, "include", "rt_amd.h")).read()


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp, i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_overlap_boxes.argtypes == [vp, vp, fp, fp, C.c_int64, C.c_int32, vp, i32p, vp]
    assert L.rt_overlap_boxes_device.argtypes == [vp, vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp, vp]
    assert L.rt_overlap_boxes.restype == L.rt_overlap_boxes_device.restype == C.c_int
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("overlap_boxes", "overlap_boxes_device", "boxes_touch", "voxelize", "voxel_boxes"):
        assert callable(getattr(rt, name)), name
    # the header's prototypes: the parameter kinds in order
    for name, kinds in (("rt_overlap_boxes_device", "rt_ctx*,const rt_scene*,const float*,const float*,int64_t,int32_t,rt_overlap_id*,int32_t*,uint8_t*,void*"),
                        ("rt_overlap_boxes", "rt_ctx*,const rt_scene*,const float*,const float*,int64_t,int32_t,rt_overlap_id*,int32_t*,uint8_t*")):
        m = re.search(r"rt_status\s+%s\s*\(([^)]*)\)\s*;" % name, HEADER)
        assert m, name
        params = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", p.strip()).replace(" *", "*")) for p in m.group(1).split(",")]
        assert ",".join(params) == kinds, (name, params)
    # refused before HIP is touched: no GPU needed (n == 0 included: the context comes first)
    three = (C.c_float * 3)(0, 0, 1)
    ids = np.zeros(2, rt.OverlapId)
    counts = np.zeros(1, np.int32)
    assert L.rt_overlap_boxes(None, None, three, three, 1, 2, C.c_void_p(ids.ctypes.data), counts.ctypes.data_as(i32p), None) == rt.RT_ERR_INVALID
    assert L.rt_overlap_boxes_device(None, None, None, None, 1, 0, None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_overlap_boxes(None, None, None, None, 0, 0, None, None, None) == rt.RT_ERR_INVALID
    assert not ids.tobytes().strip(b"\0") and counts[0] == 0


def test_the_id_in_the_header_the_binding_and_the_yardstick(rt):
    import overlap_ref as R
    m = re.search(r"typedef struct rt_overlap_id \{(.*?)\} rt_overlap_id;", HEADER, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t)\s+(\w+)\s*;", body)
    assert fields == [("int32_t", "object"), ("int32_t", "triangle")]
    for dtype in (rt.OVERLAP_ID_DTYPE, rt.OverlapId, R.ID_DTYPE):
        assert dtype.itemsize == 8 and dtype.names == ("object", "triangle")
        assert [dtype.fields[n][1] for n in dtype.names] == [0, 4] and all(dtype.fields[n][0] == np.int32 for n in dtype.names)
    assert rt.OVERLAP_ID_DTYPE == R.ID_DTYPE
    assert rt.OVERLAP_MAX == R.OVERLAP_MAX == int(re.search(r"#define\s+RT_OVERLAP_MAX\s+(\d+)", HEADER).group(1)) == 8
    # the yardstick's empty slot is {-1, -1}, and an invalid box overlaps nothing
    flat = rt.SceneObjects(rt.scenes.CONFIG_SCENES["three_sphere"]()[0]).debug_flatten()
    counts, flags, ids = R.overlap(flat, [[50, 50, 50], [np.nan, 0, 0]], [[51, 51, 51], [1, 1, 1]], 2)
    assert counts.tolist() == [0, 0] and flags.tolist() == [0, 0] and ids["object"].tolist() == [[-1, -1]] * 2 and ids["triangle"].tolist() == [[-1, -1]] * 2


def test_voxel_boxes(rt):
    lo, hi, centre = rt.voxel_boxes((-1.0, 0.0, 0.3), (2.0, 0.7, 0.3000001), (3, 5, 1))
    assert lo.shape == hi.shape == centre.shape == (15, 3) and lo.dtype == hi.dtype == centre.dtype == np.float32
    assert (lo <= hi).all() and np.array_equal(lo[0], np.float32([-1.0, 0.0, 0.3])) and np.array_equal(hi[-1], np.float32([2.0, 0.7, 0.3000001]))
    g_lo, g_hi = lo.reshape(3, 5, 1, 3), hi.reshape(3, 5, 1, 3)
    assert np.array_equal(g_lo[1:, :, :, 0], g_hi[:-1, :, :, 0]) and np.array_equal(g_lo[:, 1:, :, 1], g_hi[:, :-1, :, 1]), "neighbours share a face exactly"
    with pytest.raises(ValueError):
        rt.voxel_boxes((0, 0, 0), (1, 1, 1), (4, 0, 4))


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_overlap_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    overlap = {shape_of(n): v for n, v in notes.items() if "rt_overlap_kernel" in n}
    multihit = {shape_of(n): v for n, v in notes.items() if "rt_multihit_kernel" in n}
    render = {shape_of(n) for n in notes if "rt_render_kernel" in n}
    assert set(overlap) == set(multihit) == render and len(overlap) == 13
    report = []
    for shape, v in sorted(overlap.items()):
        report.append("threads %4d mesh %d mode %d: %d VGPRs" % (shape + (v["vgpr_count"],)))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (shape, v)
        # <= 128 registers: the four waves per SIMD of __launch_bounds__(NT, 4) are resident (512 / 128)
        assert v["agpr_count"] == 0 and v["vgpr_count"] <= 128, (shape, v)
    print("\n".join(report))
