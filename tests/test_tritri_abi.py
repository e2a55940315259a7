"""The triangle-overlap entry points without a GPU: the symbols and their ctypes signatures against the header's prototypes, the
null-context refusals, rt_tri_segment's size and offsets in the header's order against the binding's and the yardstick's dtypes, and the
kernels' register / scratch budget read from the code object inside the shipped library (one kernel per shape of RT_SHAPES; no spill, no
scratch, no AGPRs, and at most 128 VGPRs, so that the four waves per SIMD the kernel is compiled for are resident)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_overlap_triangles", "rt_overlap_triangles_device")
HEADER = open(os.path.join(ROOT, "include", "rt_amd.h")).read()


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp, i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_overlap_triangles.argtypes == [vp, vp, fp, C.c_int64, C.c_int32, vp, i32p, vp, vp]
    assert L.rt_overlap_triangles_device.argtypes == [vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp, vp, vp]
    assert L.rt_overlap_triangles.restype == L.rt_overlap_triangles_device.restype == C.c_int
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("overlap_triangles", "overlap_triangles_device", "triangles_touch", "collide_mesh"):
        assert callable(getattr(rt, name)), name
    # the header's prototypes: the parameter kinds in order
    for name, kinds in (("rt_overlap_triangles_device", "rt_ctx*,const rt_scene*,const float*,int64_t,int32_t,rt_overlap_id*,int32_t*,uint8_t*,rt_tri_segment*,void*"),
                        ("rt_overlap_triangles", "rt_ctx*,const rt_scene*,const float*,int64_t,int32_t,rt_overlap_id*,int32_t*,uint8_t*,rt_tri_segment*")):
        m = re.search(r"rt_status\s+%s\s*\(([^)]*)\)\s*;" % name, HEADER)
        assert m, name
        params = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", p.strip()).replace(" *", "*")) for p in m.group(1).split(",")]
        assert ",".join(params) == kinds, (name, params)
    # refused before HIP is touched: no GPU needed (n == 0 included: the context comes first)
    nine = (C.c_float * 9)(0, 0, 0, 1, 0, 0, 0, 1, 0)
    ids = np.zeros(2, rt.OverlapId)
    segs = np.zeros(2, rt.TriSegment)
    counts = np.zeros(1, np.int32)
    assert L.rt_overlap_triangles(None, None, nine, 1, 2, C.c_void_p(ids.ctypes.data), counts.ctypes.data_as(i32p), None, C.c_void_p(segs.ctypes.data)) == rt.RT_ERR_INVALID
    assert L.rt_overlap_triangles_device(None, None, None, 1, 0, None, None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_overlap_triangles(None, None, None, 0, 0, None, None, None, None) == rt.RT_ERR_INVALID
    assert not ids.tobytes().strip(b"\0") and not segs.tobytes().strip(b"\0") and counts[0] == 0


def test_the_segment_in_the_header_the_binding_and_the_yardstick(rt):
    import tritri_ref as R
    m = re.search(r"typedef struct rt_tri_segment \{(.*?)\} rt_tri_segment;", HEADER, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(float|int32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert fields == [("float", "p", "3"), ("float", "q", "3"), ("int32_t", "kind", ""), ("int32_t", "reserved", "")]
    for dtype in (rt.TRI_SEGMENT_DTYPE, rt.TriSegment, R.SEG_DTYPE):
        assert dtype.itemsize == 32 and dtype.names == ("p", "q", "kind", "reserved")
        assert [dtype.fields[n][1] for n in dtype.names] == [0, 12, 24, 28]
        assert dtype.fields["p"][0] == dtype.fields["q"][0] == np.dtype((np.float32, (3,))) and dtype.fields["kind"][0] == dtype.fields["reserved"][0] == np.int32
    assert rt.TRI_SEGMENT_DTYPE == R.SEG_DTYPE and rt.OVERLAP_ID_DTYPE == R.ID_DTYPE
    # the yardstick's empty slot is {-1, -1} with kind 0, a sphere's pair has kind 2 and NaNs, and a query that is not finite overlaps nothing
    flat = rt.SceneObjects(rt.scenes.CONFIG_SCENES["three_sphere"]()[0]).debug_flatten()
    c = np.asarray(flat["objects"][0]["v"][0:3], np.float32)
    r = np.float32(flat["objects"][0]["v"][3])
    through = np.concatenate([c, c + np.float32([2, 0, 0]) * r, c + np.float32([0, 2, 0]) * r])       # from the first sphere's centre to outside it
    far = through + np.float32(1000)
    bad = through.copy()
    bad[4] = np.nan
    counts, flags, ids, segs = R.overlap(flat, np.stack([through, far, bad]), 2, segments=True)
    assert counts[0] >= 1 and counts[1:].tolist() == [0, 0] and flags.tolist() == [1, 0, 0]
    assert ids["object"][0, 0] == 0 and ids["triangle"][0, 0] == -1 and segs["kind"][0, 0] == 2 and np.isnan(segs["p"][0, 0]).all() and np.isnan(segs["q"][0, 0]).all()
    assert segs["p"][0, 0].view(np.uint32).tolist() == [0x7fc00000] * 3
    assert ids["object"][1:].tolist() == [[-1, -1]] * 2 and ids["triangle"][1:].tolist() == [[-1, -1]] * 2 and not segs[1:].tobytes().strip(b"\0")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_tritri_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    tritri = {shape_of(n): v for n, v in notes.items() if "rt_tritri_kernel" in n}
    overlap = {shape_of(n): v for n, v in notes.items() if "rt_overlap_kernel" in n}
    render = {shape_of(n) for n in notes if "rt_render_kernel" in n}
    assert set(tritri) == set(overlap) == render and len(tritri) == 13
    report = []
    for shape, v in sorted(tritri.items()):
        report.append("threads %4d mesh %d mode %d: %d VGPRs" % (shape + (v["vgpr_count"],)))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (shape, v)
        # <= 128 registers: the four waves per SIMD of __launch_bounds__(NT, 4) are resident (512 / 128)
        assert v["agpr_count"] == 0 and v["vgpr_count"] <= 128, (shape, v)
    print("\n".join(report))
