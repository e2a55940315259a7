"""The sphere-cast entry points without a GPU: the symbols and their ctypes signatures against the header's prototypes, the null-context
refusals, rt_sweep's size and offsets in the header's order against the binding's and the yardstick's dtypes, the miss pattern, and the
kernels' register / scratch budget read from the code object inside the shipped library (one kernel per shape of RT_SHAPES; no spill, no
scratch, no AGPRs, and at most 128 VGPRs, so that the four waves per SIMD the kernel is compiled for - the nearest kernel's - are resident)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_sweep_spheres", "rt_sweep_spheres_device")
HEADER = open(os.path.join(ROOT, "include", "rt_amd.h")).read()


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_sweep_spheres.argtypes == [vp, vp, fp, fp, fp, fp, C.c_int64, vp]
    assert L.rt_sweep_spheres_device.argtypes == [vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp]
    assert L.rt_sweep_spheres.restype == L.rt_sweep_spheres_device.restype == C.c_int
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("sweep_spheres", "sweep_spheres_device", "sweep_grid"):
        assert callable(getattr(rt, name)), name
    # the header's prototypes: the parameter kinds in order
    for name, kinds in (("rt_sweep_spheres_device", "rt_ctx*,const rt_scene*,const float*,const float*,const float*,const float*,int64_t,rt_sweep*,void*"),
                        ("rt_sweep_spheres", "rt_ctx*,const rt_scene*,const float*,const float*,const float*,const float*,int64_t,rt_sweep*")):
        m = re.search(r"rt_status\s+%s\s*\(([^)]*)\)\s*;" % name, HEADER)
        assert m, name
        params = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", p.strip()).replace(" *", "*")) for p in m.group(1).split(",")]
        assert ",".join(params) == kinds, (name, params)
    # refused before HIP is touched: no GPU needed (n == 0 included: the context comes first)
    three = (C.c_float * 3)(0, 0, 1)
    one = (C.c_float * 1)(0.5)
    rec = np.zeros(2, rt.SweepRecord)
    assert L.rt_sweep_spheres(None, None, three, three, one, None, 1, C.c_void_p(rec.ctypes.data)) == rt.RT_ERR_INVALID
    assert L.rt_sweep_spheres_device(None, None, None, None, None, None, 1, None, None) == rt.RT_ERR_INVALID
    assert L.rt_sweep_spheres(None, None, None, None, None, None, 0, None) == rt.RT_ERR_INVALID
    assert not rec.tobytes().strip(b"\0")


def test_the_record_in_the_header_the_binding_and_the_yardstick(rt):
    import sweep_ref as R
    m = re.search(r"typedef struct __attribute__\(\(aligned\(16\)\)\) rt_sweep \{(.*?)\} rt_sweep;", HEADER, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(t, n, int(k) if k else 1) for t, n, k in re.findall(r"(float|int32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body)]
    assert fields == [("float", "t", 1), ("float", "centre", 3), ("float", "point", 3), ("int32_t", "object", 1), ("int32_t", "triangle", 1),
                      ("int32_t", "feature", 1), ("int32_t", "overlap", 1), ("int32_t", "reserved", 1)]
    offset = 0
    for dtype in (rt.SWEEP_DTYPE, rt.SweepRecord, R.DTYPE):
        assert dtype.itemsize == 48 and dtype.names == tuple(n for _, n, _ in fields)
        offset = 0
        for t, n, k in fields:
            sub, off = dtype.fields[n][0], dtype.fields[n][1]
            assert off == offset and sub.base == (np.float32 if t == "float" else np.int32) and (sub.shape or (1,)) == (k,), (n, off, sub)
            offset += 4 * k
    assert offset == 48 and rt.SWEEP_DTYPE == R.DTYPE
    assert "48 bytes.  A miss is {RT_HIT_MISS_T, {0,0,0}, {0,0,0}, -1, -1, -1, 0, 0} bit for bit" in HEADER
    assert R.MISS_T == rt.HIT_MISS_T == np.float32(float(re.search(r"#define\s+RT_HIT_MISS_T\s+([\d.]+)f", HEADER).group(1)))
    # the yardstick's miss is that pattern
    flat = rt.SceneObjects(rt.scenes.CONFIG_SCENES["three_sphere"]()[0]).debug_flatten()
    miss = R.sweep(flat, [[0, 50, 0]], [[0, 1, 0]], 0.1)[0]
    assert (miss["t"], list(miss["centre"]), list(miss["point"]), miss["object"], miss["triangle"], miss["feature"], miss["overlap"], miss["reserved"]) == \
        (R.MISS_T, [0, 0, 0], [0, 0, 0], -1, -1, -1, 0, 0)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_sweep_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    sweep = {shape_of(n): v for n, v in notes.items() if "rt_sweep_kernel" in n}
    nearest = {shape_of(n): v for n, v in notes.items() if "rt_nearest_kernel" in n}
    render = {shape_of(n) for n in notes if "rt_render_kernel" in n}
    assert set(sweep) == set(nearest) == render and len(sweep) == 13
    report = []
    for shape, v in sorted(sweep.items()):
        report.append("threads %4d mesh %d mode %d: %d VGPRs" % (shape + (v["vgpr_count"],)))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (shape, v)
        # <= 128 registers: the four waves per SIMD of __launch_bounds__(NT, 4), the nearest kernel's, are resident (512 / 128)
        assert v["agpr_count"] == 0 and v["vgpr_count"] <= 128, (shape, v)
    print("\n".join(report))
