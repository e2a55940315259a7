"""The nearest-surface entry points without a GPU: the symbols and their ctypes signatures, the record's size, alignment and offsets in the
header against the NumPy mirror, the miss pattern, the null-context refusals, and the kernels' register / scratch budget read from the code
object inside the shipped library (one kernel per shape of RT_SHAPES, no spill, no scratch, and no more registers than lets the query
kernel's four waves per SIMD be resident)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_nearest_points", "rt_nearest_points_device")


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_nearest_points.argtypes == [vp, vp, fp, fp, C.c_int64, vp]
    assert L.rt_nearest_points_device.argtypes == [vp, vp, vp, vp, C.c_int64, vp, vp]
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("nearest_points", "nearest_points_device", "distance_grid"):
        assert callable(getattr(rt, name)), name
    assert rt.NearestRecord is rt.NEAREST_DTYPE
    # refused before HIP is touched: no GPU needed (n == 0 included: the context comes first)
    three = (C.c_float * 3)(0, 0, 0)
    rec = np.zeros(1, rt.NearestRecord)
    assert L.rt_nearest_points(None, None, three, None, 1, C.c_void_p(rec.ctypes.data)) == rt.RT_ERR_INVALID
    assert L.rt_nearest_points_device(None, None, None, None, 1, None, None) == rt.RT_ERR_INVALID
    assert L.rt_nearest_points(None, None, None, None, 0, None) == rt.RT_ERR_INVALID


def test_record_size_offsets_and_miss_pattern(rt, tmp_path):
    src = tmp_path / "nearest.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %.1f\\n", sizeof(rt_nearest), _Alignof(rt_nearest), offsetof(rt_nearest, distance), '
                   'offsetof(rt_nearest, distance2), offsetof(rt_nearest, point), offsetof(rt_nearest, object), offsetof(rt_nearest, triangle), '
                   'offsetof(rt_nearest, reserved), (double)RT_HIT_MISS_T); return 0; }\n')
    exe = tmp_path / "nearest"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    dt = rt.NearestRecord
    assert int(out[0]) == dt.itemsize == 32 and int(out[1]) == 16
    assert [int(x) for x in out[2:8]] == [dt.fields[n][1] for n in ("distance", "distance2", "point", "object", "triangle", "reserved")] == [0, 4, 8, 20, 24, 28]
    assert dt.names == ("distance", "distance2", "point", "object", "triangle", "reserved")
    assert float(out[8]) == float(rt.HIT_MISS_T) == 2.0 ** 30
    # the miss pattern, as the yardstick writes it
    import nearest_ref as R
    assert R.DTYPE == dt
    miss = R.nearest({"blob": np.zeros((0, 4), np.float32), "off_nodes": 0, "off_tris": 0, "off_meshes": 0, "num_meshes": 0, "num_nodes": 0,
                      "num_triangles": 0, "objects": np.zeros(0, [("type", "<i4"), ("prim_start", "<i4"), ("v", "<f4", (8,))])}, np.zeros((1, 3), np.float32))
    assert miss.tobytes() == np.array([2.0 ** 30, 2.0 ** 30, 0, 0, 0], np.float32).tobytes() + np.array([-1, -1, 0], np.int32).tobytes()


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_nearest_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    nearest = {shape_of(n): v for n, v in notes.items() if "rt_nearest_kernel" in n}
    render = {shape_of(n) for n in notes if "rt_render_kernel" in n}
    assert set(nearest) == render and len(nearest) == 13
    report = []
    for shape, v in sorted(nearest.items()):
        report.append("threads %4d mesh %d mode %d: %d VGPRs" % (shape + (v["vgpr_count"],)))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (shape, v)
        # <= 64 registers: eight waves per SIMD could be resident (512 / 64); the kernels are compiled for the query kernel's four
        assert v["agpr_count"] == 0 and v["vgpr_count"] <= 64, (shape, v)
    print("\n".join(report))
