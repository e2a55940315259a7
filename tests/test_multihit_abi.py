"""The multi-hit entry points without a GPU: the symbols and their ctypes signatures, the null-context refusals, RT_MULTIHIT_MAX in the header
against the binding, and the kernels' register / scratch budget read from the code object inside the shipped library (one kernel per shape
of RT_SHAPES; no spill, no scratch, no AGPRs, and at most 128 VGPRs, so that the four waves per SIMD the kernel is compiled for are resident)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_trace_rays_multi", "rt_trace_rays_multi_device")


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp, i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_trace_rays_multi.argtypes == [vp, vp, fp, fp, fp, C.c_int64, C.c_int32, vp, i32p]
    assert L.rt_trace_rays_multi_device.argtypes == [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp]
    assert L.rt_version() == b"ray-tracer_amd 0.4.1 (gfx950)"
    for name in ("trace_rays_multi", "trace_rays_multi_device", "count_hits"):
        assert callable(getattr(rt, name)), name
    # refused before HIP is touched: no GPU needed (n == 0 included: the context comes first)
    three = (C.c_float * 3)(0, 0, 1)
    rec = np.zeros(2, rt.HIT_DTYPE)
    cnt = (C.c_int32 * 1)(7)
    assert L.rt_trace_rays_multi(None, None, three, three, None, 1, 2, C.c_void_p(rec.ctypes.data), cnt) == rt.RT_ERR_INVALID
    assert L.rt_trace_rays_multi_device(None, None, None, None, None, 1, 2, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_trace_rays_multi(None, None, None, None, None, 0, 0, None, None) == rt.RT_ERR_INVALID
    assert cnt[0] == 7 and not rec.tobytes().strip(b"\0")


def test_multihit_max_in_the_header_and_the_binding(rt):
    text = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert int(re.search(r"#define\s+RT_MULTIHIT_MAX\s+(\d+)", text).group(1)) == rt.MULTIHIT_MAX == 8
    import multihit_ref as R
    assert R.MULTIHIT_MAX == rt.MULTIHIT_MAX and R.HIT_DTYPE == rt.HIT_DTYPE


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_multihit_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    multi = {shape_of(n): v for n, v in notes.items() if "rt_multihit_kernel" in n}
    render = {shape_of(n) for n in notes if "rt_render_kernel" in n}
    assert set(multi) == render and len(multi) == 13
    report = []
    for shape, v in sorted(multi.items()):
        report.append("threads %4d mesh %d mode %d: %d VGPRs" % (shape + (v["vgpr_count"],)))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (shape, v)
        # <= 128 registers: the four waves per SIMD of __launch_bounds__(NT, 4) are resident (512 / 128)
        assert v["agpr_count"] == 0 and v["vgpr_count"] <= 128, (shape, v)
    print("\n".join(report))
