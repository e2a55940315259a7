"""The budget and adaptive entry points without a GPU: the symbols and their ctypes signatures against the header, the struct sizes and
the defaults, the refusals a call meets before it touches HIP, the header's RT_BUDGET_* / RT_ADAPTIVE_* against the binding, and the
budget kernels' register / scratch figures read from the code object inside the shipped library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import adaptive_ref
from conftest import ROOT
from test_abi import ctypes_kind, declared_prototypes
from test_kernel_budget import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_render_budget_device", "rt_render_budget", "rt_adaptive_params_default", "rt_adaptive_plan_device", "rt_render_adaptive",
               "rt_render_adaptive_host")


def test_symbols_and_signatures_agree_with_the_header(rt):
    L = rt.lib()
    protos = {p[0]: p[1:] for p in declared_prototypes()}
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)
        assert name in rt.ABI_SYMBOLS and name in protos, name
        ret, params = protos[name]
        assert ctypes_kind(fn.restype) == ret and [ctypes_kind(a) for a in fn.argtypes] == params, name
    # read by eye from include/rt_amd.h
    assert protos["rt_render_budget_device"] == ("int32", ["pointer"] * 4 + ["int32"] + ["pointer"] * 5)
    assert protos["rt_adaptive_plan_device"] == ("int32", ["pointer", "int32", "int32"] + ["pointer"] * 8)
    assert protos["rt_render_adaptive"] == ("int32", ["pointer"] * 4 + ["int32"] + ["pointer"] * 5)
    # in the header's order: behind the denoiser, ahead of the multi-GPU entry points
    i = rt.ABI_SYMBOLS.index("rt_render_budget_device")
    assert rt.ABI_SYMBOLS[i - 1] == "rt_denoise" and rt.ABI_SYMBOLS[i:i + 7] == list(NEW_SYMBOLS) + ["rt_render_multi"]
    for name in ("render_budget", "render_budget_device", "adaptive_plan_device", "render_adaptive", "AdaptiveParams"):
        assert callable(getattr(rt, name)), name


def test_struct_sizes_constants_and_defaults(rt):
    hdr = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    assert C.sizeof(rt.rt_adaptive_params) == 32 and C.sizeof(rt.rt_adaptive_stats) == 272
    assert rt.rt_adaptive_stats.total_samples.offset == 8 and rt.rt_adaptive_stats.active_tiles.offset == 16
    assert int(re.search(r"#define RT_BUDGET_MAX (\d+)", hdr).group(1)) == rt.BUDGET_MAX == 65535 == np.iinfo(np.uint16).max
    assert int(re.search(r"#define RT_ADAPTIVE_MAX_SPP (\d+)", hdr).group(1)) == rt.ADAPTIVE_MAX_SPP == 1 << 24
    assert int(re.search(r"#define RT_ADAPTIVE_MAX_PASSES (\d+)", hdr).group(1)) == rt.ADAPTIVE_MAX_PASSES == 64
    p = rt.rt_adaptive_params()
    C.memset(C.byref(p), 0xAB, C.sizeof(p))
    rt.lib().rt_adaptive_params_default(C.byref(p))
    got = rt.AdaptiveParams().as_dict()
    assert got == {k: getattr(p, k) for k in got} and p.reserved[0] == 0
    # the yardstick restates them
    want = adaptive_ref.DEFAULTS
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k] == np.float32(v) if isinstance(v, float) else got[k] == v, (k, got[k], v)
    rt.lib().rt_adaptive_params_default(None)                      # a null pointer is ignored
    assert rt.AdaptiveParams(step_spp=3, pixel_threshold=0.5).as_dict()["step_spp"] == 3


def test_a_null_context_is_refused_before_hip(rt):
    """no GPU needed: the entry points check their context before they touch HIP, and before every other argument"""
    L = rt.lib()
    cam, rs, p = rt.Camera(8, 8), rt.RenderData(4, 8, True, (1, 1, 1)), rt.AdaptiveParams()
    budget = np.full((8, 8), 3, np.uint16)
    count = np.full((8, 8), 7, np.uint32)
    frame = np.full((8, 8, 3), 7.0, np.float32)
    u32p, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    st = rt.rt_adaptive_stats()
    assert L.rt_render_budget(None, None, C.byref(cam.c), C.byref(rs.c), 0, None, budget.ctypes.data, count.ctypes.data_as(u32p), frame.ctypes.data_as(fp)) == rt.RT_ERR_INVALID
    assert L.rt_render_budget_device(None, None, None, None, 0, None, None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_adaptive_plan_device(None, 8, 8, None, None, None, C.byref(p.c), None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_adaptive_plan_device(None, -1, 0, None, None, None, None, None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_render_adaptive(None, None, C.byref(cam.c), C.byref(rs.c), 0, C.byref(p.c), None, None, C.byref(st), None) == rt.RT_ERR_INVALID
    assert L.rt_render_adaptive_host(None, None, C.byref(cam.c), C.byref(rs.c), 0, C.byref(p.c), frame.ctypes.data_as(fp), count.ctypes.data_as(u32p), C.byref(st)) == rt.RT_ERR_INVALID
    assert np.all(count == 7) and np.all(frame == 7.0) and st.passes == 0 and st.total_samples == 0
    with pytest.raises(ValueError, match="budget must be"):
        rt.render_budget(None, None, cam, rs, 0, np.zeros((4, 4), np.uint16))


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_budget_kernel_register_budget(rt, tmp_path):
    """one budget kernel per shape of RT_SHAPES, each within what tests/test_kernel_budget.py allows the render kernel of its shape - and, unlike the
    sphere shapes of that kernel, without a spilled register or a byte of scratch"""
    notes = kernel_notes(rt, tmp_path)
    shape_of = lambda n: tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups())
    budget = {shape_of(n): v for n, v in notes.items() if "rt_budget_kernel" in n}
    render = {shape_of(n) for n in notes if "rt_render_kernel" in n}
    assert set(budget) == render and len(budget) == 13 and sum("rt_budget_kernel" in n for n in notes) == 13
    report = []
    for (nt, mesh, mode), v in sorted(budget.items()):
        report.append("threads %4d mesh %d mode %d: %s" % (nt, mesh, mode, v))
        assert v["agpr_count"] == 0 and v["vgpr_spill_count"] == 0 and v["scratch_insts"] == 0 and v["private_segment_fixed_size"] == 0, ((nt, mesh, mode), v)
        assert v["vgpr_count"] <= (128 if nt == 1024 else (96 if mesh else 80)), ((nt, mesh, mode), v)
        assert v["sgpr_spill_count"] <= (80 if mode == 1 else 96), ((nt, mesh, mode), v)
    for n, v in notes.items():
        if "rt_adaptive" in n:
            assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["scratch_insts"] == 0, (n, v)
    assert sum("rt_adaptive" in n for n in notes) == 2
    print("\n".join(report))


def test_parameter_ranges_of_the_yardstick_defaults():
    d = adaptive_ref.DEFAULTS
    assert 1 <= d["pilot_spp"] <= 65535 and 1 <= d["step_spp"] <= 65535 and d["pilot_spp"] <= d["max_spp"] <= 1 << 24 and 0 <= d["max_passes"] <= 64
    assert d["threshold"] > 0 and math.isfinite(d["threshold"]) and d["pixel_threshold"] > 0 and d["floor"] > 0 and math.isfinite(d["floor"])
