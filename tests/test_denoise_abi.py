"""The denoiser's entry points without a GPU: the symbols and their ctypes signatures, rt_denoise_params' layout in the header against
the binding, the null-context refusals, the defaults, and the denoise kernels' register / scratch budget read from the code object
inside the shipped library."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_query_abi import LLVM, kernel_notes

NEW_SYMBOLS = ("rt_denoise_params_default", "rt_denoise", "rt_denoise_device")
FIELDS = ("iterations", "sigma_colour", "sigma_depth", "normal_power_log2", "albedo_floor", "reserved")


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp, i32 = C.c_void_p, C.POINTER(C.c_float), C.c_int32
    dp = C.POINTER(rt.rt_denoise_params)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_denoise_params_default.argtypes == [dp] and L.rt_denoise_params_default.restype is None
    assert L.rt_denoise.argtypes == [vp, i32, i32, fp, fp, fp, C.POINTER(i32), fp, dp, fp]
    assert L.rt_denoise_device.argtypes == [vp, i32, i32, vp, vp, vp, vp, vp, dp, vp, vp]
    for name in ("DenoiseParams", "denoise", "denoise_device", "render_denoised"):
        assert callable(getattr(rt, name)), name


def test_params_size_and_offsets(rt, tmp_path):
    src = tmp_path / "params.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_denoise_params), '
                   + ", ".join("offsetof(rt_denoise_params, %s)" % f for f in FIELDS) + '); return 0; }\n')
    exe = tmp_path / "params"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = rt.rt_denoise_params
    assert out[0] == C.sizeof(P) == 32
    assert out[1:] == [getattr(P, f).offset for f in FIELDS]
    assert tuple(n for n, _ in P._fields_) == FIELDS


def test_null_context_is_refused_before_hip(rt):
    """no GPU needed: the entry points check their context before they touch HIP"""
    L = rt.lib()
    plane = (C.c_float * 12)()
    ids = (C.c_int32 * 4)()
    p = rt.DenoiseParams()
    assert L.rt_denoise(None, 2, 2, plane, plane, plane, ids, plane, C.byref(p.c), plane) == rt.RT_ERR_INVALID
    assert L.rt_denoise_device(None, 2, 2, None, None, None, None, None, C.byref(p.c), None, None) == rt.RT_ERR_INVALID
    assert L.rt_denoise(None, 0, 0, None, None, None, None, None, None, None) == rt.RT_ERR_INVALID
    L.rt_denoise_params_default(None)          # a null pointer is ignored


def test_defaults_are_in_range(rt):
    raw = rt.rt_denoise_params()
    C.memset(C.byref(raw), 0xFF, C.sizeof(raw))
    rt.lib().rt_denoise_params_default(C.byref(raw))
    assert 1 <= raw.iterations <= 8 and raw.sigma_colour > 0 and raw.sigma_depth > 0 and 0 <= raw.normal_power_log2 <= 8 and raw.albedo_floor > 0
    assert list(raw.reserved) == [0, 0, 0]
    p = rt.DenoiseParams(iterations=3, sigma_colour=0.5)
    assert p.c.iterations == 3 and p.c.sigma_colour == 0.5 and p.c.sigma_depth == raw.sigma_depth and p.as_dict()["normal_power_log2"] == raw.normal_power_log2
    # the header says what they are
    hdr = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    m = re.search(r"The defaults: iterations (\d+), sigma_colour (\d+(?:\.\d+)?), sigma_depth (\d+(?:\.\d+)?), normal_power_log2 (\d+), albedo_floor (\d+(?:\.\d+)?)", hdr)
    assert m, "the header names the defaults"
    assert (int(m.group(1)), int(m.group(4))) == (raw.iterations, raw.normal_power_log2)
    assert [C.c_float(float(m.group(k))).value for k in (2, 3, 5)] == [raw.sigma_colour, raw.sigma_depth, raw.albedo_floor]
    # ... and gives the spline constants in hex
    assert all(w in hdr for w in ("0x3E2AAAAB", "0x3F2AAAAB", "0x3F800000"))


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_denoise_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    dn = {n: v for n, v in notes.items() if "rt_denoise" in n}
    # the pack pass and the level pass with and without the final remodulation
    assert len(dn) == 3 and sum("rt_denoise_pack_kernel" in n for n in dn) == 1 and sum("rt_denoise_level_kernel" in n for n in dn) == 2, sorted(dn)
    for n, v in sorted(dn.items()):
        print(n, v)
        assert not any(w in n for w in ("rt_render_kernel", "rt_query_kernel", "rt_occlusion_kernel")), n
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (n, v)
        assert v["agpr_count"] == 0, (n, v)
        # <= 64 registers: eight waves per SIMD can be resident (the kernels take 24 / 33 / 32)
        assert v["vgpr_count"] <= 64, (n, v)
    # the counted kernels are what they were
    assert sum("rt_render_kernel" in n for n in notes) == 13 and sum("rt_query_kernel" in n for n in notes) == 26 and sum("rt_occlusion_kernel" in n for n in notes) == 26
