"""The ray-query / AOV entry points without a GPU: the symbols and their ctypes signatures, the hit record's size in the header, in
ctypes and in NumPy, and the query kernels' register / scratch budget read from the code object inside the shipped library."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
NEW_SYMBOLS = ("rt_trace_rays", "rt_trace_rays_device", "rt_render_aov", "rt_render_aov_device")


def test_symbols_and_signatures(rt):
    L = rt.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    for name in NEW_SYMBOLS:
        assert name in rt.ABI_SYMBOLS and getattr(L, name) is not None, name
    assert L.rt_trace_rays.argtypes == [vp, vp, fp, fp, C.c_int64, vp]
    assert L.rt_trace_rays_device.argtypes == [vp, vp, vp, vp, C.c_int64, vp, vp]
    assert L.rt_render_aov.argtypes == [vp, vp, C.POINTER(rt.rt_camera), fp, fp, fp, fp, C.POINTER(C.c_int32), fp]
    assert L.rt_render_aov_device.argtypes == [vp, vp, C.POINTER(rt.rt_camera), fp, vp, vp, vp, vp, vp, vp]
    assert b"0.4" in L.rt_version()
    # refused before HIP is touched: no GPU needed
    assert L.rt_trace_rays(None, None, None, None, 1, None) == rt.RT_ERR_INVALID
    assert L.rt_trace_rays_device(None, None, None, None, 1, None, None) == rt.RT_ERR_INVALID
    assert L.rt_render_aov(None, None, None, None, None, None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_render_aov_device(None, None, None, None, None, None, None, None, None, None) == rt.RT_ERR_INVALID


def test_hit_record_size_and_offsets(rt, tmp_path):
    src = tmp_path / "hit.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %.1f\\n", sizeof(rt_hit), offsetof(rt_hit, point), offsetof(rt_hit, normal), '
                   'offsetof(rt_hit, object), offsetof(rt_hit, triangle), offsetof(rt_hit, u), offsetof(rt_hit, v), offsetof(rt_hit, reserved), (double)RT_HIT_MISS_T); return 0; }\n')
    exe = tmp_path / "hit"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    dt = rt.HIT_DTYPE
    assert int(out[0]) == dt.itemsize == 48 and dt.itemsize % 16 == 0
    assert [int(x) for x in out[1:8]] == [dt.fields[n][1] for n in ("point", "normal", "object", "triangle", "u", "v", "reserved")]
    assert float(out[8]) == float(rt.HIT_MISS_T) == 2.0 ** 30
    assert dt.names == ("t", "point", "normal", "object", "triangle", "u", "v", "reserved")


def kernel_notes(rt, tmp_path):
    """per kernel of the library's gfx950 code object: its resource notes and how many scratch instructions it holds"""
    lib = rt.build.build()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "discard.so")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)
    scratch, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            scratch[cur] = 0
        elif cur and re.search(r"\bscratch_", line):
            scratch[cur] += 1
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        def g(k):
            return re.search(r"\." + k + r":\s*(\S+)", blk).group(1)
        out[g("name")] = dict({k: int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")},
                              agpr_count=int(blk.split()[0]), scratch_insts=scratch.get(g("name"), -1))
    return out


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_query_kernel_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    assert sum("rt_render_kernel" in n for n in notes) == 13
    query = {n: v for n, v in notes.items() if "rt_query_kernel" in n}
    # every render shape, with and without the AOV front: <threads, has_mesh, mode, aov>
    shapes = set()
    for n, v in sorted(query.items()):
        m = re.search(r"ILi(\d+)ELb([01])ELi([012])ELb([01])E", n)
        shapes.add((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["scratch_insts"] == 0, (n, v)
        assert v["vgpr_count"] <= 128 and v["agpr_count"] == 0, (n, v)
    render = {tuple(int(x) for x in re.search(r"ILi(\d+)ELb([01])ELi([012])E", n).groups()) for n in notes if "rt_render_kernel" in n}
    assert shapes == {s + (a,) for s in render for a in (0, 1)} and len(query) == 26
