"""The scene-update entry points without a GPU: the symbols and their ctypes signatures against the header, RT_REBUILD_LDS_TRIS against the
binding and against the LDS budget it is derived from, the refusals a call meets before it touches HIP, the Python wrappers' argument checks,
and the rebuild kernels' register / scratch / LDS figures read from the code object inside the shipped library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_abi import ctypes_kind, declared_prototypes
from test_kernel_budget import kernel_notes

NEW_SYMBOLS = ("rt_scene_update_mesh_device", "rt_scene_update_mesh")


def test_symbols_and_signatures_agree_with_the_header(rt):
    L = rt.lib()
    protos = {p[0]: p[1:] for p in declared_prototypes()}
    for name in NEW_SYMBOLS + ("rt_debug_scene_read",):
        fn = getattr(L, name)
        assert name in rt.ABI_SYMBOLS and name in protos, name
        ret, params = protos[name]
        assert ctypes_kind(fn.restype) == ret and [ctypes_kind(a) for a in fn.argtypes] == params, name
    # read by eye from include/rt_amd.h: no struct crosses the two update calls
    assert protos["rt_scene_update_mesh_device"] == ("int32", ["pointer", "pointer", "int32", "pointer", "int32", "pointer"])
    assert protos["rt_scene_update_mesh"] == ("int32", ["pointer", "pointer", "int32", "pointer", "int32"])
    assert protos["rt_debug_scene_read"] == ("int32", ["pointer"] * 3)
    i = rt.ABI_SYMBOLS.index("rt_scene_update_mesh_device")
    assert rt.ABI_SYMBOLS[i - 1] == "rt_scene_get_info" and rt.ABI_SYMBOLS[i:i + 2] == list(NEW_SYMBOLS)
    for name in ("update_mesh", "update_mesh_device", "debug_read"):
        assert callable(getattr(rt.Scene, name)), name


def test_the_lds_constant_is_the_headers_and_fits_a_cu(rt):
    hdr = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    n = int(re.search(r"#define RT_REBUILD_LDS_TRIS (\d+)", hdr).group(1))
    assert n == rt.REBUILD_LDS_TRIS and n & (n - 1) == 0
    # per triangle: nine floats, a 64-bit word, two list positions, a commit index; beside them seven words per thread of partial boxes
    need = n * (36 + 8 + 8 + 4) + 1024 * 28
    assert need <= 160 * 1024 < 2 * n * (36 + 8 + 8 + 4) + 1024 * 28          # this size fits a CU's 160 KB of LDS, the next power of two does not


def test_refusals_before_hip(rt):
    """no GPU needed: a null context or scene is refused before anything else"""
    L = rt.lib()
    tris = np.zeros((4, 9), np.float32)
    p = tris.ctypes.data_as(C.POINTER(C.c_float))
    view = rt.rt_flat_view()
    assert L.rt_scene_update_mesh(None, None, 0, p, 4) == rt.RT_ERR_INVALID
    assert L.rt_scene_update_mesh_device(None, None, 0, None, 0, None) == rt.RT_ERR_INVALID
    assert L.rt_debug_scene_read(None, None, C.byref(view)) == rt.RT_ERR_INVALID
    assert not view.blob and view.blob_f4 == 0


class _NoContext:
    def _check(self, st):
        raise AssertionError("the wrapper reached the library")


def test_the_wrappers_check_their_arguments(rt):
    scene = rt.Scene.__new__(rt.Scene)                     # no handle: nothing to destroy
    scene.ctx = _NoContext()
    for bad in (np.zeros((4, 8), np.float32), np.zeros(36, np.float32), np.zeros((2, 2, 9), np.float32)):
        with pytest.raises(ValueError, match=r"\[n, 9\]"):
            scene.update_mesh(0, bad)
    with pytest.raises(ValueError, match="needs n"):
        scene.update_mesh_device(0, 0x1000)
    import torch
    for bad in (torch.zeros(4, 9), torch.zeros(4, 9, dtype=torch.float64), torch.zeros(9, 8).t()):
        with pytest.raises(ValueError, match="contiguous float32 tensor on the GPU"):
            scene.update_mesh_device(0, bad)


def test_the_rebuild_kernels_do_not_spill(rt, tmp_path):
    notes = {k: v for k, v in kernel_notes(rt, tmp_path).items() if "rt_rb_" in k}
    assert len(notes) == 6, sorted(notes)
    for name, note in notes.items():
        assert note["vgpr_spill_count"] == 0 and note["sgpr_spill_count"] == 0 and note["private_segment_fixed_size"] == 0, (name, note)
        assert note["vgpr_count"] <= 128, (name, note)                       # 1024-thread workgroups: four waves per SIMD
