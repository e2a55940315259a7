"""The C-ABI shared library: it loads, exports every symbol include/rt_amd.h declares, and
refuses to work without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np

import pytest

from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree(rt):
    assert declared_symbols() == sorted(rt.ABI_SYMBOLS)


def c_kind(decl, is_return=False):
    """a C parameter declaration (or a return type) -> pointer / float / int32 / int64 / void"""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    (base,) = words if is_return else words[:-1]          # a parameter's last word is its name
    return {"float": "float", "int32_t": "int32", "rt_status": "int32", "int64_t": "int64", "void": "void"}[base]


def declared_prototypes():
    """include/rt_amd.h -> [(name, return kind, [parameter kinds])] in the header's order"""
    text = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = []
    for statement in text.split(";"):
        m = re.search(r"([\w\s\*]+?)\b(rt_[a-z0-9_]+)\s*\((.*)\)\s*$", statement, flags=re.S)
        if m:
            ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
            params = [] if params == "void" else [p.strip() for p in params.split(",")]
            protos.append((name, c_kind(ret, is_return=True), [c_kind(p) for p in params]))
    return protos


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_float: "float", ctypes.c_int32: "int32", ctypes.c_int64: "int64"}[t]


def abi_module():
    import importlib
    return importlib.import_module("ray-tracer_amd._abi")


def test_signature_table_agrees_with_the_header(rt):
    """every function's return and every parameter, in number and kind - not only the names"""
    protos = declared_prototypes()
    table = abi_module().ABI
    assert [p[0] for p in protos] == list(table) == rt.ABI_SYMBOLS          # the header's order, each function once
    assert ctypes.sizeof(ctypes.c_int32) == 4 and ctypes.sizeof(ctypes.c_int64) == 8 and ctypes.sizeof(ctypes.c_float) == 4
    for name, ret, params in protos:
        restype, argtypes = table[name]
        assert ctypes_kind(restype) == ret, name
        assert len(argtypes) == len(params), name
        assert [ctypes_kind(a) for a in argtypes] == params, name


def test_header_parser_sees_the_kinds():
    """the parser itself, on prototypes read by eye"""
    protos = {p[0]: p[1:] for p in declared_prototypes()}
    assert protos["rt_version"] == ("pointer", [])
    assert protos["rt_material_checkerboard"] == ("void", ["pointer", "pointer", "pointer", "int32", "float"])
    assert protos["rt_trace_rays"] == ("int32", ["pointer", "pointer", "pointer", "pointer", "int64", "pointer"])
    assert protos["rt_frames_pending"] == ("int32", ["pointer"])
    assert protos["rt_debug_exhaustive"] == ("int32", ["pointer", "pointer"])


def test_applying_the_table_skips_missing_symbols(rt):
    """a library of an older revision (loaded through RT_AMD_LIB) lacks the newer entry points: the rest is still declared"""
    import types
    abi = abi_module()
    present = ["rt_render", "rt_version", "rt_obj_destroy"]
    stand_in = types.SimpleNamespace(**{n: types.SimpleNamespace() for n in present})
    abi.apply_abi(stand_in)
    assert sorted(vars(stand_in)) == sorted(present)
    for n in present:
        assert (getattr(stand_in, n).restype, getattr(stand_in, n).argtypes) == abi.ABI[n]
    L = rt.lib()
    for name, (restype, argtypes) in abi.ABI.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and fn.restype is restype, name


def test_library_exports_every_declared_symbol(rt):
    L = rt.lib()
    for name in declared_symbols():
        assert getattr(L, name) is not None, name
    assert b"gfx950" in L.rt_version()


def test_struct_layouts(rt):
    # the ctypes mirrors must match the header's PODs (4-byte fields, no padding)
    assert ctypes.sizeof(rt.rt_material) == 4 * (2 + 3 + 3 + 3 + 1 + 1 + 1 + 3 + 1) + 8 + 8      # ... + img_w, img_h + pointer
    assert ctypes.sizeof(rt.rt_camera) == 4 * 14
    assert ctypes.sizeof(rt.rt_render_settings) == 4 * 6
    assert ctypes.sizeof(rt.rt_tile_spec) == 48       # four ints, three pointers, one int (+ padding)


def test_material_factories(rt):
    m = rt.Material.create_standard((0.7, 0.3, 0.3), 0.25).c
    assert (m.type, m.tex_type, m.need_uv) == (rt.MAT_STANDARD, rt.TEX_COLOUR, 0) and abs(m.smoothness - 0.25) < 1e-7
    e = rt.Material.create_emissive((1, 0.5, 0.25), 6).c
    # src/material.cu:170 emitted = colour * strength; fields the reference leaves unset are 0
    assert list(e.emitted_light) == [6.0, 3.0, 1.5] and e.smoothness == 0.0 and e.need_uv == 0 and e.type == rt.MAT_EMISSIVE
    c = rt.Material.create_checkerboard((1, 1, 1), (0, 0, 0), 8, 0).c
    assert (c.tex_type, c.need_uv, c.num_squares) == (rt.TEX_CHECKERBOARD, 1, 8)
    r = rt.Material.create_refractive((1, 1, 1), 1.5).c
    # src/material.cu:175-185: smoothness forced to 1
    assert (r.type, r.smoothness, r.need_uv) == (rt.MAT_REFRACTIVE, 1.0, 0) and abs(r.refractive_index - 1.5) < 1e-7
    i = rt.Material.create_image(np.zeros((4, 6, 3), np.float32), 0.5).c
    assert (i.tex_type, i.need_uv, i.img_w, i.img_h) == (rt.TEX_IMAGE, 1, 6, 4)


def test_no_gpu_means_failure_not_fallback(rt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(rt.RayTracerError, match="no CPU fallback"):
        rt.Context(0)


def test_pipelined_entry_points_refuse_a_null_context(rt):
    """no GPU needed: the frames-in-flight entry points check their context before they touch HIP"""
    import ctypes as C
    L = rt.lib()
    assert L.rt_frame_submit(None, None, None, None, 0, None) == rt.RT_ERR_INVALID
    assert L.rt_frame_collect(None, 0, None, None) == rt.RT_ERR_INVALID
    assert L.rt_frame_collect_host(None, C.byref(C.c_int32(0)), None) == rt.RT_ERR_INVALID
    assert L.rt_frame_wait(None) == rt.RT_ERR_INVALID
    assert L.rt_frame_depth(None, 4) == rt.RT_ERR_INVALID
    assert L.rt_frames_pending(None) == 0
    assert (rt.PIPELINE_DEFAULT_DEPTH, rt.PIPELINE_DEPTH) == (4, 8)
    # the header's macros say the same
    import os, re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_amd.h")).read()
    assert int(re.search(r"#define RT_PIPELINE_DEPTH (\d+)", hdr).group(1)) == rt.PIPELINE_DEPTH
    assert int(re.search(r"#define RT_PIPELINE_DEFAULT_DEPTH (\d+)", hdr).group(1)) == rt.PIPELINE_DEFAULT_DEPTH
    assert int(re.search(r"RT_ERR_BUSY = (\d+)", hdr).group(1)) == rt.RT_ERR_BUSY
