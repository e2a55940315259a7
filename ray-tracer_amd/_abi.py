"""The C ABI of libraytracer_amd.so (include/rt_amd.h) as ctypes: constants, struct mirrors, one signature table, the loader,
and the few argument conversions the wrapper modules share."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

from . import build as _build

RT_OK, RT_ERR_INVALID, RT_ERR_IO, RT_ERR_UNSUPPORTED, RT_ERR_HIP, RT_ERR_NOMEM, RT_ERR_NO_DEVICE, RT_ERR_BUSY = range(8)
TEX_COLOUR, TEX_GRADIENT, TEX_CHECKERBOARD, TEX_IMAGE = 0, 1, 2, 3
MAT_STANDARD, MAT_EMISSIVE, MAT_REFRACTIVE = 0, 1, 2


class rt_material(C.Structure):
    _fields_ = [("type", C.c_int32), ("tex_type", C.c_int32), ("colour", C.c_float * 3),
                ("light", C.c_float * 3), ("dark", C.c_float * 3), ("num_squares", C.c_int32),
                ("smoothness", C.c_float), ("need_uv", C.c_int32), ("emitted_light", C.c_float * 3),
                ("refractive_index", C.c_float), ("img_w", C.c_int32), ("img_h", C.c_int32),
                ("img_rgb", C.POINTER(C.c_float))]


class rt_camera(C.Structure):
    _fields_ = [("cam_pos", C.c_float * 3), ("tl_pixel_pos", C.c_float * 3), ("delta_u", C.c_float * 3),
                ("delta_v", C.c_float * 3), ("width", C.c_int32), ("height", C.c_int32)]


class rt_render_settings(C.Structure):
    _fields_ = [("rays_per_pixel", C.c_int32), ("reflection_limit", C.c_int32), ("antialias", C.c_int32),
                ("sky_colour", C.c_float * 3)]


class rt_tile_spec(C.Structure):
    _fields_ = [("band_rows", C.c_int32), ("band_first", C.c_int32), ("band_stride", C.c_int32), ("compact", C.c_int32),
                ("tile_list", C.POINTER(C.c_uint32)), ("tile_cost", C.POINTER(C.c_uint32)), ("tile_peak", C.POINTER(C.c_uint32)),
                ("num_tiles", C.c_int32)]


class rt_rank(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("scene", C.c_void_p)]


class rt_scene_info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_objects", "num_triangles", "num_nodes", "lds_bytes", "scene_in_lds", "threads_per_block", "stack_entries", "blocks_per_cu", "kernel_variant")]


# rt_scene_info.kernel_variant / rt_flat_view.kernel_variant by name, and rt_flat_view.traits' bits (rt_device_scene.h RT_TRAIT_*)
KERNEL_VARIANTS = ("generic", "traits")
SCENE_TRAITS = {"SPHERES_ONLY": 1, "ONE_MESH": 2, "PLAIN_MATERIALS": 4}


class rt_flat_view(C.Structure):
    _fields_ = [("blob", C.POINTER(C.c_float)), ("blob_f4", C.c_int32), ("off_nodes", C.c_int32),
                ("off_tris", C.c_int32), ("off_objlds", C.c_int32), ("off_meshes", C.c_int32), ("num_meshes", C.c_int32),
                ("stack_entries", C.c_int32), ("objects", C.c_void_p),
                ("num_objects", C.c_int32), ("object_stride", C.c_int32), ("tri_uv", C.POINTER(C.c_float)),
                ("num_triangles", C.c_int32), ("num_nodes", C.c_int32), ("has_mesh", C.c_int32),
                ("traits", C.c_int32), ("kernel_variant", C.c_int32), ("tri_flip", C.POINTER(C.c_uint8))]


class rt_winding_tree_view(C.Structure):
    _fields_ = [("skip", C.POINTER(C.c_int32)), ("first", C.POINTER(C.c_int32)), ("count", C.POINTER(C.c_int32)), ("num_clusters", C.c_int32),
                ("object_range", C.POINTER(C.c_int32)), ("num_objects", C.c_int32), ("order", C.POINTER(C.c_int32)), ("num_triangles", C.c_int32),
                ("position", C.POINTER(C.c_int32)), ("moments", C.POINTER(C.c_float))]


class rt_denoise_params(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_colour", C.c_float), ("sigma_depth", C.c_float), ("normal_power_log2", C.c_int32),
                ("albedo_floor", C.c_float), ("reserved", C.c_int32 * 3)]


class rt_adaptive_params(C.Structure):
    _fields_ = [("pilot_spp", C.c_int32), ("step_spp", C.c_int32), ("max_spp", C.c_int32), ("max_passes", C.c_int32),
                ("threshold", C.c_float), ("pixel_threshold", C.c_float), ("floor", C.c_float), ("reserved", C.c_int32 * 1)]


ADAPTIVE_MAX_PASSES, ADAPTIVE_MAX_SPP = 64, 1 << 24   # RT_ADAPTIVE_*
BUDGET_MAX = 65535                                     # RT_BUDGET_MAX: the most samples one budget render gives a pixel
REBUILD_LDS_TRIS = 2048                                # RT_REBUILD_LDS_TRIS: the largest tree segment one workgroup rebuilds in LDS (update_mesh)
VIEWS_MAX = 32                                         # RT_VIEWS_MAX: the views one launch of render_views_device renders
SKY_MAX_FACE = 2048                                    # RT_SKY_MAX_FACE: the most texels on the side of a cube-map sky's face


class rt_adaptive_stats(C.Structure):
    _fields_ = [("passes", C.c_int32), ("reserved", C.c_int32), ("total_samples", C.c_uint64), ("active_tiles", C.c_int32 * ADAPTIVE_MAX_PASSES)]


# rt_hit (include/rt_amd.h) as a NumPy record: what trace_rays returns
HIT_DTYPE = np.dtype([("t", np.float32), ("point", np.float32, (3,)), ("normal", np.float32, (3,)), ("object", np.int32),
                      ("triangle", np.int32), ("u", np.float32), ("v", np.float32), ("reserved", np.int32)])
HIT_MISS_T = np.float32(1073741824.0)      # RT_HIT_MISS_T
# rt_nearest (include/rt_amd.h) as a NumPy record: what nearest_points returns.  A miss: distance and distance2 HIT_MISS_T, object -1
NEAREST_DTYPE = np.dtype([("distance", np.float32), ("distance2", np.float32), ("point", np.float32, (3,)), ("object", np.int32),
                          ("triangle", np.int32), ("reserved", np.int32)])
# rt_sweep (include/rt_amd.h) as a NumPy record: what sweep_spheres returns.  A miss: t HIT_MISS_T, object, triangle and feature -1
SWEEP_DTYPE = np.dtype([("t", np.float32), ("centre", np.float32, (3,)), ("point", np.float32, (3,)), ("object", np.int32), ("triangle", np.int32),
                        ("feature", np.int32), ("overlap", np.int32), ("reserved", np.int32)])
WINDING_SOLIDS = -1                                 # RT_WINDING_SOLIDS: the `object` that asks for the sum over the spheres, cuboids and meshes
WINDING_BETA_DEFAULT, WINDING_LEAF_TRIS = 2.0, 8   # RT_WINDING_BETA_DEFAULT, RT_WINDING_LEAF_TRIS: the fast winding numbers' accuracy parameter and leaf size
# rt_overlap_id (include/rt_amd.h) as a NumPy record: what overlap_boxes returns per rank.  An empty slot: {-1, -1}
OVERLAP_ID_DTYPE = np.dtype([("object", np.int32), ("triangle", np.int32)])
OVERLAP_MAX = 8                                   # RT_OVERLAP_MAX: the most ids per box of overlap_boxes
# rt_tri_segment (include/rt_amd.h) as a NumPy record: what overlap_triangles returns per rank with segments=True.  kind 0: an empty slot;
# 1: a segment from p to q; 2: a pair that has no segment (a sphere, a coplanar pair), its floats NaN
TRI_SEGMENT_DTYPE = np.dtype([("p", np.float32, (3,)), ("q", np.float32, (3,)), ("kind", np.int32), ("reserved", np.int32)])
MULTIHIT_MAX = 8                                  # RT_MULTIHIT_MAX: the most records per ray of trace_rays_multi
AOV_PLANES = ("depth", "normal", "albedo", "object", "ray")
VIS_BLOCKED, VIS_LIT, VIS_NO_SURFACE = 0, 1, 2      # RT_VIS_*: the bytes of render_visibility's plane
AO_PLANES = ("ao", "count")
AO_NO_SURFACE, AO_MAX_SAMPLES = 0xFFFF, 4096        # RT_AO_*: render_ao's count where the primary ray hit nothing; the most samples

# Every function include/rt_amd.h declares, in its order: name -> (restype, [argtypes]).  tests/test_abi.py parses the header and
# checks each row's parameter count and kinds.  st: rt_status; vp: an opaque handle, a device pointer, a hipStream_t, or a host
# buffer the wrappers pass by address.
st = i32 = C.c_int32
i64, f32, vp, cstr = C.c_int64, C.c_float, C.c_void_p, C.c_char_p
fp, i32p, u32p, u64p, vpp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)
mat, cam, rs = C.POINTER(rt_material), C.POINTER(rt_camera), C.POINTER(rt_render_settings)
tiles, ranks, dnp = C.POINTER(rt_tile_spec), C.POINTER(rt_rank), C.POINTER(rt_denoise_params)
adp, ads = C.POINTER(rt_adaptive_params), C.POINTER(rt_adaptive_stats)
ABI = {
    "rt_material_standard": (None, [mat, fp, f32]),
    "rt_material_checkerboard": (None, [mat, fp, fp, i32, f32]),
    "rt_material_gradient": (None, [mat, f32]),
    "rt_material_emissive": (None, [mat, fp, f32]),
    "rt_material_refractive": (None, [mat, fp, f32]),
    "rt_material_image": (None, [mat, i32, i32, fp, f32]),
    "rt_image_texture_load": (st, [cstr, cstr, i32p, i32p, C.POINTER(fp)]),
    "rt_image_texture_free": (None, [fp]),
    "rt_scene_builder_create": (st, [vpp]),
    "rt_scene_builder_destroy": (None, [vp]),
    "rt_scene_builder_error": (cstr, [vp]),
    "rt_scene_add_sphere": (st, [vp, fp, f32, mat]),
    "rt_scene_add_triangle": (st, [vp, fp, fp, fp, mat]),
    "rt_scene_add_triangle_uv": (st, [vp, fp, fp, mat]),
    "rt_scene_add_quad": (st, [vp, fp, fp, fp, fp, mat]),
    "rt_scene_add_one_way_quad": (st, [vp, fp, fp, fp, fp, i32, mat]),
    "rt_scene_add_cuboid": (st, [vp, fp, f32, f32, f32, mat]),
    "rt_scene_add_mesh": (st, [vp, fp, i32, mat]),
    "rt_scene_add_obj_mesh": (st, [vp, vp, mat]),
    "rt_scene_builder_num_objects": (i32, [vp]),
    "rt_obj_load": (st, [cstr, vpp]),
    "rt_obj_destroy": (None, [vp]),
    "rt_obj_enlarge": (None, [vp, f32]),
    "rt_obj_rotate": (None, [vp, f32, f32, f32]),
    "rt_obj_translate": (None, [vp, f32, f32, f32]),
    "rt_obj_num_vertices": (i32, [vp]),
    "rt_obj_num_faces": (i32, [vp]),
    "rt_obj_face_arity": (i32, [vp, i32]),
    "rt_obj_get_face": (None, [vp, i32, i32p]),
    "rt_obj_from_arrays": (st, [fp, i32, i32p, i32p, i32, vpp]),
    "rt_obj_get_vertices": (None, [vp, fp]),
    "rt_obj_num_triangles": (i32, [vp]),
    "rt_obj_get_triangles": (st, [vp, fp]),
    "rt_camera_default": (None, [i32, i32, cam]),
    "rt_camera_make": (None, [i32, i32, fp, f32, f32, f32, f32, f32, cam]),
    "rt_ctx_create": (st, [i32, vpp]),
    "rt_ctx_destroy": (None, [vp]),
    "rt_last_error": (cstr, [vp]),
    "rt_scene_commit": (st, [vp, vp, vpp]),
    "rt_scene_destroy": (None, [vp]),
    "rt_scene_get_info": (st, [vp, C.POINTER(rt_scene_info)]),
    "rt_scene_update_mesh_device": (st, [vp, vp, i32, vp, i32, vp]),
    "rt_scene_update_mesh": (st, [vp, vp, i32, fp, i32]),
    "rt_render": (st, [vp, vp, cam, rs, i32, i32p, fp]),
    "rt_render_frames": (st, [vp, vp, cam, rs, i32p, i32, i32p, fp]),
    "rt_render_device": (st, [vp, vp, cam, rs, i32, i32, tiles, vp, vp, vp]),
    "rt_render_device_batch": (st, [vp, vp, cam, rs, i32p, i32, i32, tiles, vp, vp]),
    "rt_frame_depth": (st, [vp, i32]),
    "rt_frame_submit": (st, [vp, vp, cam, rs, i32, tiles]),
    "rt_frame_collect": (st, [vp, i32, vp, vp]),
    "rt_frame_collect_host": (st, [vp, i32p, fp]),
    "rt_frames_pending": (i32, [vp]),
    "rt_frame_wait": (st, [vp]),
    "rt_render_views_device": (st, [vp, vp, cam, i32p, i32, rs, i32, i32, vp, vp]),
    "rt_render_views": (st, [vp, vp, cam, i32p, i32, rs, i32, i32p, fp]),
    "rt_camera_lens": (st, [cam, f32, f32, f32, f32, cam]),
    "rt_sky_create": (st, [vp, i32, fp, vpp]),
    "rt_sky_destroy": (None, [vp]),
    "rt_sky_texel_direction": (st, [i32, i32, i32, i32, fp]),
    "rt_render_sky_device": (st, [vp, vp, vp, cam, i32p, i32, rs, i32, i32, vp, vp]),
    "rt_render_sky": (st, [vp, vp, vp, cam, i32p, i32, rs, i32, i32p, fp]),
    "rt_tile_owned_rows": (i32, [tiles, i32]),
    "rt_tile_costs": (st, [vp, u32p, u32p, u32p, i32, i32p]),
    "rt_partition_tiles": (st, [u32p, i32, i32, i32, i32p]),
    "rt_tiles_copy_device": (st, [vp, vp, vp, i32, i32, u32p, i32, i32, vp]),
    "rt_max_batch_frames": (i32, [vp, i32, i32]),
    "rt_last_kernel_ms": (st, [vp, fp]),
    "rt_ctx_synchronize": (st, [vp]),
    "rt_trace_rays_device": (st, [vp, vp, vp, vp, i64, vp, vp]),
    "rt_trace_rays": (st, [vp, vp, fp, fp, i64, vp]),
    "rt_render_aov_device": (st, [vp, vp, cam, fp, vp, vp, vp, vp, vp, vp]),
    "rt_render_aov": (st, [vp, vp, cam, fp, fp, fp, fp, i32p, fp]),
    "rt_nearest_points_device": (st, [vp, vp, vp, vp, i64, vp, vp]),
    "rt_nearest_points": (st, [vp, vp, fp, fp, i64, vp]),
    "rt_winding_numbers_device": (st, [vp, vp, vp, i64, i32, vp, vp, vp]),
    "rt_winding_numbers": (st, [vp, vp, fp, i64, i32, fp, vp]),
    "rt_signed_distance_device": (st, [vp, vp, vp, vp, i64, vp, vp, vp]),
    "rt_signed_distance": (st, [vp, vp, fp, fp, i64, vp, fp]),
    "rt_winding_numbers_fast_device": (st, [vp, vp, vp, i64, i32, f32, vp, vp, vp]),
    "rt_winding_numbers_fast": (st, [vp, vp, fp, i64, i32, f32, fp, vp]),
    "rt_signed_distance_fast_device": (st, [vp, vp, vp, vp, i64, f32, vp, vp, vp]),
    "rt_signed_distance_fast": (st, [vp, vp, fp, fp, i64, f32, vp, fp]),
    "rt_trace_rays_multi_device": (st, [vp, vp, vp, vp, vp, i64, i32, vp, vp, vp]),
    "rt_trace_rays_multi": (st, [vp, vp, fp, fp, fp, i64, i32, vp, i32p]),
    "rt_sweep_spheres_device": (st, [vp, vp, vp, vp, vp, vp, i64, vp, vp]),
    "rt_sweep_spheres": (st, [vp, vp, fp, fp, fp, fp, i64, vp]),
    "rt_overlap_boxes_device": (st, [vp, vp, vp, vp, i64, i32, vp, vp, vp, vp]),
    "rt_overlap_boxes": (st, [vp, vp, fp, fp, i64, i32, vp, i32p, vp]),
    "rt_overlap_triangles_device": (st, [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp]),
    "rt_overlap_triangles": (st, [vp, vp, fp, i64, i32, vp, i32p, vp, vp]),
    "rt_occluded_rays_device": (st, [vp, vp, vp, vp, vp, i64, vp, vp]),
    "rt_occluded_rays": (st, [vp, vp, fp, fp, fp, i64, vp]),
    "rt_render_visibility_device": (st, [vp, vp, cam, fp, f32, vp, vp]),
    "rt_render_visibility": (st, [vp, vp, cam, fp, f32, vp]),
    "rt_render_ao_device": (st, [vp, vp, cam, i32, f32, f32, i32, vp, vp, vp]),
    "rt_render_ao": (st, [vp, vp, cam, i32, f32, f32, i32, vp, fp]),
    "rt_denoise_params_default": (None, [dnp]),
    "rt_denoise_device": (st, [vp, i32, i32, vp, vp, vp, vp, vp, dnp, vp, vp]),
    "rt_denoise": (st, [vp, i32, i32, fp, fp, fp, i32p, fp, dnp, fp]),
    "rt_render_budget_device": (st, [vp, vp, cam, rs, i32, tiles, vp, vp, vp, vp]),
    "rt_render_budget": (st, [vp, vp, cam, rs, i32, tiles, vp, u32p, fp]),
    "rt_adaptive_params_default": (None, [adp]),
    "rt_adaptive_plan_device": (st, [vp, i32, i32, vp, vp, vp, adp, vp, vp, vp, vp]),
    "rt_render_adaptive": (st, [vp, vp, cam, rs, i32, adp, vp, vp, ads, vp]),
    "rt_render_adaptive_host": (st, [vp, vp, cam, rs, i32, adp, fp, u32p, ads]),
    "rt_render_multi": (st, [ranks, i32, cam, rs, i32p, i32, i32p, fp]),
    "rt_render_multi_device": (st, [ranks, i32, cam, rs, i32p, i32, i32, i32, vp, vp]),
    "rt_gather": (st, [vp, vp, i32, i32, vp, vp, tiles, vp]),
    "rt_peer_access": (i32, [vp, vp]),
    "rt_to_rgba8_device": (st, [vp, vp, i32, i32, vp, vp]),
    "rt_debug_flatten": (st, [vp, C.POINTER(rt_flat_view)]),
    "rt_debug_scene_read": (st, [vp, vp, C.POINTER(rt_flat_view)]),
    "rt_debug_winding_tree": (st, [vp, C.POINTER(rt_winding_tree_view)]),
    "rt_debug_scene_winding_tree": (st, [vp, vp, C.POINTER(rt_winding_tree_view)]),
    "rt_debug_primary_cull": (st, [vp, u32p, i32, i32p]),
    "rt_debug_primary_cull_host": (st, [C.POINTER(rt_flat_view), cam, i32, u32p, C.POINTER(C.c_int64)]),
    "rt_debug_subtree_cull": (st, [vp, u32p, i32, i32p]),
    "rt_debug_subtree_cull_host": (st, [C.POINTER(rt_flat_view), cam, i32, u32p, C.POINTER(C.c_int64)]),
    "rt_debug_primary_entry": (st, [vp, u32p, i32, i32p]),
    "rt_debug_primary_entry_host": (st, [C.POINTER(rt_flat_view), cam, i32, u32p, C.POINTER(C.c_int64)]),
    "rt_debug_primary_subentry": (st, [vp, u32p, u32p, i32, i32p]),
    "rt_debug_primary_subentry_host": (st, [C.POINTER(rt_flat_view), cam, i32, i32, u32p, u32p, i32, C.POINTER(C.c_int64)]),
    "rt_debug_eval": (st, [vp, i32, u32p, u32p, i32]),
    "rt_debug_exhaustive": (st, [vp, u64p]),
    "rt_debug_read_stats": (st, [vp, u64p]),
    "rt_version": (cstr, []),
}
ABI_SYMBOLS = list(ABI)


def apply_abi(L):
    """Declare restype and argtypes of the table's functions on L.  A symbol L does not export is skipped: libraries of older
    revisions, which lack the newer entry points, are loaded through RT_AMD_LIB (tools/build_variants.py name@REV, and a bench.py
    comparison with the parent commit's library); every build of this tree exports them all (tests/test_abi.py)."""
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes


_lib = None


def lib():
    """Load libraytracer_amd.so (building it with hipcc if the sources are newer).  Raises if
    the HIP extension cannot be built or loaded: there is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RT_AMD_LIB") or _build.build()      # RT_AMD_LIB: development builds (tools/)
    # PyTorch-ROCm bundles its own libamdhip64.so.7.  Two HIP runtimes in one process cannot
    # both own the GPU, so when torch is installed it is imported first and this library then
    # binds (by SONAME) to the runtime torch already loaded; device pointers and streams are
    # then shared.  RT_AMD_NO_TORCH=1 skips this (pure ctypes use against /opt/rocm).
    if "torch" not in sys.modules and os.environ.get("RT_AMD_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    apply_abi(L)
    _lib = L
    return L


class RayTracerError(RuntimeError):
    """std::runtime_error of the reference (check_cuda_error src/utils.cu:5-10, read_file src/obj_read.cu:10)."""


class PipelineFullError(RayTracerError):
    """rt_frame_submit: RT_PIPELINE_DEPTH frames are in flight (RT_ERR_BUSY)"""


class UnsupportedMeshError(ValueError):
    """std::logic_error("Only triangle or quad meshes are supported.") src/main.cu:141"""


# ---- argument conversions shared by the wrapper modules -------------------------------------------
def _fp(a):
    arr = np.ascontiguousarray(a, dtype=np.float32)
    return arr, arr.ctypes.data_as(fp)


def _dptr(p):
    """a device pointer or stream given as an int; None is NULL"""
    return C.c_void_p(p or 0)


def _times(times_ms):
    return (C.c_int32 * len(times_ms))(*[int(x) for x in times_ms])


def _u32_backing(ids):
    """(a NULL list pointer means "bands": an empty list still needs an address)"""
    return ids if ids.size else np.zeros(1, np.uint32)


def _ray_arrays(origins, directions):
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape")
    return o, d


@contextlib.contextmanager
def _host_frame(data):
    """rt_render's host-buffer contract: yields (frame_num*, previous_render*) of a VariableRenderData for one call and stores the
    advanced frame_num afterwards - not when the call raised"""
    fn = C.c_int32(int(data.frame_num))
    buf = data.previous_render
    assert buf.dtype == np.float32 and buf.flags["C_CONTIGUOUS"]
    yield C.byref(fn), buf.ctypes.data_as(fp)
    data.frame_num = fn.value
