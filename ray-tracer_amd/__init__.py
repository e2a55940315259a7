"""ray-tracer_amd — host-side Python mirror of the reference's scene / camera / render
interface over the C ABI of libraytracer_amd.so (include/rt_amd.h).

Import with ``importlib.import_module("ray-tracer_amd")`` (the directory name has a hyphen).

The names follow the reference: ``Material.create_standard`` (src/material.cu:157),
``Object``-style factories on :class:`SceneObjects` (src/objects.cu:845-906),
:class:`ObjFileMesh` (src/obj_read.cu:47), :class:`Camera` (src/camera.cu:32),
:class:`RenderData` (src/raytracer.cu:4), :class:`VariableRenderData` + :func:`render`
(src/dispatch.cu:111-163).  All compute happens in the HIP library; there is no CPU path:
creating a :class:`Context` without a GPU raises.
"""
from . import build, scenes  # noqa: F401
from ._abi import C, np, os, sys  # noqa: F401  (rt.C, rt.np, rt.os, rt.sys are public names)
# rt.render and rt.denoise are the functions: each line below loads its module first, then binds the names over it
from ._abi import (ABI_SYMBOLS, ADAPTIVE_MAX_PASSES, ADAPTIVE_MAX_SPP, AO_MAX_SAMPLES, AO_NO_SURFACE, AOV_PLANES, HIT_DTYPE, HIT_MISS_T, MULTIHIT_MAX, NEAREST_DTYPE, OVERLAP_ID_DTYPE, OVERLAP_MAX, SWEEP_DTYPE, TRI_SEGMENT_DTYPE, MAT_EMISSIVE, MAT_REFRACTIVE, MAT_STANDARD, RT_ERR_BUSY, RT_ERR_HIP,  # noqa: F401
                   RT_ERR_INVALID, RT_ERR_IO, RT_ERR_NO_DEVICE, RT_ERR_NOMEM, RT_ERR_UNSUPPORTED, RT_OK, TEX_CHECKERBOARD, TEX_COLOUR,
                   TEX_GRADIENT, TEX_IMAGE, VIS_BLOCKED, VIS_LIT, VIS_NO_SURFACE, WINDING_BETA_DEFAULT, WINDING_LEAF_TRIS, WINDING_SOLIDS, PipelineFullError, RayTracerError, UnsupportedMeshError,
                   lib, rt_adaptive_params, rt_adaptive_stats, rt_camera, rt_denoise_params, rt_flat_view, rt_material, rt_rank, rt_render_settings, rt_scene_info, rt_tile_spec)
from .objects import (Camera, Context, Material, ObjFileMesh, RenderData, Scene, SceneObjects, VariableRenderData,  # noqa: F401
                      load_image_texture)
from .render import (PIPELINE_DEFAULT_DEPTH, PIPELINE_DEPTH, debug_eval, debug_exhaustive, frame_collect, frame_collect_host,  # noqa: F401
                     frame_depth, frame_submit, frame_wait, frames_pending, render, render_device, render_device_batch, render_frames,
                     save_png, tile_owned_rows, to_rgba8_device)
from .multi import gather, partition_tiles, render_multi, render_multi_device, tiles_copy_device  # noqa: F401
from .query import (NearestRecord, count_hits, distance_grid, nearest_points, nearest_points_device, occluded_rays, occluded_rays_device, render_ao, render_ao_device, render_aov, render_aov_device,  # noqa: F401
                    render_visibility, render_visibility_device, trace_rays, trace_rays_device, trace_rays_multi, trace_rays_multi_device, visible_between,
                    contains_points, signed_distance, signed_distance_device, signed_distance_fast, signed_distance_fast_device, signed_distance_grid, winding_numbers, winding_numbers_device,
                    winding_numbers_fast, winding_numbers_fast_device, SweepRecord, sweep_grid, sweep_spheres, sweep_spheres_device,
                    OverlapId, boxes_touch, overlap_boxes, overlap_boxes_device, voxel_boxes, voxelize,
                    TriSegment, collide_mesh, overlap_triangles, overlap_triangles_device, triangles_touch)
from .denoise import DenoiseParams, denoise, denoise_device, render_denoised  # noqa: F401
from .adaptive import BUDGET_MAX, AdaptiveParams, adaptive_plan_device, render_adaptive, render_budget, render_budget_device  # noqa: F401
from .views import VIEWS_MAX, lens_cameras, render_views, render_views_device  # noqa: F401
from .sky import SKY_MAX_FACE, Sky, render_sky, render_sky_device, sky_from_equirect, sky_texel_directions  # noqa: F401
from .cull import primary_cull_host, primary_cull_plane, primary_entry_host, primary_entry_words, primary_subentry_host, primary_subentry_tables, subtree_cull_host, subtree_cull_words  # noqa: F401
from .update import REBUILD_LDS_TRIS  # noqa: F401  (and Scene.update_mesh, Scene.update_mesh_device, Scene.debug_read)
