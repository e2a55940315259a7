"""Per-pixel sample budgets and the adaptive sampling loop (include/rt_amd.h: rt_render_budget, rt_adaptive_plan_device, rt_render_adaptive)."""
import ctypes as C

import numpy as np

from ._abi import BUDGET_MAX, _dptr, lib, rt_adaptive_params, rt_adaptive_stats  # noqa: F401  (BUDGET_MAX is a public name of this module)
from .render import _tile_spec

_FIELDS = ("pilot_spp", "step_spp", "max_spp", "max_passes", "threshold", "pixel_threshold", "floor")


class AdaptiveParams:
    """rt_adaptive_params (include/rt_amd.h): the library's defaults (rt_adaptive_params_default) with the given fields replaced"""

    def __init__(self, pilot_spp=None, step_spp=None, max_spp=None, max_passes=None, threshold=None, pixel_threshold=None, floor=None):
        self.c = rt_adaptive_params()
        lib().rt_adaptive_params_default(C.byref(self.c))
        for name, value in zip(_FIELDS, (pilot_spp, step_spp, max_spp, max_passes, threshold, pixel_threshold, floor)):
            if value is not None:
                setattr(self.c, name, value)

    def as_dict(self):
        return {n: getattr(self.c, n) for n in _FIELDS}


def _tiles(tile_list):
    """(the tile spec or None, what to pass): None is the whole image"""
    if tile_list is None:
        return None, None
    ts = _tile_spec(8, 0, 1, False, tile_list, None)
    return ts, C.byref(ts)


def _stats(s):
    return {"passes": int(s.passes), "total_samples": int(s.total_samples), "active_tiles": [int(x) for x in s.active_tiles[:s.passes]]}


def render_budget_device(ctx, scene, camera, render_data, time_ms, d_budget, d_frame, d_count=None, tile_list=None, stream=None):
    """Device-buffer form (rt_render_budget_device): d_budget (W*H uint16), d_frame (W*H*3 float32) and d_count (W*H uint32, or None)
    are device pointers; every pixel takes its budget's samples and its mean is folded into d_frame by sample counts.  tile_list: only
    these 8x8 tiles, in this order.  Asynchronous on `stream`."""
    ts, tsp = _tiles(tile_list)
    ctx._check(lib().rt_render_budget_device(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), int(time_ms), tsp, _dptr(d_budget), _dptr(d_count),
                                             _dptr(d_frame), _dptr(stream)))


def render_budget(ctx, scene, camera, render_data, time_ms, budget, frame=None, count=None, tile_list=None):
    """Host-buffer form (rt_render_budget): budget [H, W] uint16; frame [H, W, 3] float32 and count [H, W] uint32 are the accumulation so
    far (None: nothing yet) and are not changed.  Returns the new (frame, count)."""
    H, W = camera.height, camera.width
    b = np.ascontiguousarray(budget, dtype=np.uint16)
    if b.shape != (H, W):
        raise ValueError("budget must be [H, W]")
    f = np.zeros((H, W, 3), np.float32) if frame is None else np.array(frame, dtype=np.float32, order="C")
    c = np.zeros((H, W), np.uint32) if count is None else np.array(count, dtype=np.uint32, order="C")
    if f.shape != (H, W, 3) or c.shape != (H, W):
        raise ValueError("frame must be [H, W, 3] and count [H, W]")
    ts, tsp = _tiles(tile_list)
    ctx._check(lib().rt_render_budget(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), int(time_ms), tsp, C.c_void_p(b.ctypes.data),
                                      c.ctypes.data_as(C.POINTER(C.c_uint32)), f.ctypes.data_as(C.POINTER(C.c_float))))
    return f, c


def adaptive_plan_device(ctx, width, height, d_a, d_b, d_count, d_budget, d_tile_error, d_tile_active, params=None, stream=None):
    """The stopping rule on two half buffers (rt_adaptive_plan_device): device pointers to A, B (W*H*3 float32), the samples in each
    (W*H uint32) and the outputs - budget (W*H uint16), per tile the mean error (float32) and the active pixels (uint32)."""
    params = params or AdaptiveParams()
    ctx._check(lib().rt_adaptive_plan_device(ctx._h, int(width), int(height), _dptr(d_a), _dptr(d_b), _dptr(d_count), C.byref(params.c), _dptr(d_budget),
                                             _dptr(d_tile_error), _dptr(d_tile_active), _dptr(stream)))


def render_adaptive(ctx, scene, camera, render_data, time_ms, params=None):
    """The adaptive loop (rt_render_adaptive_host): a pilot, then passes that sample only where the two half buffers still disagree.
    Returns (frame [H, W, 3] float32, count [H, W] uint32 - the samples each pixel got, stats: passes, total_samples, active_tiles)."""
    params = params or AdaptiveParams()
    H, W = camera.height, camera.width
    frame = np.zeros((H, W, 3), np.float32)
    count = np.zeros((H, W), np.uint32)
    s = rt_adaptive_stats()
    ctx._check(lib().rt_render_adaptive_host(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), int(time_ms), C.byref(params.c),
                                             frame.ctypes.data_as(C.POINTER(C.c_float)), count.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(s)))
    return frame, count, _stats(s)
