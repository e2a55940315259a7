"""Several GPUs of one node from one host thread: tile ownership, the exchange step, and render() for a list of contexts."""
import ctypes as C

import numpy as np

from ._abi import RT_OK, _dptr, _host_frame, _times, _u32_backing, lib, rt_rank
from .render import _tile_spec


def partition_tiles(width, height, n_ranks, cost=None):
    """owner[ty * tiles_x + tx] = rank (rt_partition_tiles): interleaved without costs, longest-processing-time-first
    with them.  Returns an int32 array over the image's 8x8 tiles."""
    tiles_x, tiles_y = (int(width) + 7) // 8, (int(height) + 7) // 8
    owner = np.empty(tiles_x * tiles_y, np.int32)
    cp = None
    if cost is not None:
        cost = np.ascontiguousarray(cost, dtype=np.uint32)
        assert cost.size == owner.size
        cp = cost.ctypes.data_as(C.POINTER(C.c_uint32))
    st = lib().rt_partition_tiles(cp, tiles_x, tiles_y, int(n_ranks), owner.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != RT_OK:
        raise ValueError("rt_partition_tiles: bad argument")
    return owner


def tiles_copy_device(ctx, d_compact, d_frame, width, height, tile_list, to_frame=True, stream=None):
    """compact tile-list image <-> full frame on ctx's GPU (rt_tiles_copy_device)"""
    ids = np.ascontiguousarray(tile_list, dtype=np.uint32)
    backing = _u32_backing(ids)
    ctx._check(lib().rt_tiles_copy_device(ctx._h, C.c_void_p(d_compact), C.c_void_p(d_frame), int(width), int(height),
                                          backing.ctypes.data_as(C.POINTER(C.c_uint32)), int(ids.size), int(bool(to_frame)), _dptr(stream)))


def _ranks(ctxs, scenes):
    arr = (rt_rank * len(ctxs))()
    for i, (c, s) in enumerate(zip(ctxs, scenes)):
        arr[i].ctx, arr[i].scene = c._h, s._h
    return arr


def render_multi(ctxs, scenes, camera, render_data, data, times_ms):
    """render() for a node (rt_render_multi): rank i = (ctxs[i], scenes[i]) renders the bands b % n == i on its
    own GPU; the image lands in data.previous_render like render_frames on one GPU."""
    with _host_frame(data) as (fn, buf):
        ctxs[0]._check(lib().rt_render_multi(_ranks(ctxs, scenes), len(ctxs), C.byref(camera.c), C.byref(render_data.c), _times(times_ms), len(times_ms), fn, buf))
    return data.previous_render


def render_multi_device(ctxs, scenes, camera, render_data, times_ms, frame_num, d_frame, band_rows=0, stream=None):
    """device-buffer form (rt_render_multi_device): d_frame is a full frame on ctxs[0]'s GPU, updated in place.
    band_rows = 0: cost-balanced tile lists (the first call of a view measures the tiles); > 0: static bands"""
    ctxs[0]._check(lib().rt_render_multi_device(_ranks(ctxs, scenes), len(ctxs), C.byref(camera.c), C.byref(render_data.c), _times(times_ms), len(times_ms),
                                                int(frame_num), int(band_rows), C.c_void_p(d_frame), _dptr(stream)))


def gather(root, d_frame, width, height, src, d_bands, band_rows=8, band_first=0, band_stride=1, stream=None, tile_list=None):
    """the exchange step alone (rt_gather): src's compact buffer (bands, or the tiles of tile_list) -> the full frame on root's GPU"""
    ts = _tile_spec(band_rows, band_first, band_stride, True, tile_list, None)
    root._check(lib().rt_gather(root._h, C.c_void_p(d_frame), int(width), int(height), src._h, C.c_void_p(d_bands), C.byref(ts), _dptr(stream)))
