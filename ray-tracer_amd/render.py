"""Rendering on one GPU: the reference's per-frame call, its device-buffer and multi-frame forms, the frames-in-flight pipeline,
and what goes with a frame (display conversion, PNG, the device-side test hooks)."""
import ctypes as C

import numpy as np

from ._abi import _dptr, _host_frame, _times, _u32_backing, lib, rt_tile_spec


def render(ctx, scene, camera, render_data, data, current_time_ms):
    """reference render(VariableRenderData*, int) src/dispatch.cu:156-163: reads
    data.previous_render, overwrites it with the new progressive average, increments
    data.frame_num."""
    with _host_frame(data) as (fn, buf):
        ctx._check(lib().rt_render(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), int(current_time_ms), fn, buf))
    return data.previous_render


def render_frames(ctx, scene, camera, render_data, data, times_ms):
    """len(times_ms) consecutive passes of the reference's main loop body (src/main.cu:421-424) in
    one call: the same image as that many render() calls, rendered by multi-frame launches."""
    with _host_frame(data) as (fn, buf):
        ctx._check(lib().rt_render_frames(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), _times(times_ms), len(times_ms), fn, buf))
    return data.previous_render


def _tile_spec(band_rows, band_first, band_stride, compact, tile_list, tile_cost, tile_peak=None):
    """rt_tile_spec; it holds on to the arrays it points at (ts.arrays), so they live as long as it does"""
    ts = rt_tile_spec(int(band_rows), int(band_first), int(band_stride), int(bool(compact)))
    if tile_list is not None:
        ids = np.ascontiguousarray(tile_list, dtype=np.uint32)
        backing = _u32_backing(ids)
        ts.tile_list = backing.ctypes.data_as(C.POINTER(C.c_uint32))
        ts.num_tiles = int(ids.size)
        cost = None
        if tile_cost is not None:
            cost = np.ascontiguousarray(tile_cost, dtype=np.uint32)
            assert cost.size == ids.size
            if cost.size:
                ts.tile_cost = cost.ctypes.data_as(C.POINTER(C.c_uint32))
        peak = None
        if tile_peak is not None and cost is not None:
            peak = np.ascontiguousarray(tile_peak, dtype=np.uint32)
            assert peak.size == ids.size
            if peak.size:
                ts.tile_peak = peak.ctypes.data_as(C.POINTER(C.c_uint32))
        ts.arrays = (ids, backing, cost, peak)
    return ts


def render_device(ctx, scene, camera, render_data, time_ms, frame_num, d_out, d_prev=None,
                  band_rows=8, band_first=0, band_stride=1, compact=False, stream=None, tile_list=None, tile_cost=None, tile_peak=None):
    """Device-buffer form: d_out / d_prev are device pointers (ints, e.g. torch.Tensor.data_ptr()).  tile_list: the
    8x8 tiles to render (indices ty * ceil(W / 8) + tx) instead of bands."""
    ts = _tile_spec(band_rows, band_first, band_stride, compact, tile_list, tile_cost, tile_peak)
    ctx._check(lib().rt_render_device(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), int(time_ms), int(frame_num),
                                      C.byref(ts), _dptr(d_prev), C.c_void_p(d_out), _dptr(stream)))


def render_device_batch(ctx, scene, camera, render_data, times_ms, frame_num, d_frame,
                        band_rows=8, band_first=0, band_stride=1, compact=False, stream=None, tile_list=None, tile_cost=None, tile_peak=None):
    """len(times_ms) consecutive progressive frames in ONE launch, accumulated in place in the device
    buffer d_frame (bit-identical to that many render_device calls; see rt_render_device_batch)."""
    ts = _tile_spec(band_rows, band_first, band_stride, compact, tile_list, tile_cost, tile_peak)
    ctx._check(lib().rt_render_device_batch(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), _times(times_ms), len(times_ms), int(frame_num),
                                            C.byref(ts), C.c_void_p(d_frame), _dptr(stream)))


PIPELINE_DEPTH = 8          # RT_PIPELINE_DEPTH (include/rt_amd.h): at most
PIPELINE_DEFAULT_DEPTH = 4


def frame_depth(ctx, depth):
    """how many frames the caller keeps in flight: each is launched on 1 / depth of the CUs (rt_frame_depth)"""
    ctx._check(lib().rt_frame_depth(ctx._h, int(depth)))


def frame_submit(ctx, scene, camera, render_data, time_ms,
                 band_rows=8, band_first=0, band_stride=1, compact=False, tile_list=None, tile_cost=None, tile_peak=None):
    """Queue one frame seeded with time_ms on a stream of the context's own; up to PIPELINE_DEPTH may be submitted and not
    collected (rt_frame_submit).  Frames in flight overlap on the GPU."""
    ts = _tile_spec(band_rows, band_first, band_stride, compact, tile_list, tile_cost, tile_peak)
    ctx._check(lib().rt_frame_submit(ctx._h, scene._h, C.byref(camera.c), C.byref(render_data.c), int(time_ms), C.byref(ts)))


def frame_collect(ctx, frame_num, d_frame, stream=None):
    """Fold the oldest submitted frame into the device buffer d_frame as progressive frame frame_num, asynchronously on
    `stream` (rt_frame_collect).  d_frame None: discard the frame."""
    ctx._check(lib().rt_frame_collect(ctx._h, int(frame_num), _dptr(d_frame), _dptr(stream)))


def frame_collect_host(ctx, data):
    """the oldest submitted (whole) frame into data.previous_render, data.frame_num += 1 (rt_frame_collect_host); data None: discard"""
    if data is None:
        ctx._check(lib().rt_frame_collect_host(ctx._h, C.byref(C.c_int32(0)), None))
        return
    with _host_frame(data) as (fn, buf):
        ctx._check(lib().rt_frame_collect_host(ctx._h, fn, buf))


def frame_wait(ctx):
    """block until the frame collected last is in its d_frame (rt_frame_wait)"""
    ctx._check(lib().rt_frame_wait(ctx._h))


def frames_pending(ctx):
    return int(lib().rt_frames_pending(ctx._h))


def tile_owned_rows(height, band_rows=8, band_first=0, band_stride=1):
    ts = rt_tile_spec(int(band_rows), int(band_first), int(band_stride), 0)
    return lib().rt_tile_owned_rows(C.byref(ts), int(height))


def to_rgba8_device(ctx, d_rgb, width, height, d_rgba, stream=None):
    """float -> RGBA8 of src/main.cu:343-371 on the device."""
    ctx._check(lib().rt_to_rgba8_device(ctx._h, C.c_void_p(d_rgb), int(width), int(height), C.c_void_p(d_rgba), _dptr(stream)))


def save_png(path, image):
    """Writes a frame as an 8-bit RGB PNG (the format of the reference's images/*.png).  `image`
    is [H, W, 3|4] uint8, or a float frame, which is converted like the reference's display path
    (src/main.cu:343-371: int(px * 255), clamped)."""
    import struct
    import zlib
    img = np.asarray(image)
    if img.dtype != np.uint8:
        img = np.clip((img.astype(np.float32) * np.float32(255)).astype(np.int64), 0, 255).astype(np.uint8)
    img = np.ascontiguousarray(img[:, :, :3])
    h, w = img.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def debug_eval(ctx, op, bits):
    """device-side evaluation of a math / RNG header function on uint32 bit patterns (tests)"""
    a = np.ascontiguousarray(bits, dtype=np.uint32)
    out = np.empty_like(a)
    ctx._check(lib().rt_debug_eval(ctx._h, int(op), a.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))
    return out


def debug_exhaustive(ctx):
    """(differing, in range) for the device code's short reciprocal, then for its short square root, over all 2^32 inputs"""
    out = (C.c_uint64 * 4)()
    ctx._check(lib().rt_debug_exhaustive(ctx._h, out))
    return tuple(int(x) for x in out)
