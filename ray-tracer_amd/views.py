"""Camera sequences (include/rt_amd.h: rt_render_views, rt_render_views_device, rt_camera_lens): many views of a scene in one launch, as
separate frames or folded into one progressive frame - a turntable, a stereo pair, depth of field."""
import ctypes as C
import math

import numpy as np

from ._abi import VIEWS_MAX, _dptr, _times, lib, rt_camera  # noqa: F401  (VIEWS_MAX is a public name of this module)


def _cameras(cams, times_ms):
    cams = list(cams)
    if len(cams) != len(times_ms):
        raise ValueError("one time_ms per camera")
    arr = (rt_camera * max(len(cams), 1))()
    for i, c in enumerate(cams):
        arr[i] = c.c
    return arr, len(cams)


def render_views_device(ctx, scene, cams, render_data, times_ms, d_frames, accumulate=False, frame_num=0, stream=None):
    """Device-buffer form (rt_render_views_device): up to VIEWS_MAX views in ONE launch.  d_frames is a device pointer to len(cams) frames
    of W*H*3 float32 back to back (each what render_device gives for its camera and seed at frame_num 0) or, with accumulate, to one frame
    into which view i is folded as progressive frame frame_num + i.  Asynchronous on `stream`."""
    arr, n = _cameras(cams, times_ms)
    ctx._check(lib().rt_render_views_device(ctx._h, scene._h, arr, _times(times_ms), n, C.byref(render_data.c), int(bool(accumulate)), int(frame_num),
                                            _dptr(d_frames), _dptr(stream)))


def render_views(ctx, scene, cams, render_data, times_ms, accumulate=False, frame_num=0, frame=None):
    """Host-buffer form (rt_render_views): any number of views, VIEWS_MAX per launch.  Returns [n, H, W, 3] float32, one frame per camera,
    or with accumulate one [H, W, 3] frame: `frame` (the image after frame_num - 1; not changed) with the views folded in as progressive
    frames frame_num, frame_num + 1, ..."""
    arr, n = _cameras(cams, times_ms)
    if n < 1:
        raise ValueError("no cameras")
    H, W = arr[0].height, arr[0].width
    if accumulate:
        out = np.zeros((H, W, 3), np.float32) if frame is None else np.array(frame, dtype=np.float32, order="C")
        if out.shape != (H, W, 3):
            raise ValueError("frame must be [H, W, 3]")
    else:
        out = np.zeros((n, H, W, 3), np.float32)
    fn = C.c_int32(int(frame_num))
    ctx._check(lib().rt_render_views(ctx._h, scene._h, arr, _times(times_ms), n, C.byref(render_data.c), int(bool(accumulate)), C.byref(fn),
                                     out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def lens_offsets(aperture, n):
    """n points on a disc of radius `aperture` by the golden-angle spiral: r = aperture * sqrt((i + 0.5) / n), theta = i * 2.39996323.
    Deterministic (no random numbers); [n, 2] float32."""
    i = np.arange(int(n), dtype=np.float64)
    r = float(aperture) * np.sqrt((i + 0.5) / float(n))
    theta = i * 2.39996323
    return np.stack([r * np.cos(theta), r * np.sin(theta)], axis=1).astype(np.float32)


def lens_cameras(cam, focal_len, focus_dist, aperture, n):
    """n thin-lens samples of the pinhole camera `cam` (Camera.lens) at the offsets of lens_offsets: rendered with
    render_views(..., accumulate=True) they give one frame that is sharp at focus_dist and blurred elsewhere."""
    if n < 1 or not (aperture >= 0 and math.isfinite(aperture)):
        raise ValueError("n must be at least 1 and the aperture finite and not negative")
    return [cam.lens(focal_len, focus_dist, float(u), float(v)) for u, v in lens_offsets(aperture, n)]
