"""Environment lighting (include/rt_amd.h: rt_sky_create, rt_sky_texel_direction, rt_render_sky, rt_render_sky_device): a cube-map sky that
rays leaving the scene look their light up in, and the camera sequences rendered under it.  RenderData's sky colour is the map's tint."""
import ctypes as C

import numpy as np

from ._abi import SKY_MAX_FACE, _dptr, _times, lib  # noqa: F401  (SKY_MAX_FACE is a public name of this module)
from .objects import _Handle
from .views import _cameras


class Sky(_Handle):
    """A cube map on the context's GPU.  faces: [6, n, n, 3] float32 (a NumPy array or a CPU tensor), faces +X, -X, +Y, -Y, +Z, -Z, then
    rows, then columns; any value passes through, HDR, Inf and NaN included.  The map is copied: `faces` may change afterwards."""
    _destroy = "rt_sky_destroy"

    def __init__(self, ctx, faces):
        if hasattr(faces, "detach"):
            faces = faces.detach().cpu().numpy()
        faces = np.ascontiguousarray(faces, dtype=np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 3:
            raise ValueError("faces must be [6, n, n, 3]")
        self.ctx = ctx                      # (kept: the context outlives its skies)
        self.face_size = int(faces.shape[1])
        h = C.c_void_p()
        ctx._check(lib().rt_sky_create(ctx._h, self.face_size, faces.ctypes.data_as(C.POINTER(C.c_float)), C.byref(h)))
        self._h = h


def sky_texel_directions(n):
    """[6, n, n, 3] float32: the direction through the centre of every texel of an n-face map (rt_sky_texel_direction; not normalised).
    A map filled with f(direction) at these is looked up where f was evaluated."""
    n = int(n)
    if not 1 <= n <= SKY_MAX_FACE:
        raise ValueError("face size must be 1 .. SKY_MAX_FACE")
    c = ((np.arange(n, dtype=np.float32) + np.float32(0.5)) / np.float32(n)) * np.float32(2.0) - np.float32(1.0)
    t, s = np.meshgrid(c, c, indexing="ij")                  # rows carry t, columns s
    out = np.empty((6, n, n, 3), np.float32)
    for face in range(6):
        axis = face >> 1
        out[face, :, :, axis] = -1.0 if face & 1 else 1.0
        out[face, :, :, (axis + 1) % 3] = s
        out[face, :, :, (axis + 2) % 3] = t
    return out


def sky_from_equirect(image, n):
    """A cube map [6, n, n, 3] float32 from a latitude / longitude image [h, w, 3]: every texel takes the nearest source texel in its
    direction (float64; a convenience without a bit-exact definition).  Row 0 of the image is straight up (+Y), the columns go once round
    the Y axis starting at -Z."""
    image = np.asarray(image, np.float32)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("image must be [h, w, 3]")
    h, w = image.shape[:2]
    d = sky_texel_directions(n).astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    lat = np.arccos(np.clip(d[..., 1], -1.0, 1.0))                       # 0 at +Y, pi at -Y
    lon = np.arctan2(d[..., 0], -d[..., 2]) + np.pi                      # 0 .. 2 pi: -Z, -X, +Z, +X and round to -Z
    row = np.clip((lat / np.pi * h).astype(np.int64), 0, h - 1)
    col = np.clip((lon / (2.0 * np.pi) * w).astype(np.int64), 0, w - 1)
    return np.ascontiguousarray(image[row, col], np.float32)


def render_sky_device(ctx, scene, sky, cams, render_data, times_ms, d_frames, accumulate=False, frame_num=0, stream=None):
    """Device-buffer form (rt_render_sky_device): render_views_device under `sky`.  Asynchronous on `stream`."""
    arr, n = _cameras(cams, times_ms)
    ctx._check(lib().rt_render_sky_device(ctx._h, scene._h, sky._h, arr, _times(times_ms), n, C.byref(render_data.c), int(bool(accumulate)), int(frame_num),
                                          _dptr(d_frames), _dptr(stream)))


def render_sky(ctx, scene, sky, cams, render_data, times_ms, accumulate=False, frame_num=0, frame=None):
    """Host-buffer form (rt_render_sky): render_views under `sky`.  Returns [n, H, W, 3] float32 or, with accumulate, one [H, W, 3] frame."""
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
    ctx._check(lib().rt_render_sky(ctx._h, scene._h, sky._h, arr, _times(times_ms), n, C.byref(render_data.c), int(bool(accumulate)), C.byref(fn),
                                   out.ctypes.data_as(C.POINTER(C.c_float))))
    return out
