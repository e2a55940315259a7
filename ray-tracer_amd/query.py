"""Ray queries: closest hits and first-hit planes, occlusion (any-hit), the light-visibility plane and the ambient-occlusion plane."""
import ctypes as C

import numpy as np

from ._abi import AO_PLANES, AOV_PLANES, HIT_DTYPE, _dptr, _fp, _ray_arrays, lib


def trace_rays(ctx, scene, origins, directions):
    """The closest hit of every ray (rt_trace_rays): origins, directions [n, 3] float32, the direction taken as it is (not
    normalised; t is in units of its length).  Returns n records of HIT_DTYPE; a miss has object -1 and t HIT_MISS_T."""
    o, d = _ray_arrays(origins, directions)
    hits = np.zeros(o.shape[0], HIT_DTYPE)
    ctx._check(lib().rt_trace_rays(ctx._h, scene._h, _fp(o)[1], _fp(d)[1], o.shape[0], C.c_void_p(hits.ctypes.data)))
    return hits


def trace_rays_device(ctx, scene, d_origins, d_directions, n, d_hits, stream=None):
    """Device-buffer form (rt_trace_rays_device): device pointers (ints, e.g. torch.Tensor.data_ptr()) to n x 3 float32 origins and
    directions and to n records of HIT_DTYPE.itemsize bytes (16-byte aligned); asynchronous on `stream`."""
    ctx._check(lib().rt_trace_rays_device(ctx._h, scene._h, _dptr(d_origins), _dptr(d_directions), int(n), _dptr(d_hits), _dptr(stream)))


def render_aov(ctx, scene, camera, sky_colour=(0.0, 0.0, 0.0), planes=AOV_PLANES):
    """The first-hit planes of a view (rt_render_aov): a dict with the requested ones of depth [H, W], normal [H, W, 3],
    albedo [H, W, 3] (float32), object [H, W] (int32) and ray [H, W, 3] (the primary directions)."""
    unknown = [p for p in planes if p not in AOV_PLANES]
    if unknown:
        raise ValueError("unknown planes: %s" % unknown)
    W, H = camera.width, camera.height
    shapes = {"depth": (H, W), "normal": (H, W, 3), "albedo": (H, W, 3), "object": (H, W), "ray": (H, W, 3)}
    out = {p: np.zeros(shapes[p], np.int32 if p == "object" else np.float32) for p in AOV_PLANES if p in planes}
    sky = np.ascontiguousarray(sky_colour, dtype=np.float32)
    args = [out[p].ctypes.data_as(C.POINTER(C.c_int32 if p == "object" else C.c_float)) if p in out else None for p in AOV_PLANES]
    ctx._check(lib().rt_render_aov(ctx._h, scene._h, C.byref(camera.c), _fp(sky)[1], *args))
    return out


def render_aov_device(ctx, scene, camera, sky_colour=(0.0, 0.0, 0.0), d_depth=None, d_normal=None, d_albedo=None, d_object=None,
                      d_ray=None, stream=None):
    """Device-buffer form (rt_render_aov_device): device pointers to the wanted planes (None: not wanted); asynchronous on `stream`."""
    sky = np.ascontiguousarray(sky_colour, dtype=np.float32)
    ctx._check(lib().rt_render_aov_device(ctx._h, scene._h, C.byref(camera.c), _fp(sky)[1], *[_dptr(p) for p in (d_depth, d_normal, d_albedo, d_object, d_ray)],
                                          _dptr(stream)))


def occluded_rays(ctx, scene, origins, directions, tmax=None):
    """Is anything in the way (rt_occluded_rays)?  origins, directions [n, 3] float32, the direction taken as it is; tmax None ("any hit
    at all"), a scalar or n float32 limits in units of the direction's length.  Returns n uint8: 1 where the closest hit exists and lies
    at t <= tmax, else 0 (a NaN direction or a NaN limit: 0)."""
    o, d = _ray_arrays(origins, directions)
    n = o.shape[0]
    t = None
    if tmax is not None:
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
    out = np.zeros(n, np.uint8)
    ctx._check(lib().rt_occluded_rays(ctx._h, scene._h, _fp(o)[1], _fp(d)[1], _fp(t)[1] if t is not None else None, n, C.c_void_p(out.ctypes.data)))
    return out


def occluded_rays_device(ctx, scene, d_origins, d_directions, d_tmax, n, d_occluded, stream=None):
    """Device-buffer form (rt_occluded_rays_device): device pointers to n x 3 float32 origins and directions, n float32 limits (None: any
    hit at all) and n bytes of answers; asynchronous on `stream`."""
    ctx._check(lib().rt_occluded_rays_device(ctx._h, scene._h, _dptr(d_origins), _dptr(d_directions), _dptr(d_tmax), int(n), _dptr(d_occluded), _dptr(stream)))


def visible_between(ctx, scene, a, b, shrink=1e-4):
    """Line of sight between the points a[i] and b[i] ([n, 3]): True where nothing lies on the segment.  The ray is (a, b - a) with the
    difference formed in float32, the limit 1 - shrink, so that a surface b itself lies on does not count as a blocker."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
    d = (b - a).astype(np.float32)
    return occluded_rays(ctx, scene, a, d, np.float32(1.0) - np.float32(shrink)) == 0


def render_visibility(ctx, scene, camera, light_pos, bias=1e-3):
    """The light-visibility plane of a view (rt_render_visibility): [H, W] uint8 of VIS_BLOCKED, VIS_LIT, VIS_NO_SURFACE - per pixel the
    primary ray's closest hit, then the segment from P + N * bias to the point light."""
    out = np.zeros((camera.height, camera.width), np.uint8)
    light = np.ascontiguousarray(light_pos, dtype=np.float32).reshape(3)
    ctx._check(lib().rt_render_visibility(ctx._h, scene._h, C.byref(camera.c), _fp(light)[1], float(bias), C.c_void_p(out.ctypes.data)))
    return out


def render_visibility_device(ctx, scene, camera, light_pos, bias, d_visibility, stream=None):
    """Device-buffer form (rt_render_visibility_device): a device pointer to W * H bytes; asynchronous on `stream`."""
    light = np.ascontiguousarray(light_pos, dtype=np.float32).reshape(3)
    ctx._check(lib().rt_render_visibility_device(ctx._h, scene._h, C.byref(camera.c), _fp(light)[1], float(bias), _dptr(d_visibility), _dptr(stream)))


def render_ao(ctx, scene, camera, samples=16, radius=float("inf"), bias=1e-3, time_ms=0, planes=("ao",)):
    """The ambient-occlusion plane of a view (rt_render_ao): per pixel the primary ray's closest hit, then `samples` cosine-weighted
    directions of the renderer's sampler from P + N * bias on the pixel's own random stream (seeded like a frame of time_ms), each free
    if nothing lies within `radius`.  Returns a dict with the requested ones of ao [H, W] float32 (free samples / samples; 1 where
    there is no surface) and count [H, W] uint16 (the free samples; AO_NO_SURFACE where there is no surface)."""
    unknown = [p for p in planes if p not in AO_PLANES]
    if unknown:
        raise ValueError("unknown planes: %s" % unknown)
    W, H = camera.width, camera.height
    out = {p: np.zeros((H, W), np.uint16 if p == "count" else np.float32) for p in AO_PLANES if p in planes}
    count = C.c_void_p(out["count"].ctypes.data) if "count" in out else None
    ao = out["ao"].ctypes.data_as(C.POINTER(C.c_float)) if "ao" in out else None
    ctx._check(lib().rt_render_ao(ctx._h, scene._h, C.byref(camera.c), int(samples), float(radius), float(bias), int(time_ms), count, ao))
    return out


def render_ao_device(ctx, scene, camera, samples=16, radius=float("inf"), bias=1e-3, time_ms=0, d_count=None, d_ao=None, stream=None):
    """Device-buffer form (rt_render_ao_device): device pointers to W * H uint16 counts and W * H float32 (None: not wanted, but one of
    the two must be); asynchronous on `stream`."""
    ctx._check(lib().rt_render_ao_device(ctx._h, scene._h, C.byref(camera.c), int(samples), float(radius), float(bias), int(time_ms),
                                         _dptr(d_count), _dptr(d_ao), _dptr(stream)))
