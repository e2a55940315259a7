"""Queries: closest hits and first-hit planes, multi-hit queries (the first k hits of a ray, hit counts), occlusion (any-hit), the
light-visibility plane, the ambient-occlusion plane, the nearest-surface queries (closest point and distance, which are no ray questions), and
the winding-number queries (point containment, the signed distance), the sphere-cast queries (where a moving ball first touches the scene), and
the box-overlap queries (which surfaces touch a box; a voxeliser), and the triangle-overlap queries (which surfaces a triangle cuts, and
along which segment; a mesh-scene collision test)."""
import ctypes as C

import numpy as np

from ._abi import AO_PLANES, AOV_PLANES, HIT_DTYPE, MULTIHIT_MAX, NEAREST_DTYPE, OVERLAP_ID_DTYPE, OVERLAP_MAX, SWEEP_DTYPE, TRI_SEGMENT_DTYPE, WINDING_BETA_DEFAULT, WINDING_SOLIDS, _dptr, _fp, _ray_arrays, lib


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


def _ray_limits(tmax, n):
    if tmax is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))


def trace_rays_multi(ctx, scene, origins, directions, k, tmax=None):
    """The first k hits of every ray in order along it (rt_trace_rays_multi): origins, directions [n, 3] float32, the direction taken as
    it is; k from 0 to MULTIHIT_MAX; tmax None, a scalar or n float32 limits in units of the direction's length.  Returns (hits, counts):
    hits [n, k] records of HIT_DTYPE, the ones behind a ray's last hit being misses (object -1, t HIT_MISS_T), and counts [n] int32, the
    records each ray has - with k == 0 the number of ALL its hits within the limit, and hits is empty."""
    o, d = _ray_arrays(origins, directions)
    n, k = o.shape[0], int(k)
    if not 0 <= k <= MULTIHIT_MAX:
        raise ValueError("k must be 0 .. %d" % MULTIHIT_MAX)
    lim = _ray_limits(tmax, n)
    hits = np.zeros((n, k), HIT_DTYPE)
    counts = np.zeros(n, np.int32)
    ctx._check(lib().rt_trace_rays_multi(ctx._h, scene._h, _fp(o)[1], _fp(d)[1], _fp(lim)[1] if lim is not None else None, n, k,
                                         C.c_void_p(hits.ctypes.data) if hits.size else None, counts.ctypes.data_as(C.POINTER(C.c_int32))))
    return hits, counts


def count_hits(ctx, scene, origins, directions, tmax=None):
    """How many surfaces every ray meets within its limit (trace_rays_multi in count-only mode): n int32.  Crossing counts, the number
    of surfaces between two points; a sphere counts once (its near root)."""
    return trace_rays_multi(ctx, scene, origins, directions, 0, tmax)[1]


def trace_rays_multi_device(ctx, scene, origins, directions, k, tmax=None, hits=None, counts=None, n=None, stream=None):
    """Device-buffer form (rt_trace_rays_multi_device), asynchronous on `stream` (a hipStream_t as an int; None: the default stream) and
    in the context's launch order.  origins, directions are float32 torch tensors of 3 n elements on the scene's GPU, tmax None or one of
    n, hits None or a uint8 tensor of n * k * 48 bytes, counts None or an int32 tensor of n - or all are device pointers as ints (hits and
    counts may be None where the entry point allows it) together with n.  With tensors returns (hits, counts): uint8 [n, k, 48]
    (`.cpu().numpy().view(HIT_DTYPE)[..., 0]` reads it; None with k == 0) and int32 [n], new ones where none were passed."""
    k = int(k)
    if isinstance(origins, int):
        if n is None:
            raise ValueError("device pointers need n, the number of rays")
        ctx._check(lib().rt_trace_rays_multi_device(ctx._h, scene._h, _dptr(origins), _dptr(directions), _dptr(tmax), int(n), k, _dptr(hits), _dptr(counts), _dptr(stream)))
        return hits, counts
    import torch
    o_ptr, count = _device_floats(origins, 3, "origins")
    d_ptr, n_d = _device_floats(directions, 3, "directions")
    if n_d != count or (n is not None and int(n) != count):
        raise ValueError("origins, directions and n differ")
    t_ptr = None
    if tmax is not None:
        t_ptr, n_t = _device_floats(tmax, 1, "tmax")
        if n_t != count:
            raise ValueError("tmax must hold one limit per ray")
    if not 0 <= k <= MULTIHIT_MAX:
        raise ValueError("k must be 0 .. %d" % MULTIHIT_MAX)
    if k == 0:
        hits = None
    elif hits is None:
        hits = torch.empty((count, k, HIT_DTYPE.itemsize), dtype=torch.uint8, device=origins.device)
    elif str(hits.dtype) != "torch.uint8" or not hits.is_contiguous() or not hits.is_cuda or hits.numel() != count * k * HIT_DTYPE.itemsize:
        raise ValueError("hits must be a contiguous uint8 tensor on the GPU of 48 bytes per record")
    if counts is None:
        counts = torch.empty((count,), dtype=torch.int32, device=origins.device)
    elif str(counts.dtype) != "torch.int32" or not counts.is_contiguous() or not counts.is_cuda or counts.numel() != count:
        raise ValueError("counts must be a contiguous int32 tensor on the GPU, one per ray")
    ctx._check(lib().rt_trace_rays_multi_device(ctx._h, scene._h, _dptr(o_ptr), _dptr(d_ptr), _dptr(t_ptr), count, k,
                                                _dptr(hits.data_ptr() if hits is not None else None), _dptr(counts.data_ptr()), _dptr(stream)))
    return hits, counts


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


NearestRecord = NEAREST_DTYPE       # rt_nearest as a structured dtype: distance, distance2, point[3], object, triangle, reserved


def _limits(max_dist, n):
    if max_dist is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, dtype=np.float32), (n,)))


def nearest_points(ctx, scene, points, max_dist=None):
    """The closest surface point of the scene for every point (rt_nearest_points): points [n, 3] float32; max_dist None (unbounded), a
    scalar or n float32 limits.  Returns n records of NearestRecord: the unsigned distance, its square, the closest point, the object and
    (for a triangle) the flattened triangle index; a miss - nothing within the limit, a limit that is NaN or negative, a point that is
    not finite - has object -1 and distance HIT_MISS_T."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    lim = _limits(max_dist, n)
    out = np.zeros(n, NEAREST_DTYPE)
    ctx._check(lib().rt_nearest_points(ctx._h, scene._h, _fp(p)[1], _fp(lim)[1] if lim is not None else None, n, C.c_void_p(out.ctypes.data)))
    return out


def _device_floats(t, per_item, what):
    """a contiguous float32 torch tensor on the GPU -> (pointer, items)"""
    if str(t.dtype) != "torch.float32" or not t.is_contiguous() or not t.is_cuda or t.numel() % per_item:
        raise ValueError("%s must be a contiguous float32 tensor on the GPU of %d floats per point" % (what, per_item))
    return t.data_ptr(), t.numel() // per_item


def nearest_points_device(ctx, scene, points, max_dist=None, out=None, n=None, stream=None):
    """Device-buffer form (rt_nearest_points_device), asynchronous on `stream` (a hipStream_t as an int; None: the default stream) and in
    the context's launch order.  `points` is a float32 torch tensor of 3 n elements on the scene's GPU, `max_dist` None or one of n, `out`
    None or a uint8 tensor of 32 n bytes - or all three are device pointers as ints together with n.  With tensors the records come back
    as a uint8 tensor [n, 32] (the one passed as `out`, or a new one): `.cpu().numpy().view(NearestRecord)` reads them."""
    if isinstance(points, int):
        if n is None or out is None:
            raise ValueError("device pointers need n, the number of points, and out")
        ctx._check(lib().rt_nearest_points_device(ctx._h, scene._h, _dptr(points), _dptr(max_dist), int(n), _dptr(out), _dptr(stream)))
        return out
    import torch
    ptr, count = _device_floats(points, 3, "points")
    if n is not None and int(n) != count:
        raise ValueError("n differs from the points given")
    lim_ptr = None
    if max_dist is not None:
        lim_ptr, n_lim = _device_floats(max_dist, 1, "max_dist")
        if n_lim != count:
            raise ValueError("max_dist must hold one limit per point")
    if out is None:
        out = torch.empty((count, NEAREST_DTYPE.itemsize), dtype=torch.uint8, device=points.device)
    elif str(out.dtype) != "torch.uint8" or not out.is_contiguous() or not out.is_cuda or out.numel() != count * NEAREST_DTYPE.itemsize:
        raise ValueError("out must be a contiguous uint8 tensor on the GPU of 32 bytes per point")
    ctx._check(lib().rt_nearest_points_device(ctx._h, scene._h, _dptr(ptr), _dptr(lim_ptr), count, _dptr(out.data_ptr()), _dptr(stream)))
    return out


def distance_grid(scene, lo, hi, shape, max_dist=None, stream=None):
    """The scene's unsigned distance field on a regular lattice: shape = (nx, ny, nz) points from corner lo to corner hi inclusive (a
    single point along an axis sits at lo), built with torch on the context's GPU and answered by nearest_points_device without a host
    round trip.  Returns (distance, records): a float32 tensor [nx, ny, nz] and the uint8 records [nx * ny * nz, 32], x slowest."""
    import torch
    ctx = scene.ctx
    dev = torch.device("cuda", ctx.device)
    axes = []
    for k in range(3):
        m = int(shape[k])
        if m < 1:
            raise ValueError("shape must be at least 1 along every axis")
        axes.append(torch.linspace(float(lo[k]), float(hi[k]), m, dtype=torch.float32, device=dev) if m > 1
                    else torch.full((1,), float(lo[k]), dtype=torch.float32, device=dev))
    gx, gy, gz = torch.meshgrid(axes[0], axes[1], axes[2], indexing="ij")
    pts = torch.stack((gx, gy, gz), dim=-1).reshape(-1, 3).contiguous()
    lim = None if max_dist is None else torch.full((pts.shape[0],), float(max_dist), dtype=torch.float32, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream      # the lattice was produced on it: the query is queued behind
    rec = nearest_points_device(ctx, scene, pts, lim, stream=stream)
    dist = rec.view(torch.float32).reshape(-1, 8)[:, 0].reshape(int(shape[0]), int(shape[1]), int(shape[2]))
    return dist, rec


def _lattice(scene, lo, hi, shape):
    """shape = (nx, ny, nz) points from corner lo to corner hi inclusive as a float32 tensor [nx * ny * nz, 3] on the scene's GPU, x slowest"""
    import torch
    dev = torch.device("cuda", scene.ctx.device)
    axes = []
    for k in range(3):
        m = int(shape[k])
        if m < 1:
            raise ValueError("shape must be at least 1 along every axis")
        axes.append(torch.linspace(float(lo[k]), float(hi[k]), m, dtype=torch.float32, device=dev) if m > 1
                    else torch.full((1,), float(lo[k]), dtype=torch.float32, device=dev))
    gx, gy, gz = torch.meshgrid(axes[0], axes[1], axes[2], indexing="ij")
    return torch.stack((gx, gy, gz), dim=-1).reshape(-1, 3).contiguous()


def winding_numbers(ctx, scene, points, object=WINDING_SOLIDS, inside=False):
    """The generalized winding number of every point (rt_winding_numbers): points [n, 3] float32; object an index of the scene's object list,
    or WINDING_SOLIDS for the sum over its spheres, cuboids and meshes.  Returns n float32 - 1 (or -1 for an inverted mesh) inside a closed
    surface, 0 outside, a fraction near a hole or for an open surface, NaN for a point that is not finite - and with inside=True the pair
    (winding, inside): inside n uint8, 1 where |w| >= 0.5."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    w = np.zeros(n, np.float32)
    flags = np.zeros(n, np.uint8) if inside else None
    ctx._check(lib().rt_winding_numbers(ctx._h, scene._h, _fp(p)[1], n, int(object), _fp(w)[1], C.c_void_p(flags.ctypes.data) if inside else None))
    return (w, flags) if inside else w


def contains_points(ctx, scene, points, object=WINDING_SOLIDS, beta=None):
    """Which points lie inside (rt_winding_numbers, the containment bytes alone): n bool, True where |w| >= 0.5.  beta None: the exact
    query; a number: the fast one (rt_winding_numbers_fast) with that beta."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    flags = np.zeros(p.shape[0], np.uint8)
    if beta is None:
        ctx._check(lib().rt_winding_numbers(ctx._h, scene._h, _fp(p)[1], p.shape[0], int(object), None, C.c_void_p(flags.ctypes.data)))
    else:
        ctx._check(lib().rt_winding_numbers_fast(ctx._h, scene._h, _fp(p)[1], p.shape[0], int(object), float(beta), None, C.c_void_p(flags.ctypes.data)))
    return flags.astype(bool)


def winding_numbers_fast(ctx, scene, points, object=WINDING_SOLIDS, beta=WINDING_BETA_DEFAULT, inside=False):
    """winding_numbers through the meshes' dipole cluster trees (rt_winding_numbers_fast): far clusters of triangles answer with their
    dipole, so the cost per point grows with the logarithm of a mesh's size and not with the size.  beta > 0 (inf allowed): the larger,
    the closer to the exact answer and the slower; the result is a defined function of the scene and beta.  Objects that are no meshes
    answer exactly.  Worth it on meshes of thousands of triangles; on a few hundred the exact query can be as quick."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    w = np.zeros(n, np.float32)
    flags = np.zeros(n, np.uint8) if inside else None
    ctx._check(lib().rt_winding_numbers_fast(ctx._h, scene._h, _fp(p)[1], n, int(object), float(beta), _fp(w)[1], C.c_void_p(flags.ctypes.data) if inside else None))
    return (w, flags) if inside else w


def winding_numbers_device(ctx, scene, points, object=WINDING_SOLIDS, winding=None, inside=None, n=None, stream=None):
    """Device-buffer form (rt_winding_numbers_device), asynchronous on `stream` (a hipStream_t as an int; None: the default stream) and in the
    context's launch order.  `points` is a float32 torch tensor of 3 n elements on the scene's GPU, `winding` None or a float32 tensor of
    n, `inside` None or a uint8 tensor of n: returns (winding, inside), with a new winding tensor where neither was passed.  Or all three
    are device pointers as ints (one of the outputs may be None) together with n."""
    return _winding_device(ctx, scene, points, object, None, winding, inside, n, stream)


def winding_numbers_fast_device(ctx, scene, points, object=WINDING_SOLIDS, beta=WINDING_BETA_DEFAULT, winding=None, inside=None, n=None, stream=None):
    """Device-buffer form of winding_numbers_fast (rt_winding_numbers_fast_device): the arguments of winding_numbers_device and beta.  The
    trees' moments are refitted on `stream` ahead of the query when the scene was updated since the last fast query."""
    return _winding_device(ctx, scene, points, object, float(beta), winding, inside, n, stream)


def _winding_device(ctx, scene, points, object, beta, winding, inside, n, stream):
    def call(p, count, w, f):
        if beta is None:
            ctx._check(lib().rt_winding_numbers_device(ctx._h, scene._h, _dptr(p), count, int(object), _dptr(w), _dptr(f), _dptr(stream)))
        else:
            ctx._check(lib().rt_winding_numbers_fast_device(ctx._h, scene._h, _dptr(p), count, int(object), beta, _dptr(w), _dptr(f), _dptr(stream)))
    if isinstance(points, int):
        if n is None:
            raise ValueError("device pointers need n, the number of points")
        call(points, int(n), winding, inside)
        return winding, inside
    import torch
    ptr, count = _device_floats(points, 3, "points")
    if n is not None and int(n) != count:
        raise ValueError("n differs from the points given")
    if winding is None and inside is None:
        winding = torch.empty((count,), dtype=torch.float32, device=points.device)
    if winding is not None and (str(winding.dtype) != "torch.float32" or not winding.is_contiguous() or not winding.is_cuda or winding.numel() != count):
        raise ValueError("winding must be a contiguous float32 tensor on the GPU, one per point")
    if inside is not None and (str(inside.dtype) != "torch.uint8" or not inside.is_contiguous() or not inside.is_cuda or inside.numel() != count):
        raise ValueError("inside must be a contiguous uint8 tensor on the GPU, one per point")
    call(ptr, count, winding.data_ptr() if winding is not None else None, inside.data_ptr() if inside is not None else None)
    return winding, inside


def signed_distance(ctx, scene, points, max_dist=None):
    """The signed distance of every point (rt_signed_distance): negative inside the scene's solids (|winding number| >= 0.5), positive
    outside; max_dist as for nearest_points.  Returns (sdf, records): n float32 and the n NearestRecord the magnitudes come from; a miss
    under a limit is -HIT_MISS_T or HIT_MISS_T."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    lim = _limits(max_dist, n)
    rec = np.zeros(n, NEAREST_DTYPE)
    sdf = np.zeros(n, np.float32)
    ctx._check(lib().rt_signed_distance(ctx._h, scene._h, _fp(p)[1], _fp(lim)[1] if lim is not None else None, n, C.c_void_p(rec.ctypes.data), _fp(sdf)[1]))
    return sdf, rec


def signed_distance_fast(ctx, scene, points, max_dist=None, beta=WINDING_BETA_DEFAULT):
    """signed_distance with the sign from the fast winding numbers (rt_signed_distance_fast): the records are the same, the sign is
    winding_numbers_fast's."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    lim = _limits(max_dist, n)
    rec = np.zeros(n, NEAREST_DTYPE)
    sdf = np.zeros(n, np.float32)
    ctx._check(lib().rt_signed_distance_fast(ctx._h, scene._h, _fp(p)[1], _fp(lim)[1] if lim is not None else None, n, float(beta), C.c_void_p(rec.ctypes.data),
                                             _fp(sdf)[1]))
    return sdf, rec


def signed_distance_fast_device(ctx, scene, points, max_dist=None, beta=WINDING_BETA_DEFAULT, sdf=None, records=None, n=None, stream=None):
    """Device-buffer form of signed_distance_fast (rt_signed_distance_fast_device): the arguments of signed_distance_device and beta."""
    return _signed_distance_device(ctx, scene, points, max_dist, float(beta), sdf, records, n, stream)


def signed_distance_device(ctx, scene, points, max_dist=None, sdf=None, records=None, n=None, stream=None):
    """Device-buffer form (rt_signed_distance_device), asynchronous on `stream` and in the context's launch order.  `points` is a float32 torch
    tensor of 3 n elements on the scene's GPU, `max_dist` None or one of n, `sdf` None or a float32 tensor of n, `records` None (the
    context keeps them) or a uint8 tensor of 32 n bytes: returns (sdf, records).  Or all are device pointers as ints together with n."""
    return _signed_distance_device(ctx, scene, points, max_dist, None, sdf, records, n, stream)


def _signed_distance_device(ctx, scene, points, max_dist, beta, sdf, records, n, stream):
    def call(p, lim, count, rec, out):
        if beta is None:
            ctx._check(lib().rt_signed_distance_device(ctx._h, scene._h, _dptr(p), _dptr(lim), count, _dptr(rec), _dptr(out), _dptr(stream)))
        else:
            ctx._check(lib().rt_signed_distance_fast_device(ctx._h, scene._h, _dptr(p), _dptr(lim), count, beta, _dptr(rec), _dptr(out), _dptr(stream)))
    if isinstance(points, int):
        if n is None or sdf is None:
            raise ValueError("device pointers need n, the number of points, and sdf")
        call(points, max_dist, int(n), records, sdf)
        return sdf, records
    import torch
    ptr, count = _device_floats(points, 3, "points")
    if n is not None and int(n) != count:
        raise ValueError("n differs from the points given")
    lim_ptr = None
    if max_dist is not None:
        lim_ptr, n_lim = _device_floats(max_dist, 1, "max_dist")
        if n_lim != count:
            raise ValueError("max_dist must hold one limit per point")
    if sdf is None:
        sdf = torch.empty((count,), dtype=torch.float32, device=points.device)
    elif str(sdf.dtype) != "torch.float32" or not sdf.is_contiguous() or not sdf.is_cuda or sdf.numel() != count:
        raise ValueError("sdf must be a contiguous float32 tensor on the GPU, one per point")
    if records is not None and (str(records.dtype) != "torch.uint8" or not records.is_contiguous() or not records.is_cuda or records.numel() != count * NEAREST_DTYPE.itemsize):
        raise ValueError("records must be a contiguous uint8 tensor on the GPU of 32 bytes per point")
    call(ptr, lim_ptr, count, records.data_ptr() if records is not None else None, sdf.data_ptr())
    return sdf, records


def signed_distance_grid(scene, lo, hi, shape, max_dist=None, stream=None, beta=None):
    """The scene's SIGNED distance field on distance_grid's lattice, answered by signed_distance_device without a host round trip.  Returns
    (sdf, records): a float32 tensor [nx, ny, nz], negative inside, and the uint8 records [nx * ny * nz, 32], x slowest.  beta None: the
    exact sign; a number: signed_distance_fast_device's with that beta."""
    import torch
    ctx = scene.ctx
    pts = _lattice(scene, lo, hi, shape)
    lim = None if max_dist is None else torch.full((pts.shape[0],), float(max_dist), dtype=torch.float32, device=pts.device)
    if stream is None:
        stream = torch.cuda.current_stream(pts.device).cuda_stream      # the lattice was produced on it: the query is queued behind
    rec = torch.empty((pts.shape[0], NEAREST_DTYPE.itemsize), dtype=torch.uint8, device=pts.device)
    sdf, _ = _signed_distance_device(ctx, scene, pts, lim, None if beta is None else float(beta), None, rec, None, stream)
    return sdf.reshape(int(shape[0]), int(shape[1]), int(shape[2])), rec


SweepRecord = SWEEP_DTYPE           # rt_sweep as a structured dtype: t, centre[3], point[3], object, triangle, feature, overlap, reserved


def sweep_spheres(ctx, scene, origins, directions, radius, tmax=None):
    """Where a ball of radius `radius` moving from origins[i] along directions[i] first touches the scene (rt_sweep_spheres): origins,
    directions [n, 3] float32, the direction taken as it is (not normalised; t is in units of its length); radius a scalar or n float32;
    tmax None, a scalar or n float32 limits on t.  Returns n records of SweepRecord: the time of first contact, the ball's centre then,
    the contact point, the object, the flattened triangle index and which feature of the triangle was touched (0 the face, 1..3 an edge,
    4..6 a vertex; -1 on a sphere); overlap 1 (with t 0) where the ball touches the scene already at the start.  A miss - nothing within
    the limit, or an input that is not finite, a zero direction, a negative radius - has object -1 and t HIT_MISS_T."""
    o, d = _ray_arrays(origins, directions)
    n = o.shape[0]
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (n,)))
    lim = _ray_limits(tmax, n)
    out = np.zeros(n, SWEEP_DTYPE)
    ctx._check(lib().rt_sweep_spheres(ctx._h, scene._h, _fp(o)[1], _fp(d)[1], _fp(r)[1], _fp(lim)[1] if lim is not None else None, n, C.c_void_p(out.ctypes.data)))
    return out


def sweep_spheres_device(ctx, scene, origins, directions, radius, tmax=None, out=None, n=None, stream=None):
    """Device-buffer form (rt_sweep_spheres_device), asynchronous on `stream` (a hipStream_t as an int; None with tensors: torch's
    current stream, which produced them; None with pointers: the default stream) and in the context's launch order.  origins, directions are float32 torch tensors of 3 n elements on the scene's GPU, radius a number or a
    tensor of n, tmax None, a number or a tensor of n, out None or a uint8 tensor of 48 n bytes - or all are device pointers as ints
    (tmax may be None) together with n.  With tensors the records come back as a uint8 tensor [n, 48] (the one passed as `out`, or a new
    one): `.cpu().numpy().view(SweepRecord)` reads them."""
    if isinstance(origins, int):
        if n is None or out is None:
            raise ValueError("device pointers need n, the number of balls, and out")
        ctx._check(lib().rt_sweep_spheres_device(ctx._h, scene._h, _dptr(origins), _dptr(directions), _dptr(radius), _dptr(tmax), int(n), _dptr(out), _dptr(stream)))
        return out
    import torch
    o_ptr, count = _device_floats(origins, 3, "origins")
    d_ptr, n_d = _device_floats(directions, 3, "directions")
    if n_d != count or (n is not None and int(n) != count):
        raise ValueError("origins, directions and n differ")

    # the stream the kernels are queued on: the one given, else torch's current stream (what produced the tensors), never the null stream
    # behind torch's back - a number is broadcast on that stream, so that the fill is ordered ahead of the kernels
    if stream is None:
        stream = torch.cuda.current_stream(origins.device).cuda_stream
    queue = torch.cuda.ExternalStream(int(stream), device=origins.device) if int(stream) else torch.cuda.default_stream(origins.device)

    def per_ball(x, what):
        if not torch.is_tensor(x):
            with torch.cuda.stream(queue):
                x = torch.full((count,), float(x), dtype=torch.float32, device=origins.device)
            x.record_stream(queue)
        ptr, m = _device_floats(x, 1, what)
        if m != count:
            raise ValueError("%s must hold one value per ball" % what)
        return x, ptr
    radius, r_ptr = per_ball(radius, "radius")
    t_ptr = None
    if tmax is not None:
        tmax, t_ptr = per_ball(tmax, "tmax")
    if out is None:
        out = torch.empty((count, SWEEP_DTYPE.itemsize), dtype=torch.uint8, device=origins.device)
    elif str(out.dtype) != "torch.uint8" or not out.is_contiguous() or not out.is_cuda or out.numel() != count * SWEEP_DTYPE.itemsize:
        raise ValueError("out must be a contiguous uint8 tensor on the GPU of 48 bytes per ball")
    ctx._check(lib().rt_sweep_spheres_device(ctx._h, scene._h, _dptr(o_ptr), _dptr(d_ptr), _dptr(r_ptr), _dptr(t_ptr), count, _dptr(out.data_ptr()), _dptr(stream)))
    return out


def sweep_grid(scene, lo, hi, shape, direction, radius, tmax=None, stream=None):
    """A ball of `radius` sent along `direction` from every point of distance_grid's lattice (shape = (nx, ny, nz) points from corner lo
    to corner hi inclusive), built with torch on the context's GPU and answered by sweep_spheres_device without a host round trip: with
    a flat lattice above a part and the direction straight down, the rest heights of the ball - the dilated height field a ball-nose tool
    path or a "place on surface" uses.  Returns (t, records): a float32 tensor [nx, ny, nz] (HIT_MISS_T where the ball meets nothing) and
    the uint8 records [nx * ny * nz, 48], x slowest."""
    import torch
    ctx = scene.ctx
    pts = _lattice(scene, lo, hi, shape)
    dirs = torch.tensor([float(direction[0]), float(direction[1]), float(direction[2])], dtype=torch.float32, device=pts.device).repeat(pts.shape[0], 1).contiguous()
    if stream is None:
        stream = torch.cuda.current_stream(pts.device).cuda_stream      # the lattice was produced on it: the query is queued behind
    rec = sweep_spheres_device(ctx, scene, pts, dirs, radius, tmax, stream=stream)
    t = rec.view(torch.float32).reshape(-1, 12)[:, 0].reshape(int(shape[0]), int(shape[1]), int(shape[2]))
    return t, rec


OverlapId = OVERLAP_ID_DTYPE        # rt_overlap_id as a structured dtype: object, triangle ({-1, -1}: no candidate at this rank)


def _box_arrays(lo, hi):
    lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(-1, 3)
    if lo.shape != hi.shape:
        raise ValueError("lo and hi must hold n x 3 floats each")
    return lo, hi


def overlap_boxes(scene, lo, hi, k=0):
    """Which surfaces touch every axis-aligned, closed box (rt_overlap_boxes): lo, hi [n, 3] float32; k from 0 to OVERLAP_MAX.  Returns
    (counts, ids): counts [n] int32, the number of ALL surfaces - spheres and triangle records - that overlap the box, and ids [n, k]
    records of OverlapId, the k of them lowest in (object, triangle) order, {-1, -1} behind a box's last.  A box with a component that is
    not finite or with lo > hi on an axis overlaps nothing.  A sphere is a surface: a box wholly inside it does not touch it."""
    ctx = scene.ctx
    lo, hi = _box_arrays(lo, hi)
    n, k = lo.shape[0], int(k)
    if not 0 <= k <= OVERLAP_MAX:
        raise ValueError("k must be 0 .. %d" % OVERLAP_MAX)
    ids = np.zeros((n, k), OVERLAP_ID_DTYPE)
    counts = np.zeros(n, np.int32)
    ctx._check(lib().rt_overlap_boxes(ctx._h, scene._h, _fp(lo)[1], _fp(hi)[1], n, k, C.c_void_p(ids.ctypes.data) if ids.size else None,
                                      counts.ctypes.data_as(C.POINTER(C.c_int32)), None))
    return counts, ids


def boxes_touch(scene, lo, hi):
    """Whether any surface touches every box (rt_overlap_boxes in any-only mode: a box stops at its first overlapping surface): n bool."""
    ctx = scene.ctx
    lo, hi = _box_arrays(lo, hi)
    flags = np.zeros(lo.shape[0], np.uint8)
    ctx._check(lib().rt_overlap_boxes(ctx._h, scene._h, _fp(lo)[1], _fp(hi)[1], lo.shape[0], 0, None, None, C.c_void_p(flags.ctypes.data)))
    return flags.astype(bool)


def overlap_boxes_device(scene, lo, hi, k=0, ids=None, counts=None, any=None, n=None, stream=None):
    """Device-buffer form (rt_overlap_boxes_device), asynchronous on `stream` (a hipStream_t as an int; None: the default stream) and in
    the context's launch order.  lo, hi are float32 torch tensors of 3 n elements on the scene's GPU; ids None or a uint8 tensor of
    n * k * 8 bytes, counts None or an int32 tensor of n, any None or a uint8 tensor of n - or all are device pointers as ints (outputs
    may be None where the entry point allows it) together with n.  With tensors returns (counts, ids, any): new counts where none of the
    three was passed, and new ids [n, k, 8] for k > 0 where none were (`.cpu().numpy().view(OverlapId)[..., 0]` reads them); with k == 0, no counts and
    `any` given the query runs in any-only mode."""
    ctx = scene.ctx
    k = int(k)
    if isinstance(lo, int):
        if n is None:
            raise ValueError("device pointers need n, the number of boxes")
        ctx._check(lib().rt_overlap_boxes_device(ctx._h, scene._h, _dptr(lo), _dptr(hi), int(n), k, _dptr(ids), _dptr(counts), _dptr(any), _dptr(stream)))
        return counts, ids, any
    import torch
    lo_ptr, count = _device_floats(lo, 3, "lo")
    hi_ptr, n_hi = _device_floats(hi, 3, "hi")
    if n_hi != count or (n is not None and int(n) != count):
        raise ValueError("lo, hi and n differ")
    if not 0 <= k <= OVERLAP_MAX:
        raise ValueError("k must be 0 .. %d" % OVERLAP_MAX)
    none_given = ids is None and counts is None and any is None
    if k == 0:
        ids = None
    elif ids is None:
        ids = torch.empty((count, k, OVERLAP_ID_DTYPE.itemsize), dtype=torch.uint8, device=lo.device)
    elif str(ids.dtype) != "torch.uint8" or not ids.is_contiguous() or not ids.is_cuda or ids.numel() != count * k * OVERLAP_ID_DTYPE.itemsize:
        raise ValueError("ids must be a contiguous uint8 tensor on the GPU of 8 bytes per id")
    if none_given or (counts is None and any is None and k == 0):
        counts = torch.empty((count,), dtype=torch.int32, device=lo.device)
    if counts is not None and (str(counts.dtype) != "torch.int32" or not counts.is_contiguous() or not counts.is_cuda or counts.numel() != count):
        raise ValueError("counts must be a contiguous int32 tensor on the GPU, one per box")
    if any is not None and (str(any.dtype) != "torch.uint8" or not any.is_contiguous() or not any.is_cuda or any.numel() != count):
        raise ValueError("any must be a contiguous uint8 tensor on the GPU, one per box")
    ctx._check(lib().rt_overlap_boxes_device(ctx._h, scene._h, _dptr(lo_ptr), _dptr(hi_ptr), count, k, _dptr(ids.data_ptr() if ids is not None else None),
                                             _dptr(counts.data_ptr() if counts is not None else None), _dptr(any.data_ptr() if any is not None else None), _dptr(stream)))
    return counts, ids, any


def voxel_boxes(lo, hi, shape):
    """The cells of voxelize as boxes: shape = (nx, ny, nz) cells between corner lo and corner hi, cell i of an axis from edge i to edge
    i + 1 of its nx + 1 edges (lo + (hi - lo) * i / nx in binary64, rounded to float32 once; the last edge is hi), so that neighbours
    share a face exactly.  Returns (cell_lo, cell_hi, centre): float32 arrays [nx * ny * nz, 3], x slowest as in distance_grid; a centre
    is (lo + hi) * 0.5 per component."""
    edges = []
    for a in range(3):
        m = int(shape[a])
        if m < 1:
            raise ValueError("shape must be at least 1 along every axis")
        e = (float(lo[a]) + (float(hi[a]) - float(lo[a])) * np.arange(m + 1, dtype=np.float64) / m).astype(np.float32)
        e[m] = np.float32(hi[a])
        edges.append(e)
    cell_lo = np.stack(np.meshgrid(*[e[:-1] for e in edges], indexing="ij"), axis=-1).reshape(-1, 3)
    cell_hi = np.stack(np.meshgrid(*[e[1:] for e in edges], indexing="ij"), axis=-1).reshape(-1, 3)
    centre = (cell_lo + cell_hi) * np.float32(0.5)
    return np.ascontiguousarray(cell_lo), np.ascontiguousarray(cell_hi), np.ascontiguousarray(centre)


def voxelize(scene, lo, hi, shape, solid=False, beta=None):
    """The scene as voxels: shape = (nx, ny, nz) cells between corner lo and corner hi (voxel_boxes; distance_grid's axis order, x
    slowest).  A cell is set where a surface touches its closed box (overlap_boxes_device in any-only mode) and, with solid=True, also
    where its centre lies inside (contains_points' rule, |w| >= 0.5 over the spheres, cuboids and meshes; beta None: the exact winding
    numbers, a number: the fast ones with that beta).  The cell boxes are built with NumPy on the host (voxel_boxes) and uploaded, which
    is most of the call's time on a large grid; the queries run on the context's GPU, queued behind the upload on torch's current stream.
    The cells are CELLS between nx + 1 edges per axis, not distance_grid's lattice of points that includes both corners: only the axis
    order is shared.  Returns a bool tensor [nx, ny, nz]."""
    import torch
    ctx = scene.ctx
    dev = torch.device("cuda", ctx.device)
    cell_lo, cell_hi, centre = voxel_boxes(lo, hi, shape)
    stream = torch.cuda.current_stream(dev).cuda_stream      # the boxes are produced on it: the queries are queued behind
    d_lo, d_hi = torch.from_numpy(cell_lo).to(dev), torch.from_numpy(cell_hi).to(dev)
    flags = torch.empty((cell_lo.shape[0],), dtype=torch.uint8, device=dev)
    overlap_boxes_device(scene, d_lo, d_hi, 0, any=flags, stream=stream)
    cells = flags != 0
    if solid:
        inside = torch.empty_like(flags)
        _winding_device(ctx, scene, torch.from_numpy(centre).to(dev), WINDING_SOLIDS, None if beta is None else float(beta), None, inside, None, stream)
        cells = cells | (inside != 0)
    return cells.reshape(int(shape[0]), int(shape[1]), int(shape[2]))


TriSegment = TRI_SEGMENT_DTYPE      # rt_tri_segment as a structured dtype: p[3], q[3], kind (0 empty, 1 a segment, 2 a pair without one), reserved


def _tri_array(triangles):
    t = np.ascontiguousarray(triangles, dtype=np.float32)
    if t.size % 9:
        raise ValueError("triangles must hold n x 9 floats: a0, a1, a2")
    return t.reshape(-1, 9)


def overlap_triangles(scene, triangles, k=0, segments=False):
    """Which surfaces every query triangle cuts (rt_overlap_triangles): triangles [n, 3, 3] or [n, 9] float32, the vertices a0, a1, a2;
    k from 0 to OVERLAP_MAX.  Returns (counts, ids), and with segments=True (counts, ids, segs): counts [n] int32, the number of ALL
    surfaces - spheres and triangle records - that overlap the triangle; ids [n, k] records of OverlapId, the k of them lowest in
    (object, triangle) order, {-1, -1} behind a query's last; segs [n, k] records of TriSegment, the segment each pair of ids shares
    (kind 1), kind 2 for a sphere or a coplanar pair, kind 0 in an empty slot.  A triangle with a component that is not finite overlaps
    nothing.  segments=True needs k > 0."""
    ctx = scene.ctx
    t = _tri_array(triangles)
    n, k = t.shape[0], int(k)
    if not 0 <= k <= OVERLAP_MAX:
        raise ValueError("k must be 0 .. %d" % OVERLAP_MAX)
    if segments and k == 0:
        raise ValueError("segments need k > 0")
    ids = np.zeros((n, k), OVERLAP_ID_DTYPE)
    counts = np.zeros(n, np.int32)
    segs = np.zeros((n, k), TRI_SEGMENT_DTYPE) if segments else None
    ctx._check(lib().rt_overlap_triangles(ctx._h, scene._h, _fp(t)[1], n, k, C.c_void_p(ids.ctypes.data) if ids.size else None,
                                          counts.ctypes.data_as(C.POINTER(C.c_int32)), None,
                                          C.c_void_p(segs.ctypes.data) if segments and segs.size else None))
    return (counts, ids, segs) if segments else (counts, ids)


def triangles_touch(scene, triangles):
    """Whether every query triangle cuts any surface (rt_overlap_triangles in any-only mode: a query stops at its first): n bool."""
    ctx = scene.ctx
    t = _tri_array(triangles)
    flags = np.zeros(t.shape[0], np.uint8)
    ctx._check(lib().rt_overlap_triangles(ctx._h, scene._h, _fp(t)[1], t.shape[0], 0, None, None, C.c_void_p(flags.ctypes.data), None))
    return flags.astype(bool)


def overlap_triangles_device(scene, triangles, k=0, ids=None, counts=None, any=None, segments=None, n=None, stream=None):
    """Device-buffer form (rt_overlap_triangles_device), asynchronous on `stream` (a hipStream_t as an int; None: the default stream) and
    in the context's launch order.  triangles is a float32 torch tensor of 9 n elements on the scene's GPU; ids None or a uint8 tensor of
    n * k * 8 bytes, counts None or an int32 tensor of n, any None or a uint8 tensor of n, segments None, True (a new tensor) or a uint8
    tensor of n * k * 32 bytes - or all are device pointers as ints (outputs may be None where the entry point allows it) together with
    n.  With tensors returns (counts, ids, any, segments): new counts where none of ids, counts and any was passed, new ids [n, k, 8] for
    k > 0 where none were, new segments [n, k, 32] for segments=True (`.cpu().numpy().view(TriSegment)[..., 0]` reads them); with k == 0,
    no counts and `any` given the query runs in any-only mode."""
    ctx = scene.ctx
    k = int(k)
    if isinstance(triangles, int):
        if n is None:
            raise ValueError("device pointers need n, the number of triangles")
        ctx._check(lib().rt_overlap_triangles_device(ctx._h, scene._h, _dptr(triangles), int(n), k, _dptr(ids), _dptr(counts), _dptr(any), _dptr(segments), _dptr(stream)))
        return counts, ids, any, segments
    import torch
    t_ptr, count = _device_floats(triangles, 9, "triangles")
    if n is not None and int(n) != count:
        raise ValueError("triangles and n differ")
    if not 0 <= k <= OVERLAP_MAX:
        raise ValueError("k must be 0 .. %d" % OVERLAP_MAX)
    none_given = ids is None and counts is None and any is None
    if k == 0:
        ids = None
    elif ids is None:
        ids = torch.empty((count, k, OVERLAP_ID_DTYPE.itemsize), dtype=torch.uint8, device=triangles.device)
    elif str(ids.dtype) != "torch.uint8" or not ids.is_contiguous() or not ids.is_cuda or ids.numel() != count * k * OVERLAP_ID_DTYPE.itemsize:
        raise ValueError("ids must be a contiguous uint8 tensor on the GPU of 8 bytes per id")
    if segments is False:
        segments = None
    if segments is not None and k == 0:
        raise ValueError("segments need k > 0")
    if segments is True:
        segments = torch.empty((count, k, TRI_SEGMENT_DTYPE.itemsize), dtype=torch.uint8, device=triangles.device)
    elif segments is not None and (str(segments.dtype) != "torch.uint8" or not segments.is_contiguous() or not segments.is_cuda
                                   or segments.numel() != count * k * TRI_SEGMENT_DTYPE.itemsize):
        raise ValueError("segments must be a contiguous uint8 tensor on the GPU of 32 bytes per segment")
    if none_given or (counts is None and any is None and k == 0):
        counts = torch.empty((count,), dtype=torch.int32, device=triangles.device)
    if counts is not None and (str(counts.dtype) != "torch.int32" or not counts.is_contiguous() or not counts.is_cuda or counts.numel() != count):
        raise ValueError("counts must be a contiguous int32 tensor on the GPU, one per triangle")
    if any is not None and (str(any.dtype) != "torch.uint8" or not any.is_contiguous() or not any.is_cuda or any.numel() != count):
        raise ValueError("any must be a contiguous uint8 tensor on the GPU, one per triangle")
    ptr = lambda x: _dptr(x.data_ptr() if x is not None else None)
    ctx._check(lib().rt_overlap_triangles_device(ctx._h, scene._h, _dptr(t_ptr), count, k, ptr(ids), ptr(counts), ptr(any), ptr(segments), _dptr(stream)))
    return counts, ids, any, segments


def collide_mesh(scene, triangles, k=OVERLAP_MAX):
    """A mesh against the scene: every triangle of `triangles` [n, 3, 3] asked with k ids and segments (overlap_triangles), the pairs
    returned as flat arrays.  Returns a dict: query [m] (the index into `triangles`), object [m], triangle [m] (-1: a sphere), p [m, 3],
    q [m, 3], kind [m] (1: a segment from p to q - together the intersection curve; 2: a sphere or a coplanar pair, p and q NaN), counts
    [n] and truncated [n] bool, true where a triangle cuts more than k surfaces and the pairs hold only its k lowest."""
    k = int(k)
    if not 1 <= k <= OVERLAP_MAX:
        raise ValueError("k must be 1 .. %d" % OVERLAP_MAX)
    counts, ids, segs = overlap_triangles(scene, triangles, k, segments=True)
    held = ids["object"] >= 0
    query = np.broadcast_to(np.arange(ids.shape[0], dtype=np.int64)[:, None], ids.shape)[held]
    return {"query": query, "object": ids["object"][held], "triangle": ids["triangle"][held], "p": segs["p"][held], "q": segs["q"][held],
            "kind": segs["kind"][held], "counts": counts, "truncated": counts > k}
