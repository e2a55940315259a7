"""The yardstick of the ambient-occlusion plane (rt_render_ao, include/rt_amd.h): the definition restated in plain Python / NumPy float32
over the CPU oracle - orc_trace_one (what orc.Scene.trace_one calls) for every segment, orc_normal_next (det math) for every draw,
test_gpu_query.primaries for the primary rays.  No product code.  Every operation is rounded to binary32 once, in the header's order;
nothing is fused."""
import ctypes as C

import numpy as np

from test_gpu_query import primaries

F = np.float32
NO_SURFACE = 0xFFFF
WHITE = ("standard", (1, 1, 1), 0)


def _dot(a, b):
    """rows of [n, 3]: (x*x' + y*y') + z*z', every operation rounded to binary32"""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalised(a):
    """rows of [n, 3]: a * (1.0f / sqrtf((x*x + y*y) + z*z))"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(_dot(a, a))
        return a * inv[:, None]


def seed_of(px, py, W, time_ms):
    """state = (uint32)((py * W + px) * 3) * 3145739u + (uint32)time_ms * 6291469u"""
    return ((((py * W + px) * 3) & 0xFFFFFFFF) * 3145739 + (time_ms & 0xFFFFFFFF) * 6291469) & 0xFFFFFFFF


def _oracle_calls(orc):
    """orc_trace_one and orc_normal_next of the oracle's library (orc.lib()) taking plain addresses: what Scene.trace_one calls, without a
    NumPy array made per call (a plane of 4096 samples per pixel is a quarter of a million segments)"""
    L = orc.lib()
    trace = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(("orc_trace_one", L))
    draw = C.CFUNCTYPE(C.c_float, C.c_void_p, C.c_int)(("orc_normal_next", L))
    return trace, draw


def ao_reference(orc, oracle, cam_floats, W, H, samples, radius, bias, time_ms):
    """-> dict: count [H, W] uint16, ao [H, W] float32, and per sample free [H, W, samples] uint8, hit [H, W, samples] bool, t [H, W,
    samples] float32 (the oracle's blocker distance, NaN without one), direction [H, W, samples, 3]; origin [H, W, 3] (o'), surface
    [H, W] bool.  All float arrays are binary32, so every NumPy operation below is rounded to binary32 once."""
    trace, draw = _oracle_calls(orc)
    det, scene = orc.MATH_DET, oracle._h
    n = W * H
    prim = np.ascontiguousarray(primaries(cam_floats, W, H).reshape(n, 3), F)
    cam_pos = np.ascontiguousarray(cam_floats[0:3], F)
    radius, bias = F(radius), F(bias)
    rec = np.zeros(8, F)
    rec_at = rec.ctypes.data
    # 1. the primary rays' closest hits
    surface = np.zeros(n, bool)
    P, N = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for i in range(n):
        if trace(scene, cam_pos.ctypes.data, prim.ctypes.data + 12 * i, rec_at):
            surface[i] = True
            P[i], N[i] = rec[1:4], rec[4:7]
    idx = np.flatnonzero(surface)
    m = len(idx)
    N = np.ascontiguousarray(N[idx])
    # 2. o' = N * bias + P, two roundings
    o2 = np.ascontiguousarray(N * bias + P[idx])
    # 3. the renderer's per-pixel stream
    state = np.array([seed_of(int(i) % W, int(i) // W, W, time_ms) for i in idx], np.uint32)
    free = np.zeros((n, samples), np.uint8)
    hits = np.zeros((n, samples), bool)
    t = np.full((n, samples), np.nan, F)
    dirs = np.zeros((n, samples, 3), F)
    d = np.zeros((m, 3), F)
    o2_at, d_at, state_at = o2.ctypes.data, d.ctypes.data, state.ctypes.data
    # 4. the samples, in order: three draws (six PCG steps) per sample and pixel whatever it meets
    for k in range(samples):
        g = []
        for j in range(m):
            a = state_at + 4 * j
            g += [draw(a, det), draw(a, det), draw(a, det)]
        r = np.array(g, F).reshape(m, 3)
        r = np.where((_dot(r, N) < F(0.0))[:, None], -r, r)
        r = _normalised(r)
        d[...] = _normalised(N + r)
        hk, tk = np.zeros(m, bool), np.full(m, np.nan, F)
        for j in range(m):
            if trace(scene, o2_at + 12 * j, d_at + 12 * j, rec_at):
                hk[j], tk[j] = True, rec[0]
        with np.errstate(invalid="ignore"):
            occluded = hk & (tk <= radius)
        free[idx, k], hits[idx, k], t[idx, k], dirs[idx, k] = ~occluded, hk, tk, d
    # 5.
    count = np.full(n, NO_SURFACE, np.uint16)
    count[idx] = free[idx].sum(axis=1)
    ao = np.ones(n, F)
    ao[idx] = count[idx].astype(F) / F(samples)
    origin = np.zeros((n, 3), F)
    origin[idx] = o2
    return {"count": count.reshape(H, W), "ao": ao.reshape(H, W), "free": free.reshape(H, W, samples), "hit": hits.reshape(H, W, samples),
            "t": t.reshape(H, W, samples), "direction": dirs.reshape(H, W, samples, 3), "origin": origin.reshape(H, W, 3),
            "surface": surface.reshape(H, W)}


def whitened(objs):
    """the scene with every material replaced by white diffuse"""
    return [tuple(o[:-1]) + (WHITE,) for o in objs]


_CACHE = {}


def scene_reference(rt, orc, models_dir, name, W, H, samples, radius, bias, time_ms, objs=None):
    """ao_reference for a scene (a config scene by its name, or `objs` under a name of the caller's) and the default camera, computed once
    per parameter set and shared; callers leave it unchanged"""
    key = (name, W, H, samples, float(radius), float(bias), time_ms)
    if key not in _CACHE:
        if objs is None:
            objs, _ = rt.scenes.CONFIG_SCENES[name]()
        oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
        _CACHE[key] = ao_reference(orc, oracle, rt.Camera(W, H).floats(), W, H, samples, radius, bias, time_ms)
    return _CACHE[key]
