"""The yardstick of the cube-map sky (include/rt_amd.h: rt_sky_create, rt_sky_texel_direction, rt_render_sky[_device]): the definition
restated in plain Python / NumPy binary32 over the CPU oracle's exported pieces - orc_trace_one_uv for every segment, orc_pcg_next and
orc_normal_next for every draw, orc_math_* for the refraction, tests/texture_ref.py for the texture colours - with the bounce loop of
oracle/rt_oracle_core.inc (antialias jitter, reflect, refract, emission, throughput) for all three material types and the cube-map lookup
at the miss.  The per-pixel mean and the frame fold follow tests/views_ref.py's conventions: the canonical NaN, and -0 -> +0 at frame 0.
No product code.  Every array is binary32, so every NumPy operation below is rounded to binary32 once, in the header's order; nothing is
fused.  tests/test_sky_ref.py pins the loop to the oracle's own renderer."""
import ctypes as C

import numpy as np

import texture_ref
from ao_ref import seed_of
from test_gpu_query import primaries

F = np.float32
ZERO, ONE, HALF, TWO = F(0.0), F(1.0), F(0.5), F(2.0)
CANON_NAN = np.uint32(0x7FC00000)
RANGE = float(F(0.001))                 # ANTIALIAS_OFFSET_RANGE, a binary32 constant used in binary64


# ---- the cube map ---------------------------------------------------------------------------------------------------------------------------
def _coord(s, n):
    """(s * 0.5f + 0.5f) * (float)n -> towards zero, saturating, NaN -> 0, clamped to 0 .. n - 1"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(texture_ref.f2i((s * HALF + HALF) * F(n)), 0, n - 1)


def lookup(d, n):
    """directions [..., 3] (binary32) -> face, row, col (integer arrays of the leading shape)"""
    d = np.asarray(d, F)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(invalid="ignore"):
        is_x = (ax >= ay) & (ax >= az)
        is_y = ~is_x & (ay >= az)
    axis = np.where(is_x, 0, np.where(is_y, 1, 2))
    c = np.where(is_x, x, np.where(is_y, y, z))
    a = np.where(is_x, y, np.where(is_y, z, x))
    b = np.where(is_x, z, np.where(is_y, x, y))
    m = np.abs(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        face = 2 * axis + (c < ZERO)
        s, t = a / m, b / m
    return face.astype(np.int64), _coord(t, n), _coord(s, n)


def texel_directions(n):
    """[6, n, n, 3]: s = ((float)col + 0.5f) / (float)n * 2.0f - 1.0f, t from the row likewise, the major component +1 or -1; not normalised"""
    c = ((np.arange(n).astype(F) + HALF) / F(n)) * TWO - ONE
    out = np.empty((6, n, n, 3), F)
    for face in range(6):
        axis = face >> 1
        out[face, :, :, axis] = F(-1.0) if face & 1 else ONE
        out[face, :, :, (axis + 1) % 3] = c[None, :]
        out[face, :, :, (axis + 2) % 3] = c[:, None]
    return out


def normalised_rows(a):
    """rows of [..., 3] as the renderer normalises: a * (1.0f / sqrtf((x*x + y*y) + z*z))"""
    a = np.asarray(a, F)
    sq = a * a
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = ONE / np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])
        return a * inv[..., None]


# ---- the bounce loop ------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    p = a * b
    return (p[0] + p[1]) + p[2]


def _normalised(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return a * (ONE / np.sqrt(_dot(a, a)))


def _dmin(a, b):
    """CUDA's min(float, double) in binary64, dropping a NaN like fmin"""
    return a if b != b else (b if a != a else (a if a < b else b))


SMOOTHNESS_AT = {"standard": 2, "gradient": 1, "checkerboard": 4, "image": 2}       # where the neutral description keeps it


def _smoothness(material):
    """Material::smoothness: a standard material's own; 0 for an emissive one, 1 for a refractive one (oracle/rt_oracle.c's factories)"""
    kind = material[0]
    return F(material[SMOOTHNESS_AT[kind]]) if kind in SMOOTHNESS_AT else F({"emissive": 0.0, "refractive": 1.0}[kind])


class _Oracle:
    """the oracle's exported pieces taking plain addresses (what orc.Scene.trace_one_uv and orc.pcg_stream call, without an array per call)"""

    def __init__(self, orc, oracle):
        L = orc.lib()
        self.det, self.scene = orc.MATH_DET, oracle._h
        self.trace = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(("orc_trace_one_uv", L))
        self.pcg = C.CFUNCTYPE(C.c_float, C.c_void_p)(("orc_pcg_next", L))
        self.normal = C.CFUNCTYPE(C.c_float, C.c_void_p, C.c_int)(("orc_normal_next", L))
        self.sinf = lambda x: F(L.orc_math_sinf(float(x), self.det))
        self.cosf = lambda x: F(L.orc_math_cosf(float(x), self.det))
        self.asin = lambda x: L.orc_math_asin(float(x), self.det)
        self.acos = lambda x: L.orc_math_acos(float(x), self.det)
        self.state = np.zeros(1, np.uint32)
        self.o, self.d, self.rec = np.zeros(3, F), np.zeros(3, F), np.zeros(10, F)

    def u01(self):
        return F(self.pcg(self.state.ctypes.data))

    def gauss(self):
        return F(self.normal(self.state.ctypes.data, self.det))

    def closest(self, o, d):
        self.o[:], self.d[:] = o, d
        return bool(self.trace(self.scene, self.o.ctypes.data, self.d.ctypes.data, self.rec.ctypes.data))


def _reflect(k, d, N, smooth):
    """Ray::reflect: -> the new direction"""
    r = np.array([k.gauss(), k.gauss(), k.gauss()], F)
    if _dot(r, N) < ZERO:
        r = r * F(-1.0)
    r = _normalised(r)
    diffuse = _normalised(N + r)
    dn = _dot(d, N)
    specular = _normalised(d - (N * TWO) * dn)
    return _normalised(diffuse + (specular - diffuse) * smooth)


def _refract(k, d, N, material, cur_n):
    """Ray::refract: -> the new direction, the new current refractive index"""
    mat_n = F(material[2])
    if _dot(N, d) > ZERO:
        n1, n2, rn = mat_n, cur_n, N
    else:
        n1, n2, rn = cur_n, mat_n, N * F(-1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        theta1 = F(k.acos(_dmin(float(_dot(d, rn)), 1.0)))
        theta2 = F(k.asin(_dmin(float(n1 * k.sinf(theta1) / n2), 1.0)))
        critical = F(k.asin(float(n2 / n1)))
        sqrt_r0 = (n1 - n2) / (n1 + n2)
        r0 = sqrt_r0 * sqrt_r0
        x = float(ONE - k.cosf(theta1))
        x2 = x * x
        coeff = F(float(r0) + float(ONE - r0) * ((x2 * x2) * x))
        do_reflect = bool(theta1 > critical)
        if not do_reflect:
            do_reflect = bool(coeff > k.u01())
        if do_reflect:
            return _reflect(k, d, N, _smoothness(material)), n2
        perp = np.zeros(3, F)
        if theta1 != ZERO:
            perp = (d - rn * k.cosf(theta1)) / k.sinf(theta1)
        return _normalised(rn * k.cosf(theta2) + perp * k.sinf(theta2)), n2


def view_paths(orc, oracle, objs, cam, W, H, spp, limit, time_ms, antialias):
    """One view's paths, which no sky changes: per sample (arrays [H, W, spp, ...]) `fin`, the light its hits emitted, and where `missed`
    - the path left the scene - `d`, the direction it was traced with at the miss, and `thr`, its throughput there.  The Python loop
    runs once per (scene, camera, seed, settings); view_mean shades the paths under any map."""
    k = _Oracle(orc, oracle)
    cam = np.asarray(cam, F)
    prim = primaries(cam, W, H)
    shape = (H, W, max(spp, 0))
    paths = dict(fin=np.zeros(shape + (3,), F), thr=np.zeros(shape + (3,), F), d=np.zeros(shape + (3,), F), missed=np.zeros(shape, bool), spp=spp)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for py in range(H):
            for px in range(W):
                k.state[0] = seed_of(px, py, W, int(time_ms))
                for s in range(spp):
                    fin, thr = np.zeros(3, F), np.ones(3, F)
                    o, d, cur_n = cam[0:3].copy(), prim[py, px].copy(), ONE
                    for _ in range(limit):
                        if antialias:
                            off = np.array([F((float(k.u01()) - 0.5) * 2 * RANGE) for _ in range(3)], F)
                            d = _normalised(d + off)
                        if not k.closest(o, d):
                            paths["missed"][py, px, s], paths["d"][py, px, s], paths["thr"][py, px, s] = True, d, thr
                            break
                        rec = k.rec.copy()
                        P, N, material = rec[1:4], rec[4:7], objs[int(rec[7])][-1]
                        if material[0] == "refractive":
                            d, cur_n = _refract(k, d, N, material, cur_n)
                        else:
                            d = _reflect(k, d, N, _smoothness(material))
                        o = P
                        if material[0] == "emissive":
                            fin = fin + texture_ref.emitted(material) * thr
                        else:
                            thr = thr * texture_ref.texture_colour(material, rec[8], rec[9])
                    paths["fin"][py, px, s] = fin
    return paths


def view_mean(paths, faces, tint):
    """The paths of a view under the map `faces` [6, n, n, 3] tinted by `tint` (the render settings' sky colour): -> mean [H, W, 3], the
    sum of the pixel's samples in order / spp, and reads [H, W, spp, 3] int32, per sample the (face, row, col) it read or (-1, -1, -1)
    where its path did not end in the sky.  At the miss: L = texel * tint, fin = fin + L * thr."""
    faces, tint = np.asarray(faces, F), np.asarray(tint, F)
    face, row, col = lookup(paths["d"], faces.shape[1])
    missed = paths["missed"]
    reads = np.where(missed[..., None], np.stack([face, row, col], axis=-1), -1).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lit = paths["fin"] + (faces[face, row, col] * tint) * paths["thr"]
        fin = np.where(missed[..., None], lit, paths["fin"])
        colour = np.zeros(fin.shape[:2] + (3,), F)
        for s in range(fin.shape[2]):
            colour = colour + fin[:, :, s]
        return colour / F(paths["spp"]), reads


def view_means(orc, oracle, objs, cam, W, H, spp, limit, tint, time_ms, antialias, faces):
    """view_paths and view_mean in one call"""
    return view_mean(view_paths(orc, oracle, objs, cam, W, H, spp, limit, time_ms, antialias), faces, tint)


def _canon(a):
    u = np.ascontiguousarray(a, F).view(np.uint32).copy()
    u[np.isnan(a)] = CANON_NAN
    return u.view(F)


def fold(frame, mean, frame_num):
    """(c + prev * n) / (n + 1) with a NaN stored as the canonical quiet NaN; frame 0 does not read prev: (c + 0 * 0) / 1"""
    with np.errstate(invalid="ignore", over="ignore"):
        prev = np.zeros_like(mean) if frame is None or frame_num == 0 else np.asarray(frame, F)
        return _canon((mean + prev * F(frame_num)) / F(frame_num + 1))


def separate(means):
    """[n, H, W, 3]: every view's mean as its frame 0"""
    return np.stack([fold(None, m, 0) for m in means])


def accumulated(means, frame_num=0, prev=None):
    """[H, W, 3]: view i folded as progressive frame frame_num + i over `prev` (the image after frame_num - 1)"""
    frame = prev
    for i, m in enumerate(means):
        frame = fold(frame, m, frame_num + i)
    return frame
