"""What a render call takes: materials, meshes, the scene's object list, camera, settings, a GPU context and a committed scene."""
import ctypes as C
import os

import numpy as np

from . import scenes
from ._abi import (KERNEL_VARIANTS, SCENE_TRAITS, RT_ERR_BUSY, RT_ERR_INVALID, RT_ERR_IO, RT_ERR_NO_DEVICE, RT_ERR_UNSUPPORTED, RT_OK, PipelineFullError, RayTracerError,
                   UnsupportedMeshError, _fp, lib, rt_camera, rt_flat_view, rt_material, rt_render_settings, rt_scene_info, rt_winding_tree_view)


class Material:
    """Material + Texture factories, reference src/material.cu:21-51, :157-185."""

    def __init__(self, c_struct):
        self.c = c_struct

    @staticmethod
    def _create(kind, *args):
        m = rt_material()
        getattr(lib(), "rt_material_" + kind)(C.byref(m), *args)
        return Material(m)

    @staticmethod
    def create_standard(colour, smoothness):
        return Material._create("standard", _fp(colour)[1], C.c_float(smoothness))

    @staticmethod
    def create_checkerboard(light, dark, num_squares, smoothness):
        return Material._create("checkerboard", _fp(light)[1], _fp(dark)[1], int(num_squares), C.c_float(smoothness))

    @staticmethod
    def create_gradient(smoothness):
        return Material._create("gradient", C.c_float(smoothness))

    @staticmethod
    def create_emissive(colour, strength):
        return Material._create("emissive", _fp(colour)[1], C.c_float(strength))

    @staticmethod
    def create_refractive(colour, n):
        return Material._create("refractive", _fp(colour)[1], C.c_float(n))

    @staticmethod
    def create_image(rgb, smoothness):
        """rgb: [height, width, 3] float32 texels (Texture::create_image src/material.cu:42-51);
        the scene builder copies them when the object is added"""
        arr, p = _fp(np.asarray(rgb, np.float32))
        mat = Material._create("image", arr.shape[1], arr.shape[0], p, C.c_float(smoothness))
        mat._keep = arr
        return mat

    @staticmethod
    def from_desc(desc):
        kind = desc[0]
        nargs = {"standard": 2, "emissive": 2, "checkerboard": 4, "gradient": 1, "refractive": 2, "image": 2}.get(kind)
        if nargs is None:
            raise ValueError(kind)
        return getattr(Material, "create_" + kind)(*[desc[1 + i] for i in range(nargs)])


def load_image_texture(parsed_textures_path, name):
    """ImageTexture src/main.cu:40-91: entry `name` of a baked texture file -> [h, w, 3] float32"""
    w, h = C.c_int32(), C.c_int32()
    ptr = C.POINTER(C.c_float)()
    st = lib().rt_image_texture_load(os.fsencode(parsed_textures_path), name.encode(), C.byref(w), C.byref(h), C.byref(ptr))
    if st == RT_ERR_IO:
        raise RayTracerError("Could not find file to open.")
    if st != RT_OK:
        raise RayTracerError("Image file not found.\n")
    try:
        return np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 3)).copy()
    finally:
        lib().rt_image_texture_free(ptr)


class _Handle:
    """Owner of one C-side object: self._h, released by the library function the subclass names in _destroy."""
    _destroy = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                getattr(lib(), self._destroy)(self._h)
                self._h = None
        except Exception:      # interpreter shutdown: module globals may already be gone
            pass


class ObjFileMesh(_Handle):
    """reference src/obj_read.cu:47-147"""
    _destroy = "rt_obj_destroy"

    def __init__(self, filename, _handle=None):
        if _handle is not None:
            self._h = _handle
            return
        h = C.c_void_p()
        st = lib().rt_obj_load(os.fsencode(filename), C.byref(h))
        if st == RT_ERR_IO:
            raise RayTracerError("Could not find file to open.")
        if st != RT_OK:
            raise RayTracerError("could not parse %s" % filename)
        self._h = h

    @staticmethod
    def from_arrays(vertices, faces):
        """vertices [n,3] float32; faces: list of 0-based index lists"""
        v, vp_ = _fp(np.asarray(vertices, np.float32).reshape(-1, 3))
        flat = np.ascontiguousarray([i for f in faces for i in f], dtype=np.int32)
        arity = np.ascontiguousarray([len(f) for f in faces], dtype=np.int32)
        h = C.c_void_p()
        st = lib().rt_obj_from_arrays(vp_, v.shape[0], flat.ctypes.data_as(C.POINTER(C.c_int32)),
                                      arity.ctypes.data_as(C.POINTER(C.c_int32)), len(faces), C.byref(h))
        if st != RT_OK:
            raise ValueError("bad mesh arrays")
        return ObjFileMesh(None, _handle=h)

    def faces(self):
        out = []
        for i, a in enumerate(self.face_arities()):
            buf = (C.c_int32 * a)()
            lib().rt_obj_get_face(self._h, i, buf)
            out.append(list(buf))
        return out

    def enlarge(self, scale_fact):
        lib().rt_obj_enlarge(self._h, C.c_float(scale_fact))

    def rotate(self, x_angle, y_angle, z_angle):
        lib().rt_obj_rotate(self._h, C.c_float(x_angle), C.c_float(y_angle), C.c_float(z_angle))

    def translate(self, offset_x, offset_y, offset_z):
        lib().rt_obj_translate(self._h, C.c_float(offset_x), C.c_float(offset_y), C.c_float(offset_z))

    @property
    def num_vertices(self):
        return lib().rt_obj_num_vertices(self._h)

    @property
    def num_faces(self):
        return lib().rt_obj_num_faces(self._h)

    def face_arities(self):
        return [lib().rt_obj_face_arity(self._h, i) for i in range(self.num_faces)]

    def vertices(self):
        out = np.empty((self.num_vertices, 3), np.float32)
        lib().rt_obj_get_vertices(self._h, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def triangles(self):
        n = lib().rt_obj_num_triangles(self._h)
        if n < 0:
            raise UnsupportedMeshError("Only triangle or quad meshes are supported.\n")
        out = np.empty((n, 9), np.float32)
        st = lib().rt_obj_get_triangles(self._h, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st != RT_OK:
            raise ValueError("face references a missing vertex")
        return out


def _flat_view_arrays(v):
    """an rt_flat_view (rt_debug_flatten, rt_debug_scene_read) as a dict of copies"""
    blob = np.ctypeslib.as_array(v.blob, shape=(v.blob_f4, 4)).copy() if v.blob_f4 else np.zeros((0, 4), np.float32)
    raw = C.string_at(v.objects, v.num_objects * v.object_stride) if v.num_objects else b""
    objs = np.frombuffer(raw, dtype=np.dtype([("type", "<i4"), ("prim_start", "<i4"), ("need_uv", "<i4"), ("root_ref", "<u4"), ("v", "<f4", (8,))]))
    uv = np.ctypeslib.as_array(v.tri_uv, shape=(v.num_triangles, 6)).copy() if v.tri_uv else None
    flip = np.ctypeslib.as_array(v.tri_flip, shape=(v.num_triangles,)).copy() if v.tri_flip and v.num_triangles else np.zeros(0, np.uint8)
    return {"blob": blob, "tri_flip": flip, "off_nodes": v.off_nodes, "off_tris": v.off_tris, "off_objlds": v.off_objlds,
            "off_meshes": v.off_meshes, "num_meshes": v.num_meshes, "stack_entries": v.stack_entries,
            "objects": objs, "tri_uv": uv, "num_triangles": v.num_triangles, "num_nodes": v.num_nodes,
            "has_mesh": bool(v.has_mesh),
            "traits": {name for name, bit in SCENE_TRAITS.items() if v.traits & bit}, "kernel_variant": KERNEL_VARIANTS[v.kernel_variant]}


def _winding_tree_arrays(v):
    """an rt_winding_tree_view (rt_debug_winding_tree, rt_debug_scene_winding_tree) as a dict of copies"""
    def ints(p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if p and n else np.zeros(0, np.int32)
    nc = v.num_clusters
    return {"skip": ints(v.skip, nc), "first": ints(v.first, nc), "count": ints(v.count, nc),
            "object_range": ints(v.object_range, 2 * v.num_objects).reshape(-1, 2), "order": ints(v.order, v.num_triangles), "position": ints(v.position, v.num_triangles),
            "moments": np.ctypeslib.as_array(v.moments, shape=(nc, 8)).copy() if v.moments and nc else np.zeros((0, 8), np.float32)}


class SceneObjects(_Handle):
    """The object list of a scene: reference SceneObjects src/main.cu:94-296 with the
    Object::create_* factories of src/objects.cu:845-906 as methods."""
    _destroy = "rt_scene_builder_destroy"

    def __init__(self, description=None, models_dir=None):
        h = C.c_void_p()
        if lib().rt_scene_builder_create(C.byref(h)) != RT_OK:
            raise MemoryError()
        self._h = h
        self.models_dir = models_dir or scenes.models_dir()
        if description:
            self.add_description(description)

    def _check(self, st):
        if st == RT_OK:
            return
        msg = lib().rt_scene_builder_error(self._h).decode()
        if st == RT_ERR_UNSUPPORTED and "triangle or quad" in msg:
            raise UnsupportedMeshError(msg)
        if st == RT_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise ValueError(msg)

    def create_sphere(self, center, radius, mat):
        self._check(lib().rt_scene_add_sphere(self._h, _fp(center)[1], C.c_float(radius), C.byref(mat.c)))

    def create_triangle(self, p1, p2, p3, mat, uv=None):
        if uv is None:
            self._check(lib().rt_scene_add_triangle(self._h, _fp(p1)[1], _fp(p2)[1], _fp(p3)[1], C.byref(mat.c)))
        else:
            pts = np.concatenate([np.asarray(p, np.float32).reshape(3) for p in (p1, p2, p3)])
            self._check(lib().rt_scene_add_triangle_uv(self._h, _fp(pts)[1], _fp(np.asarray(uv).reshape(6))[1], C.byref(mat.c)))

    def create_quad(self, p1, p2, p3, p4, mat):
        self._check(lib().rt_scene_add_quad(self._h, _fp(p1)[1], _fp(p2)[1], _fp(p3)[1], _fp(p4)[1], C.byref(mat.c)))

    def create_one_way_quad(self, p1, p2, p3, p4, invert_normal, mat):
        self._check(lib().rt_scene_add_one_way_quad(self._h, _fp(p1)[1], _fp(p2)[1], _fp(p3)[1], _fp(p4)[1], int(bool(invert_normal)), C.byref(mat.c)))

    def create_cuboid(self, tl_near_pos, width, height, depth, mat):
        self._check(lib().rt_scene_add_cuboid(self._h, _fp(tl_near_pos)[1], C.c_float(width), C.c_float(height), C.c_float(depth), C.byref(mat.c)))

    def create_mesh(self, mesh, mat):
        """mesh: an ObjFileMesh (src/main.cu:127-148) or an array of triangles [n, 9]"""
        if isinstance(mesh, ObjFileMesh):
            self._check(lib().rt_scene_add_obj_mesh(self._h, mesh._h, C.byref(mat.c)))
        else:
            arr, p = _fp(np.asarray(mesh, np.float32).reshape(-1, 9))
            self._check(lib().rt_scene_add_mesh(self._h, p, arr.shape[0], C.byref(mat.c)))

    def add_description(self, description):
        for o in description:
            kind, mat = o[0], Material.from_desc(o[-1])
            if kind == "sphere":
                self.create_sphere(o[1], o[2], mat)
            elif kind == "triangle":
                self.create_triangle(o[1], o[2], o[3], mat)
            elif kind == "triangle_uv":
                p = np.asarray(o[1], np.float32).reshape(3, 3)
                self.create_triangle(p[0], p[1], p[2], mat, uv=o[2])
            elif kind == "quad":
                self.create_quad(o[1], o[2], o[3], o[4], mat)
            elif kind == "one_way_quad":
                self.create_one_way_quad(o[1], o[2], o[3], o[4], o[5], mat)
            elif kind == "cuboid":
                self.create_cuboid(o[1], o[2], o[3], o[4], mat)
            elif kind == "mesh":
                self.create_mesh(o[1], mat)
            elif kind == "obj":
                path = o[1] if os.path.isabs(o[1]) else os.path.join(self.models_dir, o[1])
                m = ObjFileMesh(path)
                for t in o[2]:
                    getattr(m, t[0])(*t[1:])
                self.create_mesh(m, mat)
            else:
                raise ValueError(kind)

    @property
    def num_objects(self):
        return lib().rt_scene_builder_num_objects(self._h)

    def debug_flatten(self):
        """The flattened device layout as numpy arrays (tests only)."""
        v = rt_flat_view()
        self._check(lib().rt_debug_flatten(self._h, C.byref(v)))
        return _flat_view_arrays(v)

    def debug_winding_tree(self):
        """The fast winding numbers' cluster trees as the host computes them, no device (tests only): skip, first, count [clusters],
        object_range [objects, 2], order and position [triangles], moments [clusters, 8] (c.xyz, r2, M.xyz, 0)."""
        v = rt_winding_tree_view()
        self._check(lib().rt_debug_winding_tree(self._h, C.byref(v)))
        return _winding_tree_arrays(v)


class Camera:
    """reference Camera src/camera.cu:32-108; ``assign_constant_mem`` becomes :attr:`c` (the
    48-byte DeviceCamData plus the image size), passed to render calls."""

    def __init__(self, width, height, pos=None, fov=None, focal_len=None, rot=(0.0, 0.0, 0.0), floats=None):
        self.c = rt_camera()
        if floats is not None:      # the 12 floats verbatim (fixtures)
            f = np.asarray(floats, np.float32).reshape(12)
            self.c.cam_pos[:] = f[0:3].tolist()
            self.c.tl_pixel_pos[:] = f[3:6].tolist()
            self.c.delta_u[:] = f[6:9].tolist()
            self.c.delta_v[:] = f[9:12].tolist()
            self.c.width, self.c.height = int(width), int(height)
        elif pos is None and fov is None and focal_len is None and tuple(rot) == (0.0, 0.0, 0.0):
            lib().rt_camera_default(int(width), int(height), C.byref(self.c))
        else:
            pi = np.float32(3.141592653589793)
            fov = np.float32(60) * (pi / np.float32(180)) if fov is None else fov
            lib().rt_camera_make(int(width), int(height), _fp(pos or (0, 0, 0))[1], C.c_float(fov),
                                 C.c_float(0.1 if focal_len is None else focal_len),
                                 C.c_float(rot[0]), C.c_float(rot[1]), C.c_float(rot[2]), C.byref(self.c))

    @property
    def width(self):
        return self.c.width

    @property
    def height(self):
        return self.c.height

    def floats(self):
        return np.array(list(self.c.cam_pos) + list(self.c.tl_pixel_pos) + list(self.c.delta_u) + list(self.c.delta_v), np.float32)

    def lens(self, focal_len, focus_dist, u, v):
        """One thin-lens sample of this pinhole camera (rt_camera_lens): the image plane at focus_dist, the eye moved by (u, v) on the lens.
        focal_len is what this camera was made with (0.1 by default)."""
        out = Camera(self.width, self.height, floats=self.floats())
        if lib().rt_camera_lens(C.byref(self.c), C.c_float(focal_len), C.c_float(focus_dist), C.c_float(u), C.c_float(v), C.byref(out.c)) != 0:
            raise ValueError("focal_len and focus_dist must be positive and finite, the offset finite, and the camera's pixel steps not zero")
        return out


class RenderData:
    """reference RenderData src/raytracer.cu:4-12 (defaults of RenderSettings src/main.cu:318-330)"""

    def __init__(self, rays_per_pixel=100, reflection_limit=5, antialias=True, sky_colour=(0.0, 0.0, 0.0)):
        self.c = rt_render_settings(int(rays_per_pixel), int(reflection_limit), int(bool(antialias)), (C.c_float * 3)(*[float(x) for x in sky_colour]))


class VariableRenderData:
    """reference VariableRenderData src/dispatch.cu:111-115"""

    def __init__(self, width, height):
        self.frame_num = 0
        self.previous_render = np.zeros((height, width, 3), np.float32)


class Context(_Handle):
    """One per GPU.  Raises when there is no GPU (the product has no CPU path)."""
    _destroy = "rt_ctx_destroy"

    def __init__(self, device=0):
        h = C.c_void_p()
        st = lib().rt_ctx_create(int(device), C.byref(h))
        if st == RT_ERR_NO_DEVICE:
            raise RayTracerError("Error from HIP (creating context): no usable GPU; ray-tracer_amd has no CPU fallback")
        if st != RT_OK:
            raise RayTracerError("Error from HIP (creating context): status %d" % st)
        self._h = h
        self.device = device

    def _check(self, st):
        if st != RT_OK:
            msg = lib().rt_last_error(self._h).decode()
            if st == RT_ERR_UNSUPPORTED:
                raise NotImplementedError(msg)
            if st == RT_ERR_INVALID:
                raise ValueError(msg)
            if st == RT_ERR_BUSY:
                raise PipelineFullError(msg)
            raise RayTracerError(msg)

    def last_error(self):
        """the context's most recent error message (rt_last_error; empty when there was none)"""
        m = lib().rt_last_error(self._h)
        return m.decode() if m else ""

    def commit(self, scene_objects):
        return Scene(self, scene_objects)

    def last_kernel_ms(self):
        ms = C.c_float()
        self._check(lib().rt_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def synchronize(self):
        """waits for this context's most recent launch"""
        self._check(lib().rt_ctx_synchronize(self._h))

    def tile_costs(self, with_peaks=False):
        """(tile indices in the image, costs[, peak pixel costs]) of the current view's tiles as its first launch measured
        them (rt_tile_costs; waits for that launch)"""
        n = C.c_int32()
        self._check(lib().rt_tile_costs(self._h, None, None, None, 0, C.byref(n)))
        ids, costs, peaks = np.empty(n.value, np.uint32), np.empty(n.value, np.uint32), np.empty(n.value, np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._check(lib().rt_tile_costs(self._h, ids.ctypes.data_as(u32p), costs.ctypes.data_as(u32p), peaks.ctypes.data_as(u32p), n.value, C.byref(n)))
        return (ids, costs, peaks) if with_peaks else (ids, costs)

    def max_batch_frames(self, width, height):
        """frames the multi-frame entry points put into one launch for this image size (rt_max_batch_frames)"""
        return lib().rt_max_batch_frames(self._h, int(width), int(height))

    def peer_access(self, other):
        """1: copies between the two contexts' GPUs go direct (xGMI), 0: staged by the runtime (rt_peer_access)"""
        return lib().rt_peer_access(self._h, other._h)


class Scene(_Handle):
    """A committed (uploaded) scene: replaces create_gpu_struct src/main.cu:290-295 +
    allocate_constant_mem src/dispatch.cu:104-108."""
    _destroy = "rt_scene_destroy"

    def __init__(self, ctx, scene_objects):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(lib().rt_scene_commit(ctx._h, scene_objects._h, C.byref(h)))
        self._h = h

    def info(self):
        i = rt_scene_info()
        self.ctx._check(lib().rt_scene_get_info(self._h, C.byref(i)))
        out = {n: getattr(i, n) for n, _ in i._fields_}
        out["kernel_variant"] = KERNEL_VARIANTS[i.kernel_variant]      # "generic" or "traits": which render kernel the scene's plain frames run
        return out
