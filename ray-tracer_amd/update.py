"""Time-varying geometry: a committed mesh rebuilt from new vertices on the device (rt_scene_update_mesh[_device], include/rt_amd.h).
The methods are attached to :class:`Scene`: ``scene.update_mesh(i, triangles)``, ``scene.update_mesh_device(i, tensor)``."""
from ._abi import REBUILD_LDS_TRIS, C, _dptr, fp, lib, np, rt_flat_view, rt_winding_tree_view  # noqa: F401  (REBUILD_LDS_TRIS is re-exported)
from .objects import Scene, _flat_view_arrays, _winding_tree_arrays


def _triangle_rows(triangles):
    arr = np.ascontiguousarray(triangles, dtype=np.float32)
    if arr.ndim != 2 or arr.shape[1] != 9:
        raise ValueError("triangles must have the shape [n, 9]: three points per row")
    return arr


def update_mesh(self, object_index, triangles):
    """The mesh at object_index gets new vertices: row i of `triangles` ([n, 9], n the mesh's triangle count) replaces the triangle given
    i-th at commit.  Everything the kernels read is afterwards what a fresh commit with these triangles uploads.  Returns when done."""
    arr = _triangle_rows(triangles)
    self.ctx._check(lib().rt_scene_update_mesh(self.ctx._h, self._h, int(object_index), arr.ctypes.data_as(fp), arr.shape[0]))


def update_mesh_device(self, object_index, triangles, stream=None, n=None):
    """The same from device memory, asynchronously on `stream` (a hipStream_t as an int; None: the default stream) and in the context's launch
    order.  `triangles` is a contiguous float32 torch tensor of 9 n elements on the scene's GPU, or a device pointer as an int together with n."""
    if isinstance(triangles, int):
        if n is None:
            raise ValueError("a device pointer needs n, the number of triangles")
        ptr, count = triangles, int(n)
    else:
        t = triangles
        if str(t.dtype) != "torch.float32" or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("triangles must be a contiguous float32 tensor on the GPU")
        if t.numel() % 9 or (n is not None and int(n) * 9 != t.numel()) or (t.dim() > 1 and t.shape[-1] not in (3, 9)):
            raise ValueError("triangles must hold 9 floats per triangle")
        ptr, count = t.data_ptr(), t.numel() // 9
    self.ctx._check(lib().rt_scene_update_mesh_device(self.ctx._h, self._h, int(object_index), _dptr(ptr), count, _dptr(stream)))


def debug_read(self):
    """The scene as it is ON THE DEVICE, in the dict shape of SceneObjects.debug_flatten() (tests only; waits for the device)."""
    v = rt_flat_view()
    self.ctx._check(lib().rt_debug_scene_read(self.ctx._h, self._h, C.byref(v)))
    return _flat_view_arrays(v)


def debug_winding_tree(self):
    """The fast winding numbers' cluster trees as the device holds them now, in the dict shape of SceneObjects.debug_winding_tree() (tests
    only; builds and refits them if no fast query has, and waits for the device)."""
    v = rt_winding_tree_view()
    self.ctx._check(lib().rt_debug_scene_winding_tree(self.ctx._h, self._h, C.byref(v)))
    return _winding_tree_arrays(v)


Scene.debug_winding_tree = debug_winding_tree
Scene.update_mesh = update_mesh
Scene.update_mesh_device = update_mesh_device
Scene.debug_read = debug_read
