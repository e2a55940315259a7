"""The edge-avoiding a-trous denoiser driven by the first-hit planes."""
import ctypes as C

import numpy as np

from ._abi import _dptr, _fp, lib, rt_denoise_params
from .query import render_aov_device
from .render import render_device_batch


class DenoiseParams:
    """rt_denoise_params (include/rt_amd.h): the library's defaults (rt_denoise_params_default) with the given fields replaced"""

    def __init__(self, iterations=None, sigma_colour=None, sigma_depth=None, normal_power_log2=None, albedo_floor=None):
        self.c = rt_denoise_params()
        lib().rt_denoise_params_default(C.byref(self.c))
        for name, value in (("iterations", iterations), ("sigma_colour", sigma_colour), ("sigma_depth", sigma_depth),
                            ("normal_power_log2", normal_power_log2), ("albedo_floor", albedo_floor)):
            if value is not None:
                setattr(self.c, name, value)

    def as_dict(self):
        return {n: getattr(self.c, n) for n in ("iterations", "sigma_colour", "sigma_depth", "normal_power_log2", "albedo_floor")}


def denoise(ctx, colour, normal, depth, object=None, albedo=None, params=None):
    """The edge-avoiding a-trous filter (rt_denoise): colour, normal [H, W, 3] and depth [H, W] float32, optionally object [H, W] int32
    (taps across an id edge are skipped) and albedo [H, W, 3] (the colour is divided by it before the filter and multiplied after) - the
    planes render_aov gives.  Returns the filtered [H, W, 3] float32 image; include/rt_amd.h defines it to the bit."""
    z = np.ascontiguousarray(depth, dtype=np.float32)
    if z.ndim != 2:
        raise ValueError("depth must be [H, W]")
    H, W = z.shape
    c = np.ascontiguousarray(colour, dtype=np.float32)
    n = np.ascontiguousarray(normal, dtype=np.float32)
    o = None if object is None else np.ascontiguousarray(object, dtype=np.int32)
    a = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32)
    if c.shape != (H, W, 3) or n.shape != (H, W, 3) or (o is not None and o.shape != (H, W)) or (a is not None and a.shape != (H, W, 3)):
        raise ValueError("the planes differ in shape")
    params = params or DenoiseParams()
    out = np.zeros((H, W, 3), np.float32)
    ctx._check(lib().rt_denoise(ctx._h, W, H, _fp(c)[1], _fp(n)[1], _fp(z)[1], o.ctypes.data_as(C.POINTER(C.c_int32)) if o is not None else None,
                                _fp(a)[1] if a is not None else None, C.byref(params.c), _fp(out)[1]))
    return out


def denoise_device(ctx, width, height, d_colour, d_normal, d_depth, d_object, d_albedo, d_out, params=None, stream=None):
    """Device-buffer form (rt_denoise_device): device pointers to the planes (d_object, d_albedo may be None) and to W * H * 3 floats of
    output, which may be d_colour; asynchronous on `stream`."""
    params = params or DenoiseParams()
    ctx._check(lib().rt_denoise_device(ctx._h, int(width), int(height), *[_dptr(p) for p in (d_colour, d_normal, d_depth, d_object, d_albedo)],
                                       C.byref(params.c), _dptr(d_out), _dptr(stream)))


def render_denoised(ctx, scene, camera, settings, times_ms, params=None):
    """Scene in, picture out, all on the device: renders len(times_ms) progressive frames (render_device_batch), takes the view's first-hit
    planes (render_aov_device; the sky colour is the settings') and filters the frame with them (denoise_device, albedo demodulated).
    Returns (noisy, denoised), two [H, W, 3] float32 arrays."""
    import torch
    W, H = camera.width, camera.height
    dev = torch.device("cuda:%d" % ctx.device)
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    out = torch.empty_like(frame)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    normal, albedo = torch.empty_like(frame), torch.empty_like(frame)
    obj = torch.empty((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    render_device_batch(ctx, scene, camera, settings, list(times_ms), 0, frame.data_ptr())
    render_aov_device(ctx, scene, camera, tuple(settings.c.sky_colour), d_depth=depth.data_ptr(), d_normal=normal.data_ptr(), d_albedo=albedo.data_ptr(),
                      d_object=obj.data_ptr())
    denoise_device(ctx, W, H, frame.data_ptr(), normal.data_ptr(), depth.data_ptr(), obj.data_ptr(), albedo.data_ptr(), out.data_ptr(), params)
    ctx.synchronize()
    return frame.cpu().numpy(), out.cpu().numpy()
