"""The yardstick of the camera sequences (include/rt_amd.h: rt_render_views, rt_render_views_device, rt_camera_lens): the definitions
restated over the CPU oracle's own renderer (orc.Scene.render, one call per view with that view's twelve camera floats) and, for the lens,
in NumPy float32.  No product code.  Every array is binary32, so every NumPy operation below is rounded to binary32 once, in the header's
order; nothing is fused."""
import numpy as np

F = np.float32


def separate(oracle, cams, W, H, spp, limit, sky, times_ms, antialias=True):
    """[n, H, W, 3]: view i is the oracle's frame 0 of camera cams[i] (12 floats) seeded with times_ms[i]"""
    assert len(cams) == len(times_ms)
    return np.stack([oracle.render(np.asarray(c, F), W, H, spp, limit, sky, time_ms=int(t), frame_num=0, antialias=antialias)
                     for c, t in zip(cams, times_ms)])


def accumulated(oracle, cams, W, H, spp, limit, sky, times_ms, frame_num=0, prev=None, antialias=True):
    """[H, W, 3]: view i is progressive frame frame_num + i of the oracle, each rendered over the one before (`prev`: the image after
    frame_num - 1; not read when frame_num == 0, like the oracle's own frame 0)"""
    assert len(cams) == len(times_ms)
    frame = None if prev is None else np.ascontiguousarray(prev, F).copy()
    for i, (c, t) in enumerate(zip(cams, times_ms)):
        frame = oracle.render(np.asarray(c, F), W, H, spp, limit, sky, time_ms=int(t), frame_num=frame_num + i, antialias=antialias, prev=frame)
    return frame


def lens(cam, focal_len, focus_dist, lens_u, lens_v):
    """rt_camera_lens on the 12 floats (cam_pos, tl_pixel_pos, delta_u, delta_v) -> the 12 floats of the lens sample"""
    cam = np.asarray(cam, F).reshape(12)
    pos, tl, du, dv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    focal_len, focus_dist, lens_u, lens_v = F(focal_len), F(focus_dist), F(lens_u), F(lens_v)
    s = focus_dist / focal_len
    out_du = du * s
    out_dv = dv * s
    out_tl = (tl - pos) * s + pos
    ru = F(1.0) / np.sqrt((du[0] * du[0] + du[1] * du[1]) + du[2] * du[2])
    rv = F(1.0) / np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
    eu, ev = du * ru, dv * rv
    out_pos = (eu * lens_u + ev * lens_v) + pos
    out = np.concatenate([out_pos, out_tl, out_du, out_dv])
    assert out.dtype == F
    return out


def lens_offsets(aperture, n):
    """the golden-angle spiral of lens_cameras: r = aperture * sqrt((i + 0.5) / n), theta = i * 2.39996323, as float32 pairs"""
    i = np.arange(n, dtype=np.float64)
    r = float(aperture) * np.sqrt((i + 0.5) / n)
    return np.stack([r * np.cos(i * 2.39996323), r * np.sin(i * 2.39996323)], axis=1).astype(F)
