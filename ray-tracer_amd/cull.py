"""The primary-ray cull's test and development hooks (csrc/rt_cull.h): the bit plane a context's last render launch was handed, and the same
plane computed on the host from a flattened scene; the subtree cull's gate words, a word per pixel behind the bits, and the primary entry
words behind those (csrc/rt_entry.h), in the same two forms."""
import ctypes as C

import numpy as np

from ._abi import lib, rt_flat_view
from .objects import Scene

_u32p = C.POINTER(C.c_uint32)
GATE_STATS = ("pixels", "centre_steps", "centre_steps_gated", "pixels_with_dead_gates")
ENTRY_STATS = ("pixels_triangle", "pixels_nothing", "pixels_unknown", "centre_steps_triangle", "centre_steps_nothing", "centre_steps_unknown",
               "centre_tests_triangle", "centre_tests_nothing", "centre_tests_unknown", "triangles_classified")
ENTRY_NOTHING = 2
SUB_WORDS = 64
SUBENTRY_STATS = ("pixels_wanting_table", "tables", "sub_triangle", "sub_nothing", "sub_unknown", "centre_steps_resolved", "centre_steps_all")
STATS = ("root_entering", "flagged_root_entering", "centre_steps_flagged", "centre_steps_root_entering", "flagged", "words")


def plane_words(width, height):
    """rt_cull_words: 32 pixels to a word, whole pairs of words"""
    return ((int(width) * int(height) + 63) // 64) * 2


def plane_bits(words, width, height):
    """a plane's words as a (height, width) array of 0 / 1: pixel py * width + px is bit (pixel & 31) of word pixel >> 5"""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return bits[:int(width) * int(height)].reshape(int(height), int(width))


def primary_cull_plane(ctx):
    """(used, width, height, words): whether the context's last render launch was handed a cull plane, and that plane read back from the device
    (words is None if it was not); waits for the device"""
    info = (C.c_int32 * 4)()
    ctx._check(lib().rt_debug_primary_cull(ctx._h, None, 0, info))
    if not info[0]:
        return False, 0, 0, None
    words = np.zeros(int(info[3]), np.uint32)
    ctx._check(lib().rt_debug_primary_cull(ctx._h, words.ctypes.data_as(_u32p), words.size, info))
    return True, int(info[1]), int(info[2]), words


def primary_cull_host(scene, camera, antialias=True):
    """(words, stats) of the predicate evaluated on the host, per pixel of `camera`'s image, on a SceneObjects (its flattened layout) or a committed
    Scene (what is on the device now: waits for it).  Needs no GPU for a SceneObjects."""
    v = rt_flat_view()
    if isinstance(scene, Scene):
        scene.ctx._check(lib().rt_debug_scene_read(scene.ctx._h, scene._h, C.byref(v)))
    else:
        scene._check(lib().rt_debug_flatten(scene._h, C.byref(v)))
    words = np.zeros(plane_words(camera.c.width, camera.c.height), np.uint32)
    stats = (C.c_int64 * 6)()
    st = lib().rt_debug_primary_cull_host(C.byref(v), C.byref(camera.c), 1 if antialias else 0, words.ctypes.data_as(_u32p), stats)
    if st != 0:
        raise ValueError("rt_debug_primary_cull_host refused its arguments (status %d)" % st)
    return words, dict(zip(STATS, (int(x) for x in stats)))


def subtree_cull_words(ctx):
    """(used, words): whether the context's last render launch was handed a cull plane, and the gate words behind it read back from the device as a
    (height, width) array (None if it was not): bit g set iff gate g is dead for the pixel's primary rays; waits for the device"""
    info = (C.c_int32 * 4)()
    ctx._check(lib().rt_debug_subtree_cull(ctx._h, None, 0, info))
    if not info[0]:
        return False, None
    words = np.zeros(int(info[3]), np.uint32)
    ctx._check(lib().rt_debug_subtree_cull(ctx._h, words.ctypes.data_as(_u32p), words.size, info))
    return True, words.reshape(int(info[2]), int(info[1]))


def subtree_cull_host(scene, camera, antialias=True):
    """(words, stats) of rt_cull_gate_word evaluated on the host per pixel of `camera`'s image, words as a (height, width) array; `scene` as for
    primary_cull_host.  Needs no GPU for a SceneObjects."""
    v = rt_flat_view()
    if isinstance(scene, Scene):
        scene.ctx._check(lib().rt_debug_scene_read(scene.ctx._h, scene._h, C.byref(v)))
    else:
        scene._check(lib().rt_debug_flatten(scene._h, C.byref(v)))
    words = np.zeros(int(camera.c.width) * int(camera.c.height), np.uint32)
    stats = (C.c_int64 * 4)()
    st = lib().rt_debug_subtree_cull_host(C.byref(v), C.byref(camera.c), 1 if antialias else 0, words.ctypes.data_as(_u32p), stats)
    if st != 0:
        raise ValueError("rt_debug_subtree_cull_host refused its arguments (status %d)" % st)
    return words.reshape(int(camera.c.height), int(camera.c.width)), dict(zip(GATE_STATS, (int(x) for x in stats)))


def primary_entry_words(ctx):
    """(used, words): whether the context's last render launch was handed a cull plane, and the entry words behind it read back from the device as a
    (height, width) array (None if it was not): T << 1 | 1 - every primary ray of the pixel ends on triangle T -, ENTRY_NOTHING or 0; waits for
    the device"""
    info = (C.c_int32 * 4)()
    ctx._check(lib().rt_debug_primary_entry(ctx._h, None, 0, info))
    if not info[0]:
        return False, None
    words = np.zeros(int(info[3]), np.uint32)
    ctx._check(lib().rt_debug_primary_entry(ctx._h, words.ctypes.data_as(_u32p), words.size, info))
    return True, words.reshape(int(info[2]), int(info[1]))


def primary_entry_host(scene, camera, antialias=True):
    """(words, stats) of rt_entry_word evaluated on the host per pixel of `camera`'s image, words as a (height, width) array; `scene` as for
    primary_cull_host.  Needs no GPU for a SceneObjects."""
    v = rt_flat_view()
    if isinstance(scene, Scene):
        scene.ctx._check(lib().rt_debug_scene_read(scene.ctx._h, scene._h, C.byref(v)))
    else:
        scene._check(lib().rt_debug_flatten(scene._h, C.byref(v)))
    words = np.zeros(int(camera.c.width) * int(camera.c.height), np.uint32)
    stats = (C.c_int64 * 12)()
    st = lib().rt_debug_primary_entry_host(C.byref(v), C.byref(camera.c), 1 if antialias else 0, words.ctypes.data_as(_u32p), stats)
    if st != 0:
        raise ValueError("rt_debug_primary_entry_host refused its arguments (status %d)" % st)
    return words.reshape(int(camera.c.height), int(camera.c.width)), dict(zip(ENTRY_STATS, (int(x) for x in stats)))


def primary_subentry_tables(ctx):
    """(refined, pixels, words): whether the context's last render launch was handed a plane whose view has its sub-entry tables (csrc/rt_entry.h),
    and those tables read back from the device keyed by pixel, in ascending order: pixels[i] = py * width + px, words[i, idx] the sub-word of
    sub-box idx = jx + 4 jy + 16 jz - T << 1 | 1, ENTRY_NOTHING or 0 (both None if it was not); waits for the device"""
    info = (C.c_int32 * 4)()
    ctx._check(lib().rt_debug_primary_subentry(ctx._h, None, None, 0, info))
    if not info[0]:
        return False, None, None
    n = int(info[3])
    pixels, words = np.zeros(n, np.uint32), np.zeros((n, SUB_WORDS), np.uint32)
    ctx._check(lib().rt_debug_primary_subentry(ctx._h, pixels.ctypes.data_as(_u32p), words.ctypes.data_as(_u32p), n, info))
    return True, pixels[:int(info[3])], words[:int(info[3])]


def primary_subentry_host(scene, camera, antialias=True, cap=-1):
    """(pixels, words, stats) of the sub-entry tables computed on the host as the refinement writes them, keyed by pixel in ascending order; cap:
    at most that many tables (the first pixels in order), -1 for what the image's allocation holds; `scene` as for primary_cull_host.  Needs no
    GPU for a SceneObjects."""
    v = rt_flat_view()
    if isinstance(scene, Scene):
        scene.ctx._check(lib().rt_debug_scene_read(scene.ctx._h, scene._h, C.byref(v)))
    else:
        scene._check(lib().rt_debug_flatten(scene._h, C.byref(v)))
    stats = (C.c_int64 * 8)()
    st = lib().rt_debug_primary_subentry_host(C.byref(v), C.byref(camera.c), 1 if antialias else 0, int(cap), None, None, 0, stats)
    if st != 0:
        raise ValueError("rt_debug_primary_subentry_host refused its arguments (status %d)" % st)
    n = int(stats[1])
    pixels, words = np.zeros(n, np.uint32), np.zeros((n, SUB_WORDS), np.uint32)
    if n:
        st = lib().rt_debug_primary_subentry_host(C.byref(v), C.byref(camera.c), 1 if antialias else 0, int(cap), pixels.ctypes.data_as(_u32p), words.ctypes.data_as(_u32p), n, stats)
        if st != 0:
            raise ValueError("rt_debug_primary_subentry_host refused its arguments (status %d)" % st)
    return pixels, words, dict(zip(SUBENTRY_STATS, (int(x) for x in stats)))
