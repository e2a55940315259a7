"""Reads tests/golden/ref/ (the fixtures tools/make_reference_golden.py recorded from the reference's own programs)
for test_reference_pin.py and test_gpu_reference.py.  Nothing here needs the reference or oracle/_ref."""
import json
import os

import numpy as np

from conftest import GOLDEN

REF = os.path.join(GOLDEN, "ref")
HIT, OBJECT, DIST, POINT, NORMAL, UV = 0, 1, 2, slice(3, 6), slice(6, 9), slice(9, 11)      # columns of records() (uint32 words)

_meta = None


def meta():
    global _meta
    if _meta is None:
        with open(os.path.join(REF, "meta.json")) as f:
            _meta = json.load(f)
    return _meta


def load(name):
    return np.load(os.path.join(REF, name))


def _decode(x):
    if isinstance(x, dict):
        return load(x["npy"])
    if isinstance(x, list):
        return [_decode(v) for v in x]
    return x


def scene(rt, entry):
    """(objects, sky) of a frame or hit fixture.  The reference's own scenes 0-3 are taken from rt.scenes' transcriptions of
    src/main.cu - the fixture was rendered from the reference's SceneObjects(n), so this is what checks the transcription;
    every other scene is the description the fixture itself was rendered from."""
    if entry["builtin"] is not None:
        return rt.scenes.CONFIG_SCENES["reference_scene%d" % entry["builtin"]]()
    s = meta()["scenes"][entry["scene"]]
    return _decode(s["objects"]), tuple(s["sky"])


def frames(entry):
    """the fixture's frames as [n, H, W, 3]"""
    a = load(entry["file"])
    return a if a.ndim == 4 else a[None]


def need_uv(objs):
    """per object: does its material ask for texture coordinates (the generator's rule, carried by meta.json)"""
    kinds = tuple(meta()["uv_materials"])
    return np.array([o[-1][0] in kinds for o in objs])


def records(entry):
    """a hit fixture as one row of 11 uint32 words per ray: hit flag, object, distance, point, normal, u, v.  The file holds the
    hits' rows with the ray's index in the first column; a miss is the reference's record for one: no hit, the distance INF
    (meta.json miss_distance) - here with object -1 and zeros where the reference assigns nothing"""
    stored = load(entry["file"])
    rec = np.zeros((entry["rays"], 11), np.uint32)
    rec[:, OBJECT] = np.uint32(0xFFFFFFFF)
    rec[:, DIST] = np.float32(meta()["miss_distance"]).view(np.uint32)
    idx = stored[:, 0].astype(np.int64)
    assert len(np.unique(idx)) == len(idx) and idx.max() < entry["rays"]
    rec[idx] = stored
    rec[idx, HIT] = 1
    return rec


def rays():
    """origins[4096, 3], directions[4096, 3]: the 2,048 primary rays of the coarse pixel grid, then the 2,048 random ones"""
    p = meta()["rays_primary"]
    d = load(p["directions"])
    r = load(meta()["rays_random"]["file"])
    o = np.broadcast_to(np.asarray(p["origin"], np.float32), d.shape)
    return np.ascontiguousarray(np.concatenate([o, r[:, 0:3]])), np.ascontiguousarray(np.concatenate([d, r[:, 3:6]]))


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)
