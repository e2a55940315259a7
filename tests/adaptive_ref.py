"""The yardstick of the per-pixel sample budgets and the adaptive sampling loop (include/rt_amd.h: rt_render_budget, rt_adaptive_plan_device,
rt_render_adaptive): the definitions restated in NumPy float32 over the CPU oracle's own renderer (orc.Scene.render).  No product code.
Every array is binary32, so every NumPy operation below is rounded to binary32 once, in the header's order; nothing is fused."""
import numpy as np

F = np.float32
CANON_NAN = np.uint32(0x7FC00000)
# rt_adaptive_params_default (include/rt_amd.h), restated: tests/test_adaptive_abi.py holds the library to them
DEFAULTS = dict(pilot_spp=8, step_spp=16, max_spp=512, max_passes=16, threshold=0.05, pixel_threshold=np.inf, floor=0.01)


def wrap32(t):
    """a seed as the 32-bit integer the entry points take"""
    t &= 0xFFFFFFFF
    return t - (1 << 32) if t >= (1 << 31) else t


def canon(a):
    """a NaN becomes the canonical quiet NaN"""
    a = np.ascontiguousarray(a, F).copy()
    a.view(np.uint32)[np.isnan(a)] = CANON_NAN
    return a


def pixel_means(oracle, cam, W, H, budget, limit, sky, time_ms, antialias=True):
    """c [H, W, 3]: for a pixel of budget n > 0 the pixel the oracle renders at spp = n (frame 0, this seed); 0 elsewhere.  One oracle render
    per distinct n, restricted to the rows that hold it."""
    c = np.zeros((H, W, 3), F)
    for n in np.unique(budget):
        if n == 0:
            continue
        rows = np.flatnonzero((budget == n).any(axis=1))
        img = oracle.render(cam, W, H, int(n), limit, sky, time_ms=time_ms, frame_num=0, antialias=antialias, y0=int(rows[0]), y1=int(rows[-1]) + 1)
        sel = budget == n
        c[sel] = img[sel]
    return c


def fold(c, budget, frame, count):
    """the fold of rt_render_budget_device: -> (frame, count) after the call; frame / count None: nothing accumulated yet (count NULL)"""
    budget = np.asarray(budget)
    H, W = budget.shape
    out = np.zeros((H, W, 3), F) if frame is None else np.ascontiguousarray(frame, F).copy()
    m = np.zeros((H, W), np.uint32) if count is None else np.asarray(count, np.uint32)
    n = budget.astype(np.uint32)
    nf, mf, tf = n.astype(F)[..., None], m.astype(F)[..., None], (n + m).astype(F)[..., None]
    with np.errstate(all="ignore"):
        mixed = (c * nf + out * mf) / tf
    new = np.where((m == 0)[..., None], c, mixed).astype(F)
    touched = n > 0
    out[touched] = canon(new)[touched]
    return out, (m + n).astype(np.uint32)


def budget_render(oracle, cam, W, H, budget, limit, sky, time_ms, frame=None, count=None, antialias=True, tile_list=None):
    """rt_render_budget_device.  tile_list: only the pixels of these 8x8 tiles are considered"""
    budget = np.asarray(budget, np.uint16)
    if tile_list is not None:
        tiles_x = (W + 7) // 8
        mask = np.zeros((H, W), bool)
        for g in tile_list:
            ty, tx = divmod(int(g), tiles_x)
            mask[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
        budget = np.where(mask, budget, 0).astype(np.uint16)
    c = pixel_means(oracle, cam, W, H, budget, limit, sky, time_ms, antialias)
    return fold(c, budget, frame, count)


def tiles_of(plane, fill=0):
    """[H, W] -> [tiles, 64]: the 8x8 tiles in image order, slot = row * 8 + column, slots outside the image `fill`"""
    H, W = plane.shape
    ty, tx = (H + 7) // 8, (W + 7) // 8
    p = np.full((ty * 8, tx * 8), fill, plane.dtype)
    p[:H, :W] = plane
    return p.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)


def butterfly_sum(v):
    """[tiles, 64] -> [tiles, 64]: v[i] = v[i] + v[i ^ 1], then ^ 2, ... ^ 32: every slot ends with the same bits"""
    v = np.ascontiguousarray(v, F)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for k in (1, 2, 4, 8, 16, 32):
            v = v + v[:, idx ^ k]
    return v


def tree_sum(v):
    """[tiles, 64] -> [tiles]: the explicit pairwise tree: neighbours, then pairs of pairs, ..."""
    v = np.ascontiguousarray(v, F)
    with np.errstate(all="ignore"):
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def pixel_error(A, B, floor):
    A, B = np.asarray(A, F), np.asarray(B, F)
    with np.errstate(all="ignore"):
        I = (A + B) * F(0.5)
        d = np.abs(A - B)
        num = (d[..., 0] + d[..., 1]) + d[..., 2]
        s = (I[..., 0] + I[..., 1]) + I[..., 2]
        e = num / np.sqrt(np.where(s > F(floor), s, F(floor)).astype(F))
    return np.where(np.isnan(e), F(0.0), e).astype(F)


def plan(A, B, count, step_spp, max_spp, threshold, pixel_threshold, floor, **_):
    """rt_adaptive_plan_device: -> budget [H, W] uint16, tile_error [tiles] float32, tile_active [tiles] uint32, and e [H, W]"""
    count = np.asarray(count, np.uint32)
    H, W = count.shape
    e = pixel_error(A, B, floor)
    inside = tiles_of(np.ones((H, W), bool), False)
    with np.errstate(all="ignore"):
        E = (butterfly_sum(tiles_of(e))[:, 0] / inside.sum(axis=1).astype(F)).astype(F)
        tiles_x = (W + 7) // 8
        E_px = E.reshape(-1, tiles_x)[np.arange(H)[:, None] // 8, np.arange(W)[None, :] // 8]
        active = (count < np.uint32(max_spp)) & ((E_px > F(threshold)) | (e > F(pixel_threshold)))
    left = np.uint32(max_spp) - np.minimum(count, np.uint32(max_spp))
    budget = np.where(active, np.minimum(np.uint32(step_spp), left), 0).astype(np.uint16)
    return budget, E, tiles_of(active, False).sum(axis=1).astype(np.uint32), e


def tile_list_of(tile_error, tile_active):
    """the pass's tile list: the tiles with an active pixel by decreasing error, ties by the lower index"""
    idx = [int(t) for t in np.flatnonzero(tile_active)]
    return sorted(idx, key=lambda t: (-float(tile_error[t]), t))


def render_adaptive(oracle, cam, W, H, limit, sky, time_ms, params, antialias=True):
    """rt_render_adaptive: -> frame [H, W, 3], count [H, W] uint32 (both half buffers), stats, and the half buffers (A, B, count in each)"""
    p = dict(DEFAULTS, **params)
    pilot = np.full((H, W), p["pilot_spp"], np.uint16)
    A, count = budget_render(oracle, cam, W, H, pilot, limit, sky, wrap32(time_ms), antialias=antialias)
    B, _ = budget_render(oracle, cam, W, H, pilot, limit, sky, wrap32(time_ms + 1), antialias=antialias)
    stats = {"passes": 0, "active_tiles": []}
    for k in range(1, p["max_passes"] + 1):
        budget, E, n_active, _ = plan(A, B, count, **p)
        tl = tile_list_of(E, n_active)
        if not tl:
            break
        A, count_after = budget_render(oracle, cam, W, H, budget, limit, sky, wrap32(time_ms + 2 * k), A, count, antialias, tl)
        B, _ = budget_render(oracle, cam, W, H, budget, limit, sky, wrap32(time_ms + 2 * k + 1), B, count, antialias, tl)
        count = count_after
        stats["passes"] = k
        stats["active_tiles"].append(len(tl))
    with np.errstate(all="ignore"):
        frame = canon((A + B) * F(0.5))
    stats["total_samples"] = int(2 * count.astype(np.uint64).sum())
    return frame, (2 * count).astype(np.uint32), stats, (A, B, count)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
