"""Measurements of the nearest-surface queries on the GPU, written as nearest_probe.json into the next unused profiles/rNN/ (or --out-dir):

  per scene (monkey, soup6k, sphere50k), 4,194,304 seeded points uniform in twice the scene's triangle bounds:
    nearest          nearest_points_device without limits: kernel ms (rt_last_kernel_ms), Mpoints/s
    nearest_limited  ... with a limit of a tenth of the bounds' diagonal for every point, and the fraction of points that still find a surface
    query            the closest-hit query (trace_rays_device) on as many seeded rays: for scale
    brute_force      what a caller has without the entry point: a torch float32 evaluation of every triangle record and sphere for every
                     point on the same GPU (the same region test, n x T temporaries), at the largest n that fits a fixed budget of
                     temporaries; ms per call on the host clock around a device synchronise, and ms per 2^22 points by proportion
  The three library legs alternate, `--reps` rounds after a warm-up; medians and min / max of each.

    python tools/nearest_probe.py [--points 4194304] [--reps 5] [--out-dir DIR]
"""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BRUTE_ELEMENTS = 1 << 26            # n x T of the brute force: ~40 float32 temporaries of that size are alive at its peak (~10 GB)


def next_profile_dir():
    used = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return os.path.join(ROOT, "profiles", "r%02d" % (max(used, default=0) + 1))


def torch_brute_force(torch, tris, spheres, p):
    """min over every triangle record [T, 9] and sphere [S, 4] of the squared distance from p [n, 3]: -> (dist2 [n], index [n])"""
    a, b, c = tris[None, :, 0:3], tris[None, :, 3:6], tris[None, :, 6:9]
    ap = p[:, None, :] - a
    bp, cp = ap - b, ap - c
    d1, d2, d3, d4, d5, d6 = (b * ap).sum(-1), (c * ap).sum(-1), (b * bp).sum(-1), (c * bp).sum(-1), (b * cp).sum(-1), (c * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    k = 1.0 / (va + vb + vc)
    v, w = vb * k, vc * k
    e, f = d4 - d3, d5 - d6
    zero, one = torch.zeros_like(v), torch.ones_like(v)
    m = (va <= 0) & (e >= 0) & (f >= 0)
    wbc = e / (e + f)
    v, w = torch.where(m, 1.0 - wbc, v), torch.where(m, wbc, w)
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    v, w = torch.where(m, zero, v), torch.where(m, d2 / (d2 - d6), w)
    m = (d6 >= 0) & (d5 <= d6)
    v, w = torch.where(m, zero, v), torch.where(m, one, w)
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    v, w = torch.where(m, d1 / (d1 - d3), v), torch.where(m, zero, w)
    m = (d3 >= 0) & (d4 <= d3)
    v, w = torch.where(m, one, v), torch.where(m, zero, w)
    m = (d1 <= 0) & (d2 <= 0)
    v, w = torch.where(m, zero, v), torch.where(m, zero, w)
    r = ap - (b * v[..., None] + c * w[..., None])
    dist2 = torch.nan_to_num((r * r).sum(-1), nan=float("inf"))
    if spheres.shape[0]:
        s = torch.linalg.norm(p[:, None, :] - spheres[None, :, 0:3], dim=-1) - spheres[None, :, 3]
        dist2 = torch.cat([dist2, s * s], dim=1)
    return dist2.min(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("ray-tracer_amd")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nearest_ref as R
    dev = torch.device("cuda:0")
    ctx = rt.Context(0)
    models = rt.scenes.models_dir()
    n = args.points
    out = {"tool": "nearest_probe", "version": rt.lib().rt_version().decode(), "points": n, "reps": args.reps, "scenes": {}}
    rng = np.random.default_rng(77)
    unit = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).to(dev)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    t_d = torch.from_numpy(d / np.linalg.norm(d, axis=1, keepdims=True)).to(dev)
    t_rec = torch.empty((n, rt.NearestRecord.itemsize), dtype=torch.uint8, device=dev)
    t_hit = torch.empty(n * rt.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    for name in ("monkey", "soup6k", "sphere50k"):
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        so = rt.SceneObjects(objs, models)
        flat = so.debug_flatten()
        sc = ctx.commit(so)
        _, _, tris, objects = R.sections(flat)
        corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        mid, half = torch.from_numpy((lo + hi) / 2).to(dev), torch.from_numpy(hi - lo).to(dev)
        pts = (mid + unit * half).contiguous()                       # twice the bounds: the centre +- the full extent
        limit = float(np.linalg.norm(hi - lo)) / 10.0
        lim = torch.full((n,), limit, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def nearest():
            rt.nearest_points_device(ctx, sc, pts, out=t_rec)
            return ctx.last_kernel_ms()

        def nearest_limited():
            rt.nearest_points_device(ctx, sc, pts, lim, out=t_rec)
            return ctx.last_kernel_ms()

        def query():
            rt.trace_rays_device(ctx, sc, pts.data_ptr(), t_d.data_ptr(), n, t_hit.data_ptr())
            return ctx.last_kernel_ms()

        legs = {"nearest": nearest, "nearest_limited": nearest_limited, "query": query}
        for f in legs.values():
            f(); f()
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
        nearest_limited()
        found = float((t_rec.view(torch.int32).reshape(-1, 8)[:, 5] >= 0).float().mean())
        nearest()
        dist = t_rec.view(torch.float32).reshape(-1, 8)[:, 0].clone()
        # the brute force, at the largest n that fits its budget of temporaries
        T = tris.shape[0]
        n_bf = max(256, min(n, BRUTE_ELEMENTS // max(T, 1)))
        t_tris = torch.from_numpy(np.ascontiguousarray(tris[:, 0:9])).to(dev)
        sph = np.array([o["v"][0:4] for o in objects if o["type"] == R.OBJ_SPHERE], np.float32).reshape(-1, 4)
        t_sph = torch.from_numpy(sph).to(dev)
        bf_ms = []
        for k in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bf_d2, _ = torch_brute_force(torch, t_tris, t_sph, pts[:n_bf])
            torch.cuda.synchronize()
            if k:
                bf_ms.append(1e3 * (time.perf_counter() - t0))
        agree = float((torch.abs(torch.sqrt(bf_d2) - dist[:n_bf]) <= 1e-4 * (1.0 + dist[:n_bf])).float().mean())
        row = {"triangles": int(T), "spheres": int(sph.shape[0]), "placement": sc.info()["scene_in_lds"], "threads": sc.info()["threads_per_block"],
               "limit": limit, "found_within_limit": found, "brute_force": {"n": int(n_bf), "ms": bf_ms, "ms_median": statistics.median(bf_ms),
                                                                            "ms_per_2^22_points_by_proportion": statistics.median(bf_ms) * n / n_bf,
                                                                            "agrees_with_the_library_to_1e-4": agree}}
        for k in legs:
            med = statistics.median(ms[k])
            row[k] = {"kernel_ms": ms[k], "kernel_ms_median": med, "kernel_ms_min": min(ms[k]), "kernel_ms_max": max(ms[k]), "mpoints_per_s": n / med / 1e3}
        row["brute_force_over_nearest"] = row["brute_force"]["ms_per_2^22_points_by_proportion"] / row["nearest"]["kernel_ms_median"]
        row["nearest_over_query"] = row["nearest"]["kernel_ms_median"] / row["query"]["kernel_ms_median"]
        out["scenes"][name] = row
        del sc
    out_dir = args.out_dir or next_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "nearest_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
