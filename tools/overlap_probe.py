"""Measurements of the box-overlap queries on the GPU, written as overlap_probe.json into the next unused profiles/rNN/ (or --out-dir):

  per scene (monkey, soup6k, sphere50k), 4,194,304 seeded incoherent boxes - centres uniform in twice the scene's triangle bounds, cubes
  of 0.1 %, 1 % and 10 % of the bounds' diagonal (e01, e1, e10):
    count_*, k8_*, any_*     overlap_boxes_device in count-only mode, with k = 8 (ids and counts) and in any-only mode: the kernel's ms
                             (rt_last_kernel_ms), Mboxes/s, and the share of boxes that touch something / the mean count
    nearest                  nearest_points_device on the boxes' centres: the closest thing a caller had (thresholded at the half diagonal
                             it is a superset of the touching boxes, and names one triangle, not all)
    brute_*                  a torch brute force of the same 13-axis test over the flattened triangle records (no tree, no path rule, no
                             spheres), at the largest number of boxes whose [boxes, triangles] temporaries stay within --brute-elems
                             elements, timed with events and scaled to all boxes by proportion.  Its counts, with the scene's spheres
                             added by an untimed torch sphere test (every probe scene stands on a sphere of radius 100, which the
                             kernel counts), are set against the kernel's: the share of boxes on which they are equal, and the
                             number on which the brute force has FEWER (none: the path rule can only take away)
  voxelize of the monkey at 128^3 and 256^3 (any-only kernel ms, and the wall time of the call with its uploads) against distance_grid at
  the cell centres thresholded at the half diagonal (the nearest kernel's ms): the latter is a SUPERSET of the surface cells, not the same
  answer; both cell counts are reported.
  The legs alternate, `--reps` rounds after a warm-up; medians and min / max of each.

    python tools/overlap_probe.py [--boxes 4194304] [--reps 5] [--out-dir DIR]
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


def next_profile_dir():
    used = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return os.path.join(ROOT, "profiles", "r%02d" % (max(used, default=0) + 1))


def brute_counts(torch, tris, lo, hi):
    """the bare 13-axis test in torch float32: tris [T, 12], lo, hi [m, 3] -> counts [m]"""
    ax, ay, az, s1x, s1y, s1z, s2x, s2y, s2z = (tris[None, :, k] for k in range(9))
    bx, by, bz, cx, cy, cz = ax + s1x, ay + s1y, az + s1z, ax + s2x, ay + s2y, az + s2z
    c, h = lo * 0.5 + hi * 0.5, hi * 0.5 - lo * 0.5
    lox, loy, loz, hix, hiy, hiz = (a[:, k:k + 1] for a in (lo, hi) for k in range(3))
    ccx, ccy, ccz, hx, hy, hz = (a[:, k:k + 1] for a in (c, h) for k in range(3))
    sep = ((ax > hix) & (bx > hix) & (cx > hix)) | ((ax < lox) & (bx < lox) & (cx < lox))
    sep |= ((ay > hiy) & (by > hiy) & (cy > hiy)) | ((ay < loy) & (by < loy) & (cy < loy))
    sep |= ((az > hiz) & (bz > hiz) & (cz > hiz)) | ((az < loz) & (bz < loz) & (cz < loz))
    v = [(ax - ccx, ay - ccy, az - ccz), (bx - ccx, by - ccy, bz - ccz), (cx - ccx, cy - ccy, cz - ccz)]
    nx, ny, nz = s1y * s2z - s1z * s2y, s1z * s2x - s1x * s2z, s1x * s2y - s1y * s2x
    d = (nx * v[0][0] + ny * v[0][1]) + nz * v[0][2]
    r = (hx * nx.abs() + hy * ny.abs()) + hz * nz.abs()
    sep |= (d > r) | (d < -r)

    def axis(p, rad):
        return ((p[0] > rad) & (p[1] > rad) & (p[2] > rad)) | ((p[0] < -rad) & (p[1] < -rad) & (p[2] < -rad))
    for fx, fy, fz in ((s1x, s1y, s1z), (s2x - s1x, s2y - s1y, s2z - s1z), (-s2x, -s2y, -s2z)):
        sep |= axis([w[2] * fy - w[1] * fz for w in v], hy * fz.abs() + hz * fy.abs())
        sep |= axis([w[0] * fz - w[2] * fx for w in v], hx * fz.abs() + hz * fx.abs())
        sep |= axis([w[1] * fx - w[0] * fy for w in v], hx * fy.abs() + hy * fx.abs())
    return (~sep).sum(dim=1, dtype=torch.int32)


def sphere_counts(torch, c, r, lo, hi):
    """the sphere test in torch float32: c [S, 3], r [S], lo, hi [m, 3] -> counts [m] (every probe scene stands on a sphere of radius 100)"""
    cs, l, h = c[None, :, :], lo[:, None, :], hi[:, None, :]
    e = torch.clamp(torch.maximum(l - cs, cs - h), min=0.0)
    g = torch.maximum(cs - l, h - cs)
    dmin2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    dmax2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    rr = (r * r)[None, :]
    return ((dmin2 <= rr) & (dmax2 >= rr)).sum(dim=1, dtype=torch.int32)


def summary(xs):
    return {"kernel_ms": xs, "kernel_ms_median": statistics.median(xs), "kernel_ms_min": min(xs), "kernel_ms_max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--brute-elems", type=int, default=1 << 24)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("ray-tracer_amd")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nearest_ref as R
    dev = torch.device("cuda:0")
    ctx = rt.Context(0)
    models = rt.scenes.models_dir()
    n = args.boxes
    out = {"tool": "overlap_probe", "version": rt.lib().rt_version().decode(), "boxes": n, "reps": args.reps, "brute_elems": args.brute_elems, "scenes": {}}
    rng = np.random.default_rng(79)
    unit = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).to(dev)
    t_ids = torch.empty((n, 8, 8), dtype=torch.uint8, device=dev)
    t_cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    t_any = torch.empty((n,), dtype=torch.uint8, device=dev)
    t_near = torch.empty((n, rt.NearestRecord.itemsize), dtype=torch.uint8, device=dev)
    for name in ("monkey", "soup6k", "sphere50k"):
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        so = rt.SceneObjects(objs, models)
        flat = so.debug_flatten()
        sc = ctx.commit(so)
        _, _, tris, _ = R.sections(flat)
        corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        diag = float(np.linalg.norm(hi - lo))
        mid, half = torch.from_numpy((lo + hi) / 2).to(dev), torch.from_numpy(hi - lo).to(dev)
        centre = (mid + unit * half).contiguous()                    # twice the bounds: the centre +- the full extent
        extents = {"e01": 0.001 * diag, "e1": 0.01 * diag, "e10": 0.1 * diag}
        b_lo = {k: (centre - 0.5 * e).contiguous() for k, e in extents.items()}
        b_hi = {k: (centre + 0.5 * e).contiguous() for k, e in extents.items()}
        d_tris = torch.from_numpy(np.ascontiguousarray(tris)).to(dev)
        balls = [ob for ob in flat["objects"] if int(ob["type"]) == R.OBJ_SPHERE]
        d_sc = torch.tensor([[float(x) for x in ob["v"][0:3]] for ob in balls], dtype=torch.float32, device=dev).reshape(-1, 3)
        d_sr = torch.tensor([float(ob["v"][3]) for ob in balls], dtype=torch.float32, device=dev).reshape(-1)
        m = max(1, min(n, args.brute_elems // max(1, tris.shape[0])))
        torch.cuda.synchronize()

        def count(k):
            rt.overlap_boxes_device(sc, b_lo[k], b_hi[k], 0, counts=t_cnt)
            return ctx.last_kernel_ms()

        def k8(k):
            rt.overlap_boxes_device(sc, b_lo[k], b_hi[k], 8, ids=t_ids, counts=t_cnt)
            return ctx.last_kernel_ms()

        def any_only(k):
            rt.overlap_boxes_device(sc, b_lo[k], b_hi[k], 0, any=t_any)
            return ctx.last_kernel_ms()

        def nearest():
            rt.nearest_points_device(ctx, sc, centre, None, out=t_near)
            return ctx.last_kernel_ms()

        def brute(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            c = brute_counts(torch, d_tris, b_lo[k][:m], b_hi[k][:m])
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * (n / m), c

        legs = {}
        for k in extents:
            legs["count_" + k] = (lambda k=k: count(k))
            legs["k8_" + k] = (lambda k=k: k8(k))
            legs["any_" + k] = (lambda k=k: any_only(k))
        legs["nearest"] = nearest
        for f in legs.values():
            f(); f()
        for k in extents:
            brute(k)
        ms = {k: [] for k in legs}
        brutes = {"brute_" + k: [] for k in extents}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
            for k in extents:
                brutes["brute_" + k].append(brute(k)[0])
        info = sc.info()
        row = {"triangles": int(tris.shape[0]), "placement": info["scene_in_lds"], "threads": info["threads_per_block"], "diagonal": diag, "extents": extents,
               "brute_boxes": m}
        for k in extents:
            count(k)
            torch.cuda.synchronize()
            row["outcome_" + k] = {"touching": float((t_cnt > 0).float().mean()), "mean_count": float(t_cnt.float().mean()), "max_count": int(t_cnt.max())}
            # the timed brute force covers the triangle records alone; with the scene's spheres added (untimed) its counts are the kernel's,
            # but for the path rule - which can only take a triangle away
            agree = brute(k)[1] + sphere_counts(torch, d_sc, d_sr, b_lo[k][:m], b_hi[k][:m])
            row["outcome_" + k]["brute_with_spheres_equal_share"] = float((agree == t_cnt[:m]).float().mean())
            row["outcome_" + k]["brute_with_spheres_below_kernel"] = int((agree < t_cnt[:m]).sum())
        for k in legs:
            row[k] = summary(ms[k])
            row[k]["mboxes_per_s"] = n / row[k]["kernel_ms_median"] / 1e3
        for k, xs in brutes.items():
            row[k] = {"scaled_ms": xs, "scaled_ms_median": statistics.median(xs), "scaled_ms_min": min(xs), "scaled_ms_max": max(xs)}
            row[k]["brute_over_count"] = row[k]["scaled_ms_median"] / row["count_" + k[6:]]["kernel_ms_median"]
        for k in extents:
            row["any_over_count_" + k] = row["any_" + k]["kernel_ms_median"] / row["count_" + k]["kernel_ms_median"]
            row["count_over_nearest_" + k] = row["count_" + k]["kernel_ms_median"] / row["nearest"]["kernel_ms_median"]
        out["scenes"][name] = row
        if name == "monkey":
            vox = {}
            pad = 0.02 * (hi - lo)
            g_lo, g_hi = lo - pad, hi + pad
            for size in (128, 256):
                shape = (size, size, size)
                cell = (g_hi - g_lo) / size
                half_diag = 0.5 * float(np.linalg.norm(cell))
                c_lo, c_hi = g_lo + 0.5 * cell, g_hi - 0.5 * cell          # distance_grid's lattice: the cell centres
                v_ms, v_wall, d_ms, d_wall = [], [], [], []
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    cells = rt.voxelize(sc, g_lo, g_hi, shape)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    kv = ctx.last_kernel_ms()
                    dist, _ = rt.distance_grid(sc, c_lo, c_hi, shape)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    kd = ctx.last_kernel_ms()
                    if rep:
                        v_ms.append(kv); v_wall.append((t1 - t0) * 1e3); d_ms.append(kd); d_wall.append((t2 - t1) * 1e3)
                near = dist <= half_diag
                vox[str(size)] = {"cells": size ** 3, "half_diagonal": half_diag, "voxelize": summary(v_ms), "voxelize_wall_ms_median": statistics.median(v_wall),
                                  "distance_grid": summary(d_ms), "distance_grid_wall_ms_median": statistics.median(d_wall),
                                  "surface_cells": int(cells.sum()), "thresholded_cells": int(near.sum()), "surface_not_in_thresholded": int((cells & ~near).sum()),
                                  "voxelize_over_distance_grid": statistics.median(v_ms) / statistics.median(d_ms)}
                del cells, dist, near
            out["voxelize_monkey"] = vox
        del sc
    out_dir = args.out_dir or next_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "overlap_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
