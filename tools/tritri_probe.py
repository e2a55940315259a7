"""Measurements of the triangle-overlap queries on the GPU, written as tritri_probe.json into the next unused profiles/rNN/ (or --out-dir):

  per scene (monkey, soup6k, sphere50k), 4,194,304 seeded incoherent query triangles - centres uniform in twice the scene's triangle
  bounds, the three vertices the centre plus offsets uniform in +- half of 0.1 %, 1 % and 10 % of the bounds' diagonal per component
  (s01, s1, s10):
    count_*, k8_*, any_*, seg_*   overlap_triangles_device in count-only mode, with k = 8 (ids and counts), in any-only mode, and with
                             k = 8 and segments: the kernel's ms (rt_last_kernel_ms), Mtriangles/s, the share of queries that cut
                             something / the mean count
    boxes_*                  overlap_boxes_device in count-only mode on the same triangles' bounding boxes: the superset a caller had
                             before (same build, same scene); its mean count beside the triangles'
    brute_*                  a torch brute force of the same test over the flattened triangle records (no tree, no path rule, no
                             spheres; a coplanar pair, which chance does not draw, goes through the intervals like any other), at the
                             largest number of queries whose [queries, triangles] temporaries stay within --brute-elems elements,
                             timed with events and scaled to all queries by proportion.  Its counts are set against the kernel's with
                             the spheres' share taken off (the kernel's count of the same queries on the scene's spheres alone is not
                             separable, so the comparison is made on the queries whose kernel any-byte on a spheres-only copy of the
                             scene is 0): the share on which they are equal
  The legs alternate, `--reps` rounds after a warm-up; medians and min / max of each.

    python tools/tritri_probe.py [--triangles 4194304] [--reps 5] [--out-dir DIR]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from overlap_probe import next_profile_dir, summary  # noqa: E402


def brute_counts(torch, tris, q):
    """the definition's steps 1 to 3 and 5 in torch float32: tris [T, 12], q [m, 9] -> counts [m]"""
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    sub = lambda a, b: (a[0] - b[0], a[1] - b[1], a[2] - b[2])
    a = [tuple(q[:, 3 * i + c:3 * i + c + 1] for c in range(3)) for i in range(3)]
    p0, s1, s2 = (tuple(tris[None, :, 3 * j + c] for c in range(3)) for j in range(3))
    qv = [p0, tuple(p0[c] + s1[c] for c in range(3)), tuple(p0[c] + s2[c] for c in range(3))]
    ok = None
    for c in range(3):
        lo = torch.minimum(torch.minimum(a[0][c], a[1][c]), a[2][c])
        hi = torch.maximum(torch.maximum(a[0][c], a[1][c]), a[2][c])
        sep = ((qv[0][c] > hi) & (qv[1][c] > hi) & (qv[2][c] > hi)) | ((qv[0][c] < lo) & (qv[1][c] < lo) & (qv[2][c] < lo))
        ok = ~sep if ok is None else ok & ~sep
    z, e1, e2 = sub(a[0], a[0]), sub(a[1], a[0]), sub(a[2], a[0])
    na, nb = cross(e1, e2), cross(s1, s2)
    hA = [dot(nb, sub(a[i], p0)) for i in range(3)]
    d = [sub(qv[j], a[0]) for j in range(3)]
    hB = [dot(na, d[j]) for j in range(3)]
    for h in (hA, hB):
        ok = ok & ~(((h[0] > 0) & (h[1] > 0) & (h[2] > 0)) | ((h[0] < 0) & (h[1] < 0) & (h[2] < 0)))
    D = cross(na, nb)

    def ends(v, h):
        c1, c2, c3, c4 = h[0] * h[1] > 0, h[0] * h[2] > 0, (h[1] * h[2] > 0) | (h[0] != 0), h[1] != 0
        l2 = c1 | (~c2 & ~c3 & ~c4)
        l1 = ~c1 & (c2 | (~c3 & c4))
        l0 = ~l1 & ~l2
        pick = lambda x: torch.where(l0, x[0], torch.where(l1, x[1], x[2]))
        vl, hl = pick(v), pick(h)
        at = lambda vo, ho: torch.where(hl - ho == 0, vl, vl + (vo - vl) * (hl / (hl - ho)))
        return at(torch.where(l0, v[1], v[0]), torch.where(l0, h[1], h[0])), at(torch.where(l0 | l1, v[2], v[1]), torch.where(l0 | l1, h[2], h[1]))
    xA1, xA2 = ends([dot(D, z), dot(D, e1), dot(D, e2)], hA)
    xB1, xB2 = ends([dot(D, d[j]) for j in range(3)], hB)
    a_below = (xA1 < xB1) & (xA1 < xB2) & (xA2 < xB1) & (xA2 < xB2)
    b_below = (xB1 < xA1) & (xB1 < xA2) & (xB2 < xA1) & (xB2 < xA2)
    return (ok & ~(a_below | b_below)).sum(dim=1, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--brute-elems", type=int, default=1 << 23)
    ap.add_argument("--out-dir", default=None)
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("ray-tracer_amd")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nearest_ref as R
    dev = torch.device("cuda:0")
    ctx = rt.Context(0)
    models = rt.scenes.models_dir()
    n = args.triangles
    out = {"tool": "tritri_probe", "version": rt.lib().rt_version().decode(), "triangles": n, "reps": args.reps, "brute_elems": args.brute_elems, "scenes": {}}
    rng = np.random.default_rng(83)
    unit = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 1, 3)).astype(np.float32)).to(dev)
    offs = torch.from_numpy(rng.uniform(-0.5, 0.5, (n, 3, 3)).astype(np.float32)).to(dev)
    t_ids = torch.empty((n, 8, 8), dtype=torch.uint8, device=dev)
    t_seg = torch.empty((n, 8, 32), dtype=torch.uint8, device=dev)
    t_cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    t_box = torch.empty((n,), dtype=torch.int32, device=dev)
    t_any = torch.empty((n,), dtype=torch.uint8, device=dev)
    for name in ("monkey", "soup6k", "sphere50k"):
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        so = rt.SceneObjects(objs, models)
        flat = so.debug_flatten()
        sc = ctx.commit(so)
        balls = ctx.commit(rt.SceneObjects([o for o in objs if o[0] == "sphere"], models))       # the scene's spheres alone: which queries they touch
        _, _, tris, _ = R.sections(flat)
        corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        diag = float(np.linalg.norm(hi - lo))
        mid, half = torch.from_numpy((lo + hi) / 2).to(dev), torch.from_numpy(hi - lo).to(dev)
        centre = mid + unit * half                                   # twice the bounds: the centre +- the full extent
        sizes = {"s01": 0.001 * diag, "s1": 0.01 * diag, "s10": 0.1 * diag}
        q = {k: (centre + offs * s).reshape(n, 9).contiguous() for k, s in sizes.items()}
        b_lo = {k: v.reshape(n, 3, 3).min(dim=1).values.contiguous() for k, v in q.items()}
        b_hi = {k: v.reshape(n, 3, 3).max(dim=1).values.contiguous() for k, v in q.items()}
        d_tris = torch.from_numpy(np.ascontiguousarray(tris)).to(dev)
        m = max(1, min(n, args.brute_elems // max(1, tris.shape[0])))
        torch.cuda.synchronize()

        def count(k):
            rt.overlap_triangles_device(sc, q[k], 0, counts=t_cnt)
            return ctx.last_kernel_ms()

        def k8(k):
            rt.overlap_triangles_device(sc, q[k], 8, ids=t_ids, counts=t_cnt)
            return ctx.last_kernel_ms()

        def any_only(k):
            rt.overlap_triangles_device(sc, q[k], 0, any=t_any)
            return ctx.last_kernel_ms()

        def seg(k):
            rt.overlap_triangles_device(sc, q[k], 8, ids=t_ids, counts=t_cnt, segments=t_seg)
            return ctx.last_kernel_ms()

        def boxes(k):
            rt.overlap_boxes_device(sc, b_lo[k], b_hi[k], 0, counts=t_box)
            return ctx.last_kernel_ms()

        def brute(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            c = brute_counts(torch, d_tris, q[k][:m])
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * (n / m), c

        legs = {}
        for k in sizes:
            legs["count_" + k] = (lambda k=k: count(k))
            legs["k8_" + k] = (lambda k=k: k8(k))
            legs["any_" + k] = (lambda k=k: any_only(k))
            legs["seg_" + k] = (lambda k=k: seg(k))
            legs["boxes_" + k] = (lambda k=k: boxes(k))
        for f in legs.values():
            f(); f()
        for k in sizes:
            brute(k)
        ms = {k: [] for k in legs}
        brutes = {"brute_" + k: [] for k in sizes}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
            for k in sizes:
                brutes["brute_" + k].append(brute(k)[0])
        info = sc.info()
        row = {"triangles": int(tris.shape[0]), "placement": info["scene_in_lds"], "threads": info["threads_per_block"], "diagonal": diag, "sizes": sizes,
               "brute_queries": m}
        for k in sizes:
            count(k)
            boxes(k)
            rt.overlap_triangles_device(balls, q[k], 0, any=t_any)
            torch.cuda.synchronize()
            clear = t_any[:m] == 0
            row["outcome_" + k] = {"cutting": float((t_cnt > 0).float().mean()), "mean_count": float(t_cnt.float().mean()), "max_count": int(t_cnt.max()),
                                   "truncated_at_8": float((t_cnt > 8).float().mean()), "boxes_mean_count": float(t_box.float().mean()),
                                   "ids_not_below_boxes": int((t_cnt > t_box).sum()),
                                   "brute_equal_share": float((brute(k)[1][clear] == t_cnt[:m][clear]).float().mean()), "brute_compared": int(clear.sum())}
        for k in legs:
            row[k] = summary(ms[k])
            row[k]["mqueries_per_s"] = n / row[k]["kernel_ms_median"] / 1e3
        for k, xs in brutes.items():
            s = k[6:]
            row[k] = {"scaled_ms": xs, "scaled_ms_median": statistics.median(xs), "scaled_ms_min": min(xs), "scaled_ms_max": max(xs)}
            row[k]["brute_over_count"] = row[k]["scaled_ms_median"] / row["count_" + s]["kernel_ms_median"]
            # the one expectation: the query beats the brute force by more than both spreads
            gap = row[k]["scaled_ms_median"] - row["count_" + s]["kernel_ms_median"]
            row[k]["beats_brute_by_more_than_both_spreads"] = bool(gap > row[k]["scaled_ms_max"] - row[k]["scaled_ms_min"] and
                                                                   gap > row["count_" + s]["kernel_ms_max"] - row["count_" + s]["kernel_ms_min"])
        for k in sizes:
            c = row["count_" + k]["kernel_ms_median"]
            row["ratios_" + k] = {"k8_over_count": row["k8_" + k]["kernel_ms_median"] / c, "any_over_count": row["any_" + k]["kernel_ms_median"] / c,
                                  "seg_over_k8": row["seg_" + k]["kernel_ms_median"] / row["k8_" + k]["kernel_ms_median"],
                                  "count_over_boxes": c / row["boxes_" + k]["kernel_ms_median"]}
        out["scenes"][name] = row
        del sc, balls
    out_dir = args.out_dir or next_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "tritri_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
