"""Measurements of the sphere-cast queries on the GPU, written as sweep_probe.json into the next unused profiles/rNN/ (or --out-dir):

  per scene (monkey, soup6k, sphere50k), 4,194,304 seeded incoherent balls - origins uniform in twice the scene's triangle bounds, unit
  directions uniform on the sphere:
    sweep_r0, sweep_r1, sweep_r10   sweep_spheres_device at r = 0, at 1 % and at 10 % of the bounds' diagonal: the sweep kernel's ms
                                    (rt_last_kernel_ms reports the second of the call's two launches), Mballs/s, and what came of the balls
    query                           the closest-hit query (trace_rays_device) on the same rays: for scale
    nearest_r1, nearest_r10         nearest_points_device on the origins with the radii as limits: what the call's first launch costs
    chain_r1, chain_r10             the conservative-advancement chain a caller had without the entry point: repeated
                                    nearest_points_device launches from the origins, each ball stepped by (distance - r) / |d|, until
                                    every ball is within 1e-4 of the sweep's t, or has passed its limit (the sweep's t, or the time at
                                    which a ball that meets nothing has left the scene's reach), or has stopped moving.  Kernel times only:
                                    the stepping arithmetic between the launches is left out, in the chain's favour.  Launches, and the sum
                                    of their kernel ms.
  The legs alternate, `--reps` rounds after a warm-up; medians and min / max of each.

    python tools/sweep_probe.py [--balls 4194304] [--reps 5] [--out-dir DIR]
"""
import argparse
import importlib
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHAIN_MAX = 256                     # launches of one chain, at most (reported when reached)


def next_profile_dir():
    used = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return os.path.join(ROOT, "profiles", "r%02d" % (max(used, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--balls", type=int, default=1 << 22)
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
    n = args.balls
    out = {"tool": "sweep_probe", "version": rt.lib().rt_version().decode(), "balls": n, "reps": args.reps, "chain_max_launches": CHAIN_MAX, "scenes": {}}
    rng = np.random.default_rng(78)
    unit = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).to(dev)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    t_d = torch.from_numpy(d / np.linalg.norm(d, axis=1, keepdims=True)).to(dev)
    t_rec = torch.empty((n, rt.SweepRecord.itemsize), dtype=torch.uint8, device=dev)
    t_near = torch.empty((n, rt.NearestRecord.itemsize), dtype=torch.uint8, device=dev)
    t_hit = torch.empty(n * rt.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
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
        org = (mid + unit * half).contiguous()                       # twice the bounds: the centre +- the full extent
        radii = {"r0": 0.0, "r1": 0.01 * diag, "r10": 0.1 * diag}
        t_r = {k: torch.full((n,), v, dtype=torch.float32, device=dev) for k, v in radii.items()}
        torch.cuda.synchronize()

        def sweep(k):
            rt.sweep_spheres_device(ctx, sc, org, t_d, t_r[k], out=t_rec)
            return ctx.last_kernel_ms()

        def nearest(k):
            rt.nearest_points_device(ctx, sc, org, t_r[k], out=t_near)
            return ctx.last_kernel_ms()

        def query():
            rt.trace_rays_device(ctx, sc, org.data_ptr(), t_d.data_ptr(), n, t_hit.data_ptr())
            return ctx.last_kernel_ms()

        def chain(k):
            """(launches, the sum of their kernel ms, balls left when CHAIN_MAX was reached)"""
            sweep(k)
            rec = t_rec.view(torch.float32).reshape(-1, 12)
            hit = t_rec.view(torch.int32).reshape(-1, 12)[:, 7] >= 0
            # the limit of a ball that meets nothing: once it is farther from the bounds' centre than their diagonal and r, moving away, it is done
            leave = (torch.linalg.norm(org - mid, dim=1) + 1.5 * diag + radii[k])
            goal = torch.where(hit, rec[:, 0], leave)
            t = torch.zeros(n, dtype=torch.float32, device=dev)
            alive = torch.ones(n, dtype=torch.bool, device=dev)
            launches, ms = 0, 0.0
            while launches < CHAIN_MAX and bool(alive.any()):
                idx = torch.nonzero(alive).reshape(-1)
                p = (org[idx] + t_d[idx] * t[idx, None]).contiguous()
                res = rt.nearest_points_device(ctx, sc, p)
                ms += ctx.last_kernel_ms()
                launches += 1
                step = res.view(torch.float32).reshape(-1, 8)[:, 0] - radii[k]
                t_new = t[idx] + torch.clamp(step, min=0.0)
                done = (t_new >= goal[idx] - 1e-4) | (step <= 1e-7)
                t[idx] = t_new
                alive[idx[done]] = False
            return launches, ms, int(alive.sum())

        legs = {"sweep_r0": lambda: sweep("r0"), "sweep_r1": lambda: sweep("r1"), "sweep_r10": lambda: sweep("r10"), "query": query,
                "nearest_r1": lambda: nearest("r1"), "nearest_r10": lambda: nearest("r10")}
        for f in legs.values():
            f(); f()
        ms = {k: [] for k in legs}
        chains = {"chain_r1": [], "chain_r10": []}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
            for k in chains:
                chains[k].append(chain(k[6:]))
        row = {"triangles": int(tris.shape[0]), "placement": sc.info()["scene_in_lds"], "threads": sc.info()["threads_per_block"], "diagonal": diag, "radii": radii}
        for k in ("r0", "r1", "r10"):
            sweep(k)
            torch.cuda.synchronize()
            words = t_rec.view(torch.int32).reshape(-1, 12)
            row["outcome_" + k] = {"contact": float(((words[:, 7] >= 0) & (words[:, 10] == 0)).float().mean()), "overlap": float((words[:, 10] == 1).float().mean()),
                                   "miss": float((words[:, 7] < 0).float().mean())}
        for k in legs:
            med = statistics.median(ms[k])
            row[k] = {"kernel_ms": ms[k], "kernel_ms_median": med, "kernel_ms_min": min(ms[k]), "kernel_ms_max": max(ms[k]), "mballs_per_s": n / med / 1e3}
        for k, runs in chains.items():
            tot = [r[1] for r in runs]
            row[k] = {"launches": [r[0] for r in runs], "left_at_the_cap": [r[2] for r in runs], "kernel_ms_sum": tot, "kernel_ms_sum_median": statistics.median(tot),
                      "kernel_ms_sum_min": min(tot), "kernel_ms_sum_max": max(tot)}
            r = k[6:]
            one = row["sweep_" + r]["kernel_ms_median"] + row["nearest_" + r]["kernel_ms_median"]
            row[k]["chain_over_sweep_call"] = row[k]["kernel_ms_sum_median"] / one
        row["sweep_r0_over_query"] = row["sweep_r0"]["kernel_ms_median"] / row["query"]["kernel_ms_median"]
        out["scenes"][name] = row
        del sc
    out_dir = args.out_dir or next_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sweep_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
