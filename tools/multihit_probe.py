"""Measurements of the multi-hit ray queries on the GPU, written as multihit_probe.json into the next unused profiles/rNN/ (or --out-dir):

  per scene (monkey, soup6k, sphere50k), 4,194,304 seeded incoherent rays - origins uniform in twice the scene's triangle bounds, unit
  directions uniform on the sphere (nearest_probe.py's rays of its closest-hit leg):
    multi_k1, multi_k4, multi_k8   trace_rays_multi_device with k = 1, 4, 8: kernel ms (rt_last_kernel_ms: the multi-hit kernel and, where
                                   the scene has a textured sphere, the texture-coordinate pass behind it)
    count_only                     ... with k = 0
    query                          the closest-hit query (trace_rays_device) on the same rays: its code is the parent's, byte for byte
    chained_k4, chained_k8         what a caller has without the entry point: k launches of trace_rays_device, every ray re-rooted between
                                   them at its hit point plus 1e-4 of its direction (torch, on the device, not timed); the SUM of the k
                                   kernel times - uploads, downloads and the re-rooting are left out, in the chain's favour
  The legs alternate, `--reps` rounds after a warm-up; medians, min / max and the spread (max - min) / median of each; every multi-hit leg
  as a ratio to `query`, k = 4 and 8 as a ratio to the chain of as many launches.

    python tools/multihit_probe.py [--rays 4194304] [--reps 5] [--out-dir DIR]
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
EPS = 1e-4


def next_profile_dir():
    used = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return os.path.join(ROOT, "profiles", "r%02d" % (max(used, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
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
    n = args.rays
    out = {"tool": "multihit_probe", "version": rt.lib().rt_version().decode(), "rays": n, "reps": args.reps, "reroot_epsilon": EPS, "scenes": {}}
    rng = np.random.default_rng(77)
    unit = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).to(dev)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    t_d = torch.from_numpy(d / np.linalg.norm(d, axis=1, keepdims=True)).to(dev)
    t_multi = torch.empty((n, 8, rt.HIT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    t_cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    t_hit = torch.empty((n, rt.HIT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    for name in ("monkey", "soup6k", "sphere50k"):
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        so = rt.SceneObjects(objs, models)
        flat = so.debug_flatten()
        sc = ctx.commit(so)
        _, _, tris, _ = R.sections(flat)
        corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        mid, half = torch.from_numpy((lo + hi) / 2).to(dev), torch.from_numpy(hi - lo).to(dev)
        org = (mid + unit * half).contiguous()
        torch.cuda.synchronize()

        def multi(k):
            def run():
                rt.trace_rays_multi_device(ctx, sc, org.data_ptr(), t_d.data_ptr(), k, hits=t_multi.data_ptr() if k else None, counts=t_cnt.data_ptr(), n=n)
                return ctx.last_kernel_ms()
            return run

        def query():
            rt.trace_rays_device(ctx, sc, org.data_ptr(), t_d.data_ptr(), n, t_hit.data_ptr())
            return ctx.last_kernel_ms()

        def chained(k):
            def run():
                o, total = org, 0.0
                for _ in range(k):
                    rt.trace_rays_device(ctx, sc, o.data_ptr(), t_d.data_ptr(), n, t_hit.data_ptr())
                    total += ctx.last_kernel_ms()
                    rec = t_hit.view(torch.float32).reshape(n, 12)
                    o = (rec[:, 1:4] + EPS * t_d).contiguous()           # a ray that missed is re-rooted at 0 + eps * d: it goes on costing a launch's share
                return total
            return run

        legs = {"multi_k1": multi(1), "multi_k4": multi(4), "multi_k8": multi(8), "count_only": multi(0), "query": query, "chained_k4": chained(4), "chained_k8": chained(8)}
        for f in legs.values():
            f()
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
        legs["count_only"]()
        torch.cuda.synchronize()
        counts = t_cnt.float()
        row = {"triangles": int(tris.shape[0]), "placement": sc.info()["scene_in_lds"], "threads": sc.info()["threads_per_block"],
               "hits_per_ray_mean": float(counts.mean()), "rays_without_a_hit": float((t_cnt == 0).float().mean()), "rays_of_more_than_8_hits": float((t_cnt > 8).float().mean())}
        for k in legs:
            med = statistics.median(ms[k])
            row[k] = {"kernel_ms": ms[k], "kernel_ms_median": med, "kernel_ms_min": min(ms[k]), "kernel_ms_max": max(ms[k]), "spread": (max(ms[k]) - min(ms[k])) / med,
                      "mrays_per_s": n / med / 1e3}
        for k in ("multi_k1", "multi_k4", "multi_k8", "count_only"):
            row[k + "_over_query"] = row[k]["kernel_ms_median"] / row["query"]["kernel_ms_median"]
        for k in (4, 8):
            row["multi_k%d_over_chained_k%d" % (k, k)] = row["multi_k%d" % k]["kernel_ms_median"] / row["chained_k%d" % k]["kernel_ms_median"]
        out["scenes"][name] = row
        del sc
    out_dir = args.out_dir or next_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "multihit_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
