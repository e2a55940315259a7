"""Measurements of the occlusion queries and the visibility plane on the GPU (one JSON line), the sibling of tools/query_probe.py:

  incoherent  2^22 seeded random rays (query_probe's) on monkey, soup6k and sphere50k: occluded_rays_device against its yardstick,
              trace_rays_device on the same rays in the same loop, alternating pairs after a warm-up; kernel ms from rt_last_kernel_ms,
              medians and spreads (max - min) of both, for tmax = NULL and for a per-ray limit of half the scene's extent (the extent
              is taken as the 90th percentile of the batch's closest-hit distances)
  visibility  the metric scene at 1920x1080: render_visibility_device against render_aov_device (depth only) of the same view
  small       1 / 64 / 4,096 / 65,536 rays on monkey: ms per call end to end (launch + wait on the host clock)
  refill      with --sweep 8,16,24,32: the same incoherent leg on monkey and sphere50k in a fresh child process per value, each loading
              the development build libraytracer_amd_refill<N>.so (build.build_variant("refill<N>", ["-DRT_OCCLUSION_REFILL=<N>"]))

    python tools/occlusion_probe.py [--pairs 7] [--rays 4194304] [--sweep 8,16,24,32]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.query_probe import random_rays          # noqa: E402


def spread(x):
    return max(x) - min(x)


def incoherent(rt, ctx, torch, names, n, pairs):
    dev = torch.device("cuda:0")
    models = rt.scenes.models_dir()
    o, d = random_rays(n, 21)
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t_h = torch.empty(n * rt.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    t_b = torch.empty(n, dtype=torch.uint8, device=dev)
    out = {}
    for name in names:
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        sc = ctx.commit(rt.SceneObjects(objs, models))

        def closest():
            rt.trace_rays_device(ctx, sc, t_o.data_ptr(), t_d.data_ptr(), n, t_h.data_ptr())
            return ctx.last_kernel_ms()

        def occluded(t_t):
            rt.occluded_rays_device(ctx, sc, t_o.data_ptr(), t_d.data_ptr(), t_t.data_ptr() if t_t is not None else None, n, t_b.data_ptr())
            return ctx.last_kernel_ms()

        closest()
        hits = t_h.cpu().numpy().view(rt.HIT_DTYPE)
        hit = hits["object"] >= 0
        extent = float(np.percentile(hits["t"][hit], 90))
        t_half = torch.full((n,), extent / 2, dtype=torch.float32, device=dev)
        res = {"rays": n, "hit_fraction": float(hit.mean()), "extent_p90": extent, "placement": sc.info()["scene_in_lds"], "threads": sc.info()["threads_per_block"]}
        for label, t_t in (("tmax_null", None), ("tmax_half_extent", t_half)):
            for _ in range(2):
                occluded(t_t); closest()
            o_ms, c_ms = [], []
            for _ in range(pairs):
                o_ms.append(occluded(t_t))
                c_ms.append(closest())
            frac = float(t_b.cpu().numpy().mean())
            om, cm = statistics.median(o_ms), statistics.median(c_ms)
            res[label] = {"occlusion_kernel_ms_median": om, "occlusion_spread_ms": spread(o_ms), "occlusion_kernel_ms": o_ms,
                          "closest_kernel_ms_median": cm, "closest_spread_ms": spread(c_ms), "closest_kernel_ms": c_ms,
                          "occlusion_over_closest": om / cm, "occlusion_mrays_per_s": n / om / 1e3, "occluded_fraction": frac,
                          "not_slower_beyond_spread": bool(om <= cm + spread(c_ms))}
        out[name] = res
    return out, (rt, ctx, sc, t_o, t_d, t_b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--sweep-leg", action="store_true", help="(child of --sweep) the incoherent leg on monkey and sphere50k with the library RT_AMD_LIB names")
    args = ap.parse_args()
    import torch
    rt = importlib.import_module("ray-tracer_amd")
    ctx = rt.Context(0)
    if args.sweep_leg:
        res, _ = incoherent(rt, ctx, torch, ("monkey", "sphere50k"), args.rays, args.pairs)
        print(json.dumps({name: {k: {"occlusion_kernel_ms_median": v[k]["occlusion_kernel_ms_median"], "occlusion_spread_ms": v[k]["occlusion_spread_ms"],
                                     "closest_kernel_ms_median": v[k]["closest_kernel_ms_median"]} for k in ("tmax_null", "tmax_half_extent")}
                          for name, v in res.items()}))
        return
    dev = torch.device("cuda:0")
    models = rt.scenes.models_dir()
    out = {"tool": "occlusion_probe", "version": rt.lib().rt_version().decode()}
    out["incoherent"], _ = incoherent(rt, ctx, torch, ("monkey", "soup6k", "sphere50k"), args.rays, args.pairs)

    # ---- the visibility plane against the AOV pass (depth only) of the same view
    objs, _ = rt.scenes.monkey()
    scene = ctx.commit(rt.SceneObjects(objs, models))
    W, H = 1920, 1080
    cam = rt.Camera(W, H)
    depth = torch.empty((H, W), device=dev)
    plane = torch.empty((H, W), dtype=torch.uint8, device=dev)
    light = (1.5, 2.0, 0.2)

    def vis():
        rt.render_visibility_device(ctx, scene, cam, light, 1e-3, plane.data_ptr())
        return ctx.last_kernel_ms()

    def aov():
        rt.render_aov_device(ctx, scene, cam, (0.0, 0.0, 0.0), d_depth=depth.data_ptr())
        return ctx.last_kernel_ms()

    for _ in range(3):
        vis(); aov()
    v_ms, a_ms = [], []
    for _ in range(12):
        v_ms.append(vis())
        a_ms.append(aov())
    codes = np.bincount(plane.cpu().numpy().reshape(-1), minlength=3)
    vm, am = statistics.median(v_ms), statistics.median(a_ms)
    out["visibility"] = {"scene": "monkey", "width": W, "height": H, "light": light, "bias": 1e-3, "pairs": 12, "visibility_kernel_ms_median": vm,
                         "visibility_spread_ms": spread(v_ms), "visibility_kernel_ms": v_ms, "aov_depth_kernel_ms_median": am, "aov_depth_spread_ms": spread(a_ms),
                         "aov_depth_kernel_ms": a_ms, "visibility_over_aov": vm / am, "blocked": int(codes[0]), "lit": int(codes[1]), "no_surface": int(codes[2])}

    # ---- small batches
    n = 65536
    o, d = random_rays(n, 21)
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t_b = torch.empty(n, dtype=torch.uint8, device=dev)
    small = {}
    for k in (1, 64, 4096, 65536):
        for _ in range(3):
            rt.occluded_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), None, k, t_b.data_ptr())
        ctx.synchronize()
        reps = 20
        t0 = time.perf_counter()
        for _ in range(reps):
            rt.occluded_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), None, k, t_b.data_ptr())
            ctx.synchronize()
        small[str(k)] = {"ms_per_call": (time.perf_counter() - t0) * 1e3 / reps, "kernel_ms_last": ctx.last_kernel_ms()}
    out["small_batches_monkey"] = small

    # ---- the refill threshold: one fresh child per development build
    if args.sweep:
        out["refill_sweep"] = {}
        del ctx
        for v in args.sweep.split(","):
            lib = os.path.join(ROOT, "ray-tracer_amd", "libraytracer_amd_refill%s.so" % v)
            if not os.path.exists(lib):
                out["refill_sweep"][v] = "no such build: " + os.path.basename(lib)
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweep-leg", "--pairs", str(args.pairs), "--rays", str(args.rays)],
                               env=dict(os.environ, RT_AMD_LIB=lib), capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                out["refill_sweep"][v] = "child failed (%d): %s" % (r.returncode, r.stderr[-300:])
                break                                   # nothing more is started on the GPU after a failure
            out["refill_sweep"][v] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
