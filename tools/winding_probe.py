"""Measurements of the winding-number queries on the GPU, written as winding_probe.json into the next unused profiles/rNN/ (or --out-dir):

  per scene (monkey, soup6k, sphere50k), 4,194,304 seeded points uniform in twice the scene's triangle bounds:
    winding          winding_numbers_device over the solids: kernel ms (rt_last_kernel_ms), Mpoints/s, triangle terms per second and what share
                     of the VALU's plain-instruction peak that is at --valu-per-term instructions a term (the count in the kernel's record loop)
    signed_distance  signed_distance_device: the nearest-surface launch and the winding launch together
    nearest          nearest_points_device on the same points: for scale
    brute_force      what a caller has without the entry point: a torch float32 evaluation of the same sum (atan2 per point and triangle,
                     n x T temporaries) on the same GPU at the largest n that fits a fixed budget of temporaries; ms per call on the host
                     clock around a device synchronise, and ms per 2^22 points by proportion
  The three library legs alternate, `--reps` rounds after a warm-up; medians and min / max of each.

    python tools/winding_probe.py [--points 4194304] [--reps 5] [--out-dir DIR]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BRUTE_ELEMENTS = 1 << 26            # n x T of the brute force: ~30 float32 temporaries of that size are alive at its peak
VALU_PEAK = 256 * 4 * 32 * 2.4e9    # lane-instructions per second: 256 CUs x 4 SIMDs x 32 lanes a cycle (a wave64 instruction issues over 2 cycles) at 2.4 GHz; 157.3 TFLOPS is this x 2 for an FMA


def torch_brute_force(torch, tris, flip, p):
    """the signed sum of atan2(det, den) over every triangle record [T, 9] for p [n, 3], over 2 pi: -> [n]"""
    a = tris[None, :, 0:3] - p[:, None, :]
    b, c = a + tris[None, :, 3:6], a + tris[None, :, 6:9]
    la, lb, lc = torch.linalg.norm(a, dim=-1), torch.linalg.norm(b, dim=-1), torch.linalg.norm(c, dim=-1)
    nrm = torch.cross(tris[:, 3:6], tris[:, 6:9], dim=-1)
    det = (a * nrm[None, :, :]).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (a * c).sum(-1) * lb + (b * c).sum(-1) * la
    return (torch.atan2(det, den) * flip[None, :]).sum(dim=1) / (2.0 * np.pi)


def main():
    from nearest_probe import next_profile_dir
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--valu-per-term", type=int, default=156)
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
    out = {"tool": "winding_probe", "version": rt.lib().rt_version().decode(), "points": n, "reps": args.reps, "valu_per_term": args.valu_per_term,
           "valu_peak_lane_instructions_per_s": VALU_PEAK, "scenes": {}}
    rng = np.random.default_rng(77)
    unit = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).to(dev)
    t_rec = torch.empty((n, rt.NearestRecord.itemsize), dtype=torch.uint8, device=dev)
    t_w = torch.empty((n,), dtype=torch.float32, device=dev)
    t_sdf = torch.empty((n,), dtype=torch.float32, device=dev)
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
        torch.cuda.synchronize()

        def winding():
            rt.winding_numbers_device(ctx, sc, pts, winding=t_w)
            return ctx.last_kernel_ms()

        def signed_distance():
            rt.signed_distance_device(ctx, sc, pts, sdf=t_sdf, records=t_rec)
            return ctx.last_kernel_ms()

        def nearest():
            rt.nearest_points_device(ctx, sc, pts, out=t_rec)
            return ctx.last_kernel_ms()

        legs = {"winding": winding, "signed_distance": signed_distance, "nearest": nearest}
        for f in legs.values():
            f(); f()
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
        winding()
        torch.cuda.synchronize()
        inside = float((t_w.abs() >= 0.5).float().mean())
        # the brute force, at the largest n that fits its budget of temporaries (the meshes' records only: spheres add nothing to the sum's cost)
        mesh = np.array([o["type"] == R.OBJ_MESH for o in objects])
        assert mesh.any() and all(o["type"] in (R.OBJ_MESH, R.OBJ_SPHERE) for o in objects), name
        T = tris.shape[0]
        n_bf = max(256, min(n, BRUTE_ELEMENTS // max(T, 1)))
        t_tris = torch.from_numpy(np.ascontiguousarray(tris[:, 0:9])).to(dev)
        t_flip = torch.from_numpy(1.0 - 2.0 * flat["tri_flip"].astype(np.float32)).to(dev)
        sph = np.array([o["v"][0:4] for o in objects if o["type"] == R.OBJ_SPHERE], np.float32).reshape(-1, 4)
        t_sph = torch.from_numpy(sph).to(dev)
        bf_ms = []
        for k in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bf_w = torch_brute_force(torch, t_tris, t_flip, pts[:n_bf])
            if sph.shape[0]:
                bf_w = bf_w + (torch.linalg.norm(pts[:n_bf, None, :] - t_sph[None, :, 0:3], dim=-1) < t_sph[None, :, 3]).float().sum(dim=1)
            torch.cuda.synchronize()
            if k:
                bf_ms.append(1e3 * (time.perf_counter() - t0))
        agree = float((torch.abs(bf_w - t_w[:n_bf]) <= 1e-3).float().mean())
        row = {"triangles": int(T), "spheres": int(sph.shape[0]), "placement": sc.info()["scene_in_lds"], "inside_share": inside,
               "brute_force": {"n": int(n_bf), "ms": bf_ms, "ms_median": statistics.median(bf_ms),
                               "ms_per_2^22_points_by_proportion": statistics.median(bf_ms) * n / n_bf, "agrees_with_the_library_to_1e-3": agree}}
        for k in legs:
            med = statistics.median(ms[k])
            row[k] = {"kernel_ms": ms[k], "kernel_ms_median": med, "kernel_ms_min": min(ms[k]), "kernel_ms_max": max(ms[k]), "mpoints_per_s": n / med / 1e3}
        terms = float(n) * T / (row["winding"]["kernel_ms_median"] * 1e-3)
        row["winding"]["terms_per_s"] = terms
        row["winding"]["share_of_valu_peak"] = terms * args.valu_per_term / VALU_PEAK
        row["brute_force_over_winding"] = row["brute_force"]["ms_per_2^22_points_by_proportion"] / row["winding"]["kernel_ms_median"]
        row["winding_over_nearest"] = row["winding"]["kernel_ms_median"] / row["nearest"]["kernel_ms_median"]
        row["signed_distance_over_nearest"] = row["signed_distance"]["kernel_ms_median"] / row["nearest"]["kernel_ms_median"]
        out["scenes"][name] = row
        del sc
    out_dir = args.out_dir or next_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "winding_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
