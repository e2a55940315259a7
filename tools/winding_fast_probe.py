"""Measurements of the fast winding numbers on the GPU, written as winding_fast_probe.json into the next unused profiles/rNN/ (or --out-dir):

  per scene (monkey, soup6k, sphere50k), 4,194,304 seeded points uniform in twice the scene's triangle bounds (tools/winding_probe.py's):
    exact                    winding_numbers_device over the solids: kernel ms (rt_last_kernel_ms)
    fast_beta2 / 3 / 4       winding_numbers_fast_device, the moments fresh (no refit in the launch)
    signed_distance / _fast  signed_distance_device against signed_distance_fast_device at the default beta
    refit                    the refit alone, after an update of the mesh with its own vertices: the gather, the leaves, one launch per height
  The legs alternate, `--reps` rounds after a warm-up: medians and min / max of each, the ratios exact / fast, and whether the gap at the
  default beta exceeds both legs' spreads.  Beside the times: on the probe's own points the largest |w_fast - w_exact| and the share of inside
  bytes that differ (computed on the device from the two outputs), the accuracy tests/golden/winding_fast_meta.json records per beta, and
  what the compiler made of the kernels (VGPRs, SGPRs, spills, scratch, read from the library's code object).

    python tools/winding_fast_probe.py [--points 4194304] [--reps 5] [--out-dir DIR]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BETAS = (2.0, 3.0, 4.0)


def kernel_notes(lib_path):
    """registers, spills and scratch of the winding kernels, from the library's gfx950 code object"""
    import compare_kernels as ck
    with tempfile.TemporaryDirectory() as tmp:
        notes = ck.notes(ck.code_object(lib_path, tmp, "lib"))
    return {name: v for name, v in notes.items() if "rt_winding" in name}


def commit_order_triangles(flat, tree, obj, R):
    """the mesh's triangles [n, 9] in commit order, from the records as flattened (p0, p0 + s1, p0 + s2)"""
    tris = R.sections(flat)[2]
    s = int(flat["objects"][obj]["prim_start"])
    e = int(flat["objects"][obj + 1]["prim_start"]) if obj + 1 < len(flat["objects"]) else flat["num_triangles"]
    rec = tris[tree["position"][s:e]]
    out = np.zeros((e - s, 9), np.float32)
    out[tree["order"][s:e]] = np.concatenate([rec[:, 0:3], rec[:, 0:3] + rec[:, 3:6], rec[:, 0:3] + rec[:, 6:9]], axis=1)
    return out


def main():
    from nearest_probe import next_profile_dir
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
    meta_path = os.path.join(ROOT, "tests", "golden", "winding_fast_meta.json")
    meta = json.load(open(meta_path))["per_scene"] if os.path.exists(meta_path) else {}
    out = {"tool": "winding_fast_probe", "version": rt.lib().rt_version().decode(), "points": n, "reps": args.reps, "betas": list(BETAS),
           "kernels": kernel_notes(rt.build.LIB), "scenes": {}}
    rng = np.random.default_rng(77)
    unit = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).to(dev)
    t_rec = torch.empty((n, rt.NearestRecord.itemsize), dtype=torch.uint8, device=dev)
    t_exact = torch.empty((n,), dtype=torch.float32, device=dev)
    t_fast = torch.empty((n,), dtype=torch.float32, device=dev)
    t_sdf = torch.empty((n,), dtype=torch.float32, device=dev)
    for name in ("monkey", "soup6k", "sphere50k"):
        objs, _ = rt.scenes.CONFIG_SCENES[name]()
        so = rt.SceneObjects(objs, models)
        flat = so.debug_flatten()
        sc = ctx.commit(so)
        tris = R.sections(flat)[2]
        corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        mid, half = torch.from_numpy((lo + hi) / 2).to(dev), torch.from_numpy(hi - lo).to(dev)
        pts = (mid + unit * half).contiguous()                       # twice the bounds: the centre +- the full extent
        tree = sc.debug_winding_tree()
        mesh = [i for i, o in enumerate(flat["objects"]) if o["type"] == R.OBJ_MESH][0]
        own = torch.from_numpy(commit_order_triangles(flat, tree, mesh, R)).to(dev)
        torch.cuda.synchronize()

        def exact():
            rt.winding_numbers_device(ctx, sc, pts, winding=t_exact)
            return ctx.last_kernel_ms()

        def fast(beta):
            def run():
                rt.winding_numbers_fast_device(ctx, sc, pts, beta=beta, winding=t_fast)
                return ctx.last_kernel_ms()
            return run

        def signed_distance():
            rt.signed_distance_device(ctx, sc, pts, sdf=t_sdf, records=t_rec)
            return ctx.last_kernel_ms()

        def signed_distance_fast():
            rt.signed_distance_fast_device(ctx, sc, pts, sdf=t_sdf, records=t_rec)
            return ctx.last_kernel_ms()

        def refit():
            sc.update_mesh_device(mesh, own)
            sc.debug_winding_tree()                                  # the refit alone, in a launch of its own
            return ctx.last_kernel_ms()

        legs = {"exact": exact, "signed_distance": signed_distance, "signed_distance_fast": signed_distance_fast, "refit": refit}
        legs.update({"fast_beta%g" % b: fast(b) for b in BETAS})
        for f in legs.values():
            f(); f()
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():
                ms[k].append(f())
        row = {"triangles": int(tris.shape[0]), "clusters": int(tree["skip"].shape[0]), "placement": sc.info()["scene_in_lds"], "recorded_accuracy": meta.get(name)}
        for k in legs:
            med = statistics.median(ms[k])
            row[k] = {"kernel_ms": ms[k], "kernel_ms_median": med, "kernel_ms_min": min(ms[k]), "kernel_ms_max": max(ms[k])}
        exact()
        row["on_the_probes_points"] = {}
        for b in BETAS:
            fast(b)()
            torch.cuda.synchronize()
            row["on_the_probes_points"]["%g" % b] = {"worst_abs_difference": float((t_fast - t_exact).abs().max()),
                                                     "inside_bytes_that_differ": float(((t_fast.abs() >= 0.5) != (t_exact.abs() >= 0.5)).float().mean())}
            row["exact_over_fast_beta%g" % b] = row["exact"]["kernel_ms_median"] / row["fast_beta%g" % b]["kernel_ms_median"]
        row["signed_distance_over_fast"] = row["signed_distance"]["kernel_ms_median"] / row["signed_distance_fast"]["kernel_ms_median"]
        e, f2 = row["exact"], row["fast_beta2"]
        spreads = (e["kernel_ms_max"] - e["kernel_ms_min"]) + (f2["kernel_ms_max"] - f2["kernel_ms_min"])
        row["fast_beats_exact_by_more_than_both_spreads"] = bool(e["kernel_ms_median"] - f2["kernel_ms_median"] > spreads)
        out["scenes"][name] = row
        del sc
    out_dir = args.out_dir or next_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "winding_fast_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
