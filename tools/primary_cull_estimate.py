"""What the primary-ray cull (csrc/rt_cull.h) flags in a view, on the CPU alone (development tool; no GPU, the project's own flattened tree):
   python tools/primary_cull_estimate.py [--scene monkey] [--width 128] [--height 72] [--no-antialias]
For a config scene (ray-tracer_amd/scenes.py) and an image size it evaluates the kernel's predicate per pixel through
rt_debug_primary_cull_host and prints the flagged share of the pixels whose jitter cone may enter a mesh's root box, and the share of the
centre-ray node steps of those pixels that the flagged ones carry - the traversal work the render kernel no longer does for primary rays.
For the other root-entering pixels it prints, from rt_debug_subtree_cull_host, the share of the centre ray's node steps that lie below a dead
gate (the subtree cull): the steps the kernel's walk takes without the pixel's gate word and no longer takes with it.  And, from
rt_debug_primary_entry_host, the three classes of the primary entry word (csrc/rt_entry.h) among those pixels - `triangle`, `nothing`, not
known - with the share of the gated centre-ray node steps and triangle tests that the first two no longer run (a `triangle` pixel keeps one
triangle test)."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def estimate(scene="monkey", width=128, height=72, antialias=True):
    rt = importlib.import_module("ray-tracer_amd")
    objs, _sky = getattr(rt.scenes, scene)()
    _words, st = rt.primary_cull_host(rt.SceneObjects(objs), rt.Camera(width, height), antialias)
    st = dict(st, scene=scene, width=width, height=height, antialias=bool(antialias), pixels=width * height)
    st["flagged_share_of_root_entering"] = st["flagged_root_entering"] / st["root_entering"] if st["root_entering"] else 0.0
    st["step_share_of_flagged"] = st["centre_steps_flagged"] / st["centre_steps_root_entering"] if st["centre_steps_root_entering"] else 0.0
    _gates, gt = rt.subtree_cull_host(rt.SceneObjects(objs), rt.Camera(width, height), antialias)
    st.update({"gate_" + k: v for k, v in gt.items()})
    st["dead_gate_step_share"] = 1.0 - gt["centre_steps_gated"] / gt["centre_steps"] if gt["centre_steps"] else 0.0
    _entry, et = rt.primary_entry_host(rt.SceneObjects(objs), rt.Camera(width, height), antialias)
    st.update({"entry_" + k: v for k, v in et.items()})
    px = et["pixels_triangle"] + et["pixels_nothing"] + et["pixels_unknown"]
    steps = et["centre_steps_triangle"] + et["centre_steps_nothing"] + et["centre_steps_unknown"]
    tests = et["centre_tests_triangle"] + et["centre_tests_nothing"] + et["centre_tests_unknown"]
    st["entry_resolved_share"] = (et["pixels_triangle"] + et["pixels_nothing"]) / px if px else 0.0
    st["entry_step_share_removed"] = (et["centre_steps_triangle"] + et["centre_steps_nothing"]) / steps if steps else 0.0
    st["entry_test_share_removed"] = (et["centre_tests_triangle"] - et["pixels_triangle"] + et["centre_tests_nothing"]) / tests if tests else 0.0
    # the sub-entry tables of the not-known pixels (csrc/rt_entry.h): every one of them gets a table here, whatever the image's allocation holds
    _p, _w, sub = rt.primary_subentry_host(rt.SceneObjects(objs), rt.Camera(width, height), antialias, cap=1 << 30)
    st.update({"sub_" + k: v for k, v in sub.items()})
    boxes = sub["sub_triangle"] + sub["sub_nothing"] + sub["sub_unknown"]
    st["sub_resolved_share"] = (sub["sub_triangle"] + sub["sub_nothing"]) / boxes if boxes else 0.0
    st["sub_step_weighted_share"] = sub["centre_steps_resolved"] / sub["centre_steps_all"] if sub["centre_steps_all"] else 0.0
    return st


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scene", default="monkey")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=72)
    ap.add_argument("--no-antialias", action="store_true")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    st = estimate(a.scene, a.width, a.height, not a.no_antialias)
    if a.json:
        print(json.dumps(st))
        return
    print("%s %dx%d antialias=%s" % (st["scene"], st["width"], st["height"], st["antialias"]))
    print("pixels whose cone may enter a root box: %d of %d" % (st["root_entering"], st["pixels"]))
    print("of those, flagged (no leaf reachable):  %d (%.1f %%)" % (st["flagged_root_entering"], 100 * st["flagged_share_of_root_entering"]))
    print("flagged pixels in all:                  %d (%.1f %% of the image)" % (st["flagged"], 100.0 * st["flagged"] / st["pixels"]))
    print("centre-ray node steps: %.1f per flagged root-entering pixel, %.1f per other root-entering pixel" % (
        st["centre_steps_flagged"] / max(st["flagged_root_entering"], 1),
        (st["centre_steps_root_entering"] - st["centre_steps_flagged"]) / max(st["root_entering"] - st["flagged_root_entering"], 1)))
    print("share of those steps carried by the flagged pixels: %.1f %%" % (100 * st["step_share_of_flagged"]))
    print("unflagged root-entering pixels: %d, %d with a dead gate; kernel-order centre-ray node steps %.1f per pixel, %.1f with the gate word" % (
        st["gate_pixels"], st["gate_pixels_with_dead_gates"], st["gate_centre_steps"] / max(st["gate_pixels"], 1),
        st["gate_centre_steps_gated"] / max(st["gate_pixels"], 1)))
    print("share of those steps below a dead gate:             %.1f %%" % (100 * st["dead_gate_step_share"]))
    print("entry words of the unflagged root-entering pixels: triangle %d, nothing %d, not known %d (resolved %.1f %%)" % (
        st["entry_pixels_triangle"], st["entry_pixels_nothing"], st["entry_pixels_unknown"], 100 * st["entry_resolved_share"]))
    print("gated centre-ray node steps by class: %d / %d / %d; triangle tests: %d / %d / %d" % (
        st["entry_centre_steps_triangle"], st["entry_centre_steps_nothing"], st["entry_centre_steps_unknown"],
        st["entry_centre_tests_triangle"], st["entry_centre_tests_nothing"], st["entry_centre_tests_unknown"]))
    print("share of those node steps the entry words remove:   %.1f %%; of the triangle tests: %.1f %%" % (
        100 * st["entry_step_share_removed"], 100 * st["entry_test_share_removed"]))
    print("sub-entry tables of the %d not-known pixels: sub-boxes triangle %d, nothing %d, not known %d: resolved %.1f %%, weighted by the centre ray's gated node steps %.1f %%" % (
        st["sub_tables"], st["sub_sub_triangle"], st["sub_sub_nothing"], st["sub_sub_unknown"], 100 * st["sub_resolved_share"], 100 * st["sub_step_weighted_share"]))


if __name__ == "__main__":
    main()
