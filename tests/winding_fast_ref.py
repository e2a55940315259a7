"""The yardstick of the fast winding numbers (rt_winding_numbers_fast, rt_signed_distance_fast, include/rt_amd.h) in NumPy binary32: no product code.

It reads a flattened scene (SceneObjects.debug_flatten() / Scene.debug_read()) and the REPORTED cluster trees (SceneObjects.debug_winding_tree()
/ Scene.debug_winding_tree(): the topology, the order list and where every triangle's record sits - the topology is no part of the
definition), restates the moments and the walk in the header's order, every operation one NumPy float32 operation, and iterates over the
clusters in preorder, vectorised over the points with masks.

    moments(flat, tree)                         -> float32 [clusters, 8]: (c.xyz, r2, M.xyz, 0), what the host text and the device must hold
    winding(flat, tree, points, beta, obj=-1)   -> float32 [n], byte for byte what the library must answer
    work(...)                                   -> cluster visits and triangle terms per point

What the approximation costs in accuracy is measured against the exact yardstick tests/winding_ref.py, never against the code under test:
measure_meta() is how tests/golden/winding_fast_meta.json was made (python tests/winding_fast_ref.py)."""
import json
import os

import numpy as np

import nearest_ref as NR
import winding_ref as W

LEAF_TRIS = 8
BETA_DEFAULT = np.float32(2.0)
THIRD = np.float32(float.fromhex("0x1.555556p-2"))      # RT_WN_THIRD
QUARTER = np.float32(0.25)
F0 = np.float32(0)
dot = NR.dot


def mesh_objects(flat):
    return [i for i, o in enumerate(flat["objects"]) if int(o["type"]) == W.OBJ_MESH]


def gathered(flat, tree):
    """(records [triangles, 12], flip bytes [triangles]) in cluster order: entry prim_start + j is the triangle at cluster position j"""
    tris = NR.sections(flat)[2]
    pos = tree["position"]
    rec = np.zeros((flat["num_triangles"], 12), np.float32)
    flip = np.zeros(flat["num_triangles"], np.uint8)
    for i in mesh_objects(flat):
        s, e, _ = W.object_records(flat, i)
        rec[s:e] = tris[pos[s:e]]
        flip[s:e] = flat["tri_flip"][pos[s:e]]
    return rec, flip


def heights(tree):
    skip, count = tree["skip"], tree["count"]
    h = np.zeros(skip.shape[0], np.int64)
    for i in range(skip.shape[0] - 1, -1, -1):
        if count[i] == 0:
            h[i] = 1 + max(h[i + 1], h[skip[i + 1]])
    return h


def sums(flat, tree):
    """per cluster (Msum [3], Asum, Gsum [3], lo [3], hi [3]): the leaves over their triangles in cluster order, the rest bottom-up"""
    rec, flip = gathered(flat, tree)
    skip, first, count = tree["skip"], tree["first"], tree["count"]
    nc = skip.shape[0]
    M, A, G = np.zeros((nc, 3), np.float32), np.zeros(nc, np.float32), np.zeros((nc, 3), np.float32)
    lo, hi = np.zeros((nc, 3), np.float32), np.zeros((nc, 3), np.float32)
    leaves = np.nonzero(count > 0)[0]
    if leaves.size:
        lo[leaves] = rec[first[leaves], 0:3]
        hi[leaves] = rec[first[leaves], 0:3]
    with np.errstate(all="ignore"):
        for k in range(LEAF_TRIS):
            at = leaves[count[leaves] > k]
            if not at.size:
                break
            t = rec[first[at] + k]
            f = flip[first[at] + k] == 1
            p0, s1, s2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
            n = np.stack([s1[:, 1] * s2[:, 2] - s1[:, 2] * s2[:, 1], s1[:, 2] * s2[:, 0] - s1[:, 0] * s2[:, 2], s1[:, 0] * s2[:, 1] - s1[:, 1] * s2[:, 0]], axis=1)
            n = np.where(f[:, None], W.neg(n), n)
            a = np.sqrt(dot(n[:, 0], n[:, 1], n[:, 2], n[:, 0], n[:, 1], n[:, 2]))
            g = p0 + (s1 + s2) * THIRD
            M[at] = M[at] + n
            A[at] = A[at] + a
            G[at] = G[at] + a[:, None] * g
            for corner in (p0, p0 + s1, p0 + s2):
                lo[at] = np.where(corner < lo[at], corner, lo[at])
                hi[at] = np.where(hi[at] < corner, corner, hi[at])
        h = heights(tree)
        for level in range(1, int(h.max()) + 1 if nc else 0):
            at = np.nonzero(h == level)[0]
            L = at + 1
            R = skip[L]
            M[at], A[at], G[at] = M[L] + M[R], A[L] + A[R], G[L] + G[R]
            lo[at] = np.where(lo[R] < lo[L], lo[R], lo[L])
            hi[at] = np.where(hi[L] < hi[R], hi[R], hi[L])
    return M, A, G, lo, hi


def moments(flat, tree):
    M, A, G, lo, hi = sums(flat, tree)
    with np.errstate(all="ignore"):
        c = np.where((A > F0)[:, None], G / A[:, None], lo)
        a, b = c - lo, hi - c
        e = np.where(a > b, a, b)
        r2 = dot(e[:, 0], e[:, 1], e[:, 2], e[:, 0], e[:, 1], e[:, 2])
        out = np.zeros((A.shape[0], 8), np.float32)
        out[:, 0:3], out[:, 3], out[:, 4:7] = c, r2, QUARTER * M
    return out


def mesh_walk(flat, tree, mom, rec, flip, i, p, beta2, counts=None):
    """A [n] of mesh object i before the final scale: the clusters in preorder, every point either skipping (inside a subtree it left
    behind) or at the cluster.  counts: [visits, terms] [2, n] int64, added to"""
    c0, c1 = (int(x) for x in tree["object_range"][i])
    skip, first, count = tree["skip"], tree["first"], tree["count"]
    A = np.zeros(p.shape[0], np.float32)
    until = np.full(p.shape[0], c0, np.int64)        # the next cluster the point visits
    with np.errstate(all="ignore"):
        for ci in range(c0, c1):
            at = np.nonzero(until <= ci)[0]
            if not at.size:
                continue
            q = p[at]
            dx, dy, dz = mom[ci, 0] - q[:, 0], mom[ci, 1] - q[:, 1], mom[ci, 2] - q[:, 2]
            d2 = dot(dx, dy, dz, dx, dy, dz)
            far = d2 > beta2 * mom[ci, 3]
            if counts is not None:
                counts[0, at] += 1
            fa = at[far]
            if fa.size:
                A[fa] = A[fa] + dot(mom[ci, 4], mom[ci, 5], mom[ci, 6], dx[far], dy[far], dz[far]) / (d2[far] * np.sqrt(d2[far]))
                until[fa] = skip[ci]
            near = at[~far]
            if near.size and count[ci] > 0:
                for k in range(int(first[ci]), int(first[ci] + count[ci])):
                    term = W.term32(rec[k], p[near])
                    A[near] = A[near] + (W.neg(term) if flip[k] else term)
                if counts is not None:
                    counts[1, near] += int(count[ci])
                until[near] = skip[ci]
    return A


def winding(flat, tree, points, beta, obj=W.SOLIDS, mom=None, counts=None):
    """the winding numbers rt_winding_numbers_fast must answer; mom: the moments to walk with (default: moments(flat, tree))"""
    p_all = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ok = np.isfinite(p_all).all(axis=1)
    p = np.where(ok[:, None], p_all, F0)
    with np.errstate(all="ignore"):
        beta2 = np.float32(beta) * np.float32(beta)
    meshes = mesh_objects(flat)
    if meshes:
        mom = moments(flat, tree) if mom is None else mom
        rec, flip = gathered(flat, tree)

    def one(i):
        if i not in meshes:
            return W.object_winding(flat, i, p)
        A = np.zeros(p.shape[0], np.float32)
        sub = None if counts is None else np.zeros((2, int(ok.sum())), np.int64)
        A[ok] = mesh_walk(flat, tree, mom, rec, flip, i, p[ok], beta2, sub)
        if counts is not None:
            counts[:, ok] += sub
        return A * W.INV_2PI

    with np.errstate(all="ignore"):
        if obj >= 0:
            w = one(obj)
        else:
            w = np.zeros(p.shape[0], np.float32)
            for i, o in enumerate(flat["objects"]):
                if int(o["type"]) in (W.OBJ_SPHERE, W.OBJ_CUBOID, W.OBJ_MESH):
                    w = w + one(i)
    return np.where(ok & ~np.isnan(w), w, W.QNAN).astype(np.float32)


def work(flat, tree, points, beta):
    """(cluster visits, triangle terms) per point [2, n] of the solids' query"""
    counts = np.zeros((2, np.asarray(points).reshape(-1, 3).shape[0]), np.int64)
    winding(flat, tree, points, beta, counts=counts)
    return counts


def check_topology(flat, tree):
    """raises AssertionError unless the reported trees are valid: every triangle of a mesh in exactly one leaf, leaves of at most LEAF_TRIS,
    preorder with consistent skip, order a permutation per mesh and position its image in the flattened list"""
    skip, first, count, rng = tree["skip"], tree["first"], tree["count"], tree["object_range"]
    assert rng.shape == (len(flat["objects"]), 2)
    at = 0
    for i, o in enumerate(flat["objects"]):
        c0, c1 = (int(x) for x in rng[i])
        if int(o["type"]) != W.OBJ_MESH:
            assert c0 == c1 == 0, (i, c0, c1)
            continue
        s, e, _ = W.object_records(flat, i)
        assert c0 == at and c1 >= c0 and (c1 > c0) == (e > s), (i, c0, c1, at)
        at = c1
        assert sorted(tree["order"][s:e].tolist()) == list(range(e - s)), "order is no permutation of the mesh's commit indices"
        assert sorted(tree["position"][s:e].tolist()) == list(range(s, e)), "position is no permutation of the mesh's records"
        seen = np.zeros(e - s, np.int64)

        def subtree(c, end):
            """checks the subtree rooted at c, which must end at `end`; returns the triangles below it"""
            assert c0 <= c < c1 and skip[c] == end, (c, int(skip[c]), end)
            if count[c] > 0:
                assert 1 <= count[c] <= LEAF_TRIS and skip[c] == c + 1 and s <= first[c] and first[c] + count[c] <= e, (c, int(first[c]), int(count[c]))
                seen[first[c] - s:first[c] - s + count[c]] += 1
                return int(count[c])
            assert c + 1 < end and c + 1 < skip[c + 1] < end, (c, "an internal cluster has two children")
            left, right = subtree(c + 1, int(skip[c + 1])), subtree(int(skip[c + 1]), end)
            assert left == (left + right + 1) // 2 and left + right > LEAF_TRIS, (c, left, right)
            return left + right

        if c1 > c0:
            assert subtree(c0, c1) == e - s
        assert (seen == 1).all(), "a triangle is in no leaf, or in two"
    assert at == skip.shape[0]


# ---- the measured accuracy ------------------------------------------------------------------------------------------------------------
META = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "winding_fast_meta.json")
BETAS = (2.0, 3.0, 4.0)
META_SCENES = ("cube", "monkey", "reference_scene0", "random6", "soup6k", "sphere50k")
META_UNIFORM = {"soup6k": 300, "sphere50k": 200}          # the exact yardstick is linear in the mesh: fewer points on the large ones
WORK_POINTS = 2000


def scene_objects(rt, name):
    if name.startswith("random"):
        from random_scenes import random_scene
        return random_scene(int(name[6:]))[0]
    return rt.scenes.CONFIG_SCENES[name]()[0]


def meta_points(flat, name):
    """(points, how many of the leading ones are uniform in twice the bounds): winding_ref.query_points with the scene's seed"""
    n = META_UNIFORM.get(name, 600)
    return W.query_points(flat, sum(name.encode()), n), n


def uniform_points(flat, seed, n):
    """n points uniform in twice the bounds of the scene's TRIANGLES (the centre +- the full extent, as tools/winding_probe.py draws them:
    sphere50k's ground sphere of radius 100 would otherwise put nearly every point far from the whole mesh)"""
    tris = NR.sections(flat)[2]
    corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]]).astype(np.float64)
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo)
    return (mid + np.random.default_rng(seed).uniform(-1, 1, (n, 3)) * half).astype(np.float32)


def inside_points(flat, name):
    """the uniform points the inside bytes are compared over: in twice the triangle bounds"""
    return uniform_points(flat, 1000 + sum(name.encode()), META_UNIFORM.get(name, 2000))


def measure_scene(flat, tree, name):
    """per beta the worst and the mean |w_fast - w_exact| over winding_ref.query_points' points (the exact yardstick in binary32), the same
    over the uniform points in twice the triangle bounds, and at the default beta the share of those whose inside byte differs"""
    pts, _ = meta_points(flat, name)
    uni = inside_points(flat, name)
    exact, exact_uni = W.winding(flat, pts), W.winding(flat, uni)
    mom = moments(flat, tree)
    out = {"points": int(pts.shape[0]), "uniform_points": int(uni.shape[0]), "worst": {}, "mean": {}, "worst_uniform": {}}
    for beta in BETAS:
        fast, fast_uni = winding(flat, tree, pts, beta, mom=mom), winding(flat, tree, uni, beta, mom=mom)
        err = np.abs(fast.astype(np.float64) - exact.astype(np.float64))
        err = err[~np.isnan(err)]
        out["worst"]["%g" % beta] = float(err.max())
        out["mean"]["%g" % beta] = float(err.mean())
        out["worst_uniform"]["%g" % beta] = float(np.abs(fast_uni.astype(np.float64) - exact_uni.astype(np.float64)).max())
        if beta == float(BETA_DEFAULT):
            out["inside_differs"] = float((W.inside(fast_uni) != W.inside(exact_uni)).mean())
    return out


def measure_meta():
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rt = importlib.import_module("ray-tracer_amd")
    per = {}
    for name in META_SCENES:
        so = rt.SceneObjects(scene_objects(rt, name))
        flat, tree = so.debug_flatten(), so.debug_winding_tree()
        per[name] = measure_scene(flat, tree, name)
        if name == "sphere50k":
            c = work(flat, tree, uniform_points(flat, 77, WORK_POINTS), BETA_DEFAULT)
            per[name]["work"] = {"visits_mean": float(c[0].mean()), "terms_mean": float(c[1].mean()), "triangles": int(flat["num_triangles"])}
        print(name, json.dumps(per[name]), flush=True)
    return {"betas": list(BETAS), "per_scene": per, "margin": 4.0,
            "bound": "|w_fast - w_exact| <= margin * worst[beta] per scene over winding_ref.query_points' points, w_exact from tests/winding_ref.py in binary32"}


if __name__ == "__main__":
    meta = measure_meta()
    with open(META, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
