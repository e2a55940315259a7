"""The yardstick of the triangle-overlap queries (rt_overlap_triangles, include/rt_amd.h) in NumPy binary32: no product code, no pruning.

It reads a flattened scene (SceneObjects.debug_flatten() / Scene.debug_read()), walks each mesh's tree ONCE to give every triangle, for
every query, its path flag (overlap_ref.tree_paths on the query's bounding box: compares alone), evaluates EVERY candidate of every query
with the header's steps - the query's box, the two height tests, the in-plane axes of a coplanar pair, Moeller's intervals; a sphere by the
nearest section's point-triangle distance - and lists the overlapping ones in (object, triangle) order.  Every operation is one NumPy
float32 operation, so every intermediate is rounded once, as on the device (nothing is fused there).

    overlap(flat, tris, k=0, segments=False, detail=None) -> (counts [n] int32, any [n] uint8, ids [n, k] of ID_DTYPE[, segs [n, k] of
                                                SEG_DTYPE]): byte for byte what the library must answer; detail, a dict, receives the
                                                [n, C] matrices (hit; bare: without the path rule; boxes: step 1 alone; coplanar) and the
                                                candidates' objects and triangles
    query_triangles(flat, seed, n, sizes)    -> [n, 9]: the seeded queries of the tests

measure_meta() (tests/test_tritri_ref.py) is how tests/golden/tritri_meta.json was made (python tests/tritri_ref.py)."""
import json
import os

import numpy as np

from nearest_ref import OBJ_SPHERE, sections, tri_eval, triangle_owners
from overlap_ref import ID_DTYPE, OVERLAP_MAX, surface_bounds, tree_paths

SEG_DTYPE = np.dtype([("p", np.float32, (3,)), ("q", np.float32, (3,)), ("kind", np.int32), ("reserved", np.int32)])
CHUNK = 128             # queries evaluated at once: bounds the [queries, triangles] temporaries
F0 = np.float32(0)
NAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
META = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tritri_meta.json")


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def all3(f, h):
    return f(h[0]) & f(h[1]) & f(h[2])


def lone(h):
    """Moeller's sign rule: (l0, l1, l2), exactly one set"""
    c1, c2, c3, c4 = h[0] * h[1] > 0, h[0] * h[2] > 0, (h[1] * h[2] > 0) | (h[0] != 0), h[1] != 0
    l2 = c1 | (~c2 & ~c3 & ~c4)
    l1 = ~c1 & (c2 | (~c3 & c4))
    return ~l1 & ~l2, l1, l2


def cross_at(vl, vo, hl, ho):
    den = hl - ho
    return np.where(den == 0, vl, vl + (vo - vl) * (hl / den))


def ends(v, h, l):
    """the two ends of an interval: values v at heights h, the lone vertex l = (l0, l1, l2); the others in index order"""
    pick = lambda x: np.where(l[0], x[0], np.where(l[1], x[1], x[2]))
    vl, hl = pick(v), pick(h)
    va, ha = np.where(l[0], v[1], v[0]), np.where(l[0], h[1], h[0])
    vb, hb = np.where(l[0] | l[1], v[2], v[1]), np.where(l[0] | l[1], h[2], h[1])
    return cross_at(vl, va, hl, ha), cross_at(vl, vb, hl, hb)


def axis_separates(u, w):
    lt = gt = True
    for ui in u:
        for wj in w:
            lt, gt = lt & (ui < wj), gt & (ui > wj)
    return lt | gt


def prep(q):
    """valid [n], lo [n, 3], hi [n, 3] of the queries q [n, 9]"""
    a = q.reshape(-1, 3, 3)
    lo = np.fmin(np.fmin(a[:, 0], a[:, 1]), a[:, 2])
    hi = np.fmax(np.fmax(a[:, 0], a[:, 1]), a[:, 2])
    return np.isfinite(q).all(axis=1), lo, hi


def tri_test(t, q, lo, hi):
    """the records t [T, 12] against the queries q [n, 9] -> dict of [n, T]: boxes (step 1 passed), hit, coplanar, and the segment's
    p, q [n, T, 3] (meaningful where hit and not coplanar)"""
    a = [tuple(q[:, None, 3 * i + c] for c in range(3)) for i in range(3)]
    p0 = tuple(t[None, :, c] for c in range(3))
    s1 = tuple(t[None, :, 3 + c] for c in range(3))
    s2 = tuple(t[None, :, 6 + c] for c in range(3))
    qv = [p0, tuple(p0[c] + s1[c] for c in range(3)), tuple(p0[c] + s2[c] for c in range(3))]
    sep = False
    for c in range(3):
        l, h = lo[:, c:c + 1], hi[:, c:c + 1]
        sep = sep | ((qv[0][c] > h) & (qv[1][c] > h) & (qv[2][c] > h)) | ((qv[0][c] < l) & (qv[1][c] < l) & (qv[2][c] < l))
    boxes = ~sep
    z, e1, e2 = sub(a[0], a[0]), sub(a[1], a[0]), sub(a[2], a[0])
    na, nb = cross(e1, e2), cross(s1, s2)
    hA = [dot(nb, sub(a[i], p0)) for i in range(3)]
    ok = boxes & ~(all3(lambda x: x > 0, hA) | all3(lambda x: x < 0, hA))
    d = [sub(qv[j], a[0]) for j in range(3)]
    hB = [dot(na, d[j]) for j in range(3)]
    ok = ok & ~(all3(lambda x: x > 0, hB) | all3(lambda x: x < 0, hB))
    coplanar = all3(lambda x: x == 0, hA) | all3(lambda x: x == 0, hB)
    csep = False
    for n_, f in ((na, e1), (na, sub(a[2], a[1])), (na, sub(a[0], a[2])), (nb, s1), (nb, sub(s2, s1)), (nb, tuple(-s2[c] for c in range(3)))):
        X = cross(n_, f)
        csep = csep | axis_separates([dot(X, z), dot(X, e1), dot(X, e2)], [dot(X, d[j]) for j in range(3)])
    D = cross(na, nb)
    pA, pB = [dot(D, z), dot(D, e1), dot(D, e2)], [dot(D, d[j]) for j in range(3)]
    lA, lB = lone(hA), lone(hB)
    xA1, xA2 = ends(pA, hA, lA)
    xB1, xB2 = ends(pB, hB, lB)
    a_below = (xA1 < xB1) & (xA1 < xB2) & (xA2 < xB1) & (xA2 < xB2)
    b_below = (xB1 < xA1) & (xB1 < xA2) & (xB2 < xA1) & (xB2 < xA2)
    hit = ok & np.where(coplanar, ~csep, ~(a_below | b_below))
    a_in, b_in = xA1 <= xA2, xB1 <= xB2
    minA, maxA, minB, maxB = np.where(a_in, xA1, xA2), np.where(a_in, xA2, xA1), np.where(b_in, xB1, xB2), np.where(b_in, xB2, xB1)
    lower_b, upper_b = minB > minA, maxB < maxA
    P, Q = [], []
    for c in range(3):
        a1, a2 = ends([a[i][c] for i in range(3)], hA, lA)
        b1, b2 = ends([qv[j][c] for j in range(3)], hB, lB)
        P.append(np.where(lower_b, np.where(b_in, b1, b2), np.where(a_in, a1, a2)))
        Q.append(np.where(upper_b, np.where(b_in, b2, b1), np.where(a_in, a2, a1)))
    shape = np.broadcast(hit, coplanar).shape
    return {"boxes": np.broadcast_to(boxes, shape), "hit": np.broadcast_to(hit, shape), "coplanar": np.broadcast_to(coplanar & ok, shape),
            "p": np.stack([np.broadcast_to(x, shape) for x in P], axis=-1), "q": np.stack([np.broadcast_to(x, shape) for x in Q], axis=-1)}


def sphere_test(c, r, q):
    """spheres c [S, 3], r [S] against the queries q [n, 9] -> [n, S]"""
    rec = np.concatenate([q[:, 0:3], q[:, 3:6] - q[:, 0:3], q[:, 6:9] - q[:, 0:3], np.zeros((q.shape[0], 3), np.float32)], axis=1)
    near2, _ = tri_eval(rec[:, None, :], c[None, :, :])
    far2 = None
    for i in range(3):
        v = tuple(q[:, None, 3 * i + k] - c[None, :, k] for k in range(3))
        d2 = dot(v, v)
        far2 = d2 if far2 is None else np.fmax(far2, d2)
    rr = (r * r)[None, :]
    return (near2 <= rr) & (far2 >= rr)


def overlap(flat, tris_q, k=0, segments=False, detail=None):
    nodes, meshes, tris, objects = sections(flat)
    q_all = np.ascontiguousarray(tris_q, np.float32).reshape(-1, 9)
    n, T = q_all.shape[0], tris.shape[0]
    spheres = [i for i, ob in enumerate(objects) if ob["type"] == OBJ_SPHERE]
    S = len(spheres)
    owner = triangle_owners(objects, T)
    assert (owner >= 0).all(), "a triangle of the flattened scene that no object offers"
    sc = np.array([objects[i]["v"][0:3] for i in spheres], np.float32).reshape(-1, 3)
    sr = np.array([objects[i]["v"][3] for i in spheres], np.float32).reshape(-1)
    cand_obj = np.concatenate([np.asarray(spheres, np.int64), owner])
    cand_tri = np.concatenate([np.full(S, -1, np.int64), np.arange(T, dtype=np.int64)])
    order = np.lexsort((cand_tri, cand_obj))                      # the object, then the triangle
    cand_obj, cand_tri = cand_obj[order], cand_tri[order]
    C = cand_obj.shape[0]
    counts = np.zeros(n, np.int32)
    ids = np.zeros((n, k), ID_DTYPE)
    ids["object"] = ids["triangle"] = -1
    segs = np.zeros((n, k), SEG_DTYPE)
    keep = {name: [] for name in ("hit", "bare", "boxes", "coplanar")} if detail is not None else None
    with np.errstate(all="ignore"):
        for at in range(0, n, CHUNK):
            q = q_all[at:at + CHUNK]
            m = q.shape[0]
            valid, lo, hi = prep(q)
            hs = sphere_test(sc, sr, q) if S else np.zeros((m, 0), bool)
            if T:
                r = tri_test(tris, q, lo, hi)
                path = tree_paths(nodes, meshes, lo, hi, T)
            else:
                r = {"boxes": np.zeros((m, 0), bool), "hit": np.zeros((m, 0), bool), "coplanar": np.zeros((m, 0), bool),
                     "p": np.zeros((m, 0, 3), np.float32), "q": np.zeros((m, 0, 3), np.float32)}
                path = np.zeros((m, 0), bool)
            cat = lambda s_part, t_part: (np.concatenate([s_part, t_part], axis=1) & valid[:, None])[:, order]
            hit = cat(hs, r["hit"] & path)
            cop = cat(np.zeros_like(hs), r["coplanar"])
            P = np.concatenate([np.zeros((m, S, 3), np.float32), r["p"]], axis=1)[:, order]
            Q = np.concatenate([np.zeros((m, S, 3), np.float32), r["q"]], axis=1)[:, order]
            cnt = hit.sum(axis=1).astype(np.int32)
            counts[at:at + m] = cnt
            rank = np.cumsum(hit, axis=1) - 1
            rows_all = np.arange(m)
            for s in range(k):
                col = np.argmax(hit & (rank == s), axis=1)
                rows = cnt > s
                ids["object"][at:at + m][rows, s] = cand_obj[col[rows]]
                ids["triangle"][at:at + m][rows, s] = cand_tri[col[rows]]
                none = rows & ((cand_tri[col] < 0) | cop[rows_all, col])          # a sphere, or a coplanar pair: kind 2
                one = rows & ~none
                sg = segs[at:at + m]
                sg["kind"][one, s], sg["kind"][none, s] = 1, 2
                sg["p"][one, s], sg["q"][one, s] = P[rows_all, col][one], Q[rows_all, col][one]
                sg["p"][none, s] = sg["q"][none, s] = NAN
            if keep is not None:
                keep["hit"].append(hit)
                keep["bare"].append(cat(hs, r["hit"]))
                keep["boxes"].append(cat(np.ones_like(hs), r["boxes"]))
                keep["coplanar"].append(cop)
    if detail is not None:
        detail.update({name: (np.concatenate(v) if v else np.zeros((0, C), bool)) for name, v in keep.items()}, object=cand_obj, triangle=cand_tri)
    out = (counts, (counts > 0).astype(np.uint8), ids)
    return out + (segs,) if segments else out


# ---- the queries of the tests ----------------------------------------------------------------------------------------------------------
def query_triangles(flat, seed, n, sizes=(0.05, 0.1, 0.3)):
    """seeded query triangles: the centre uniform in the bounds of the scene's triangle records (surface_bounds), the three vertices the
    centre plus offsets uniform in +- size * diagonal per component, the sizes taken in turn"""
    rng = np.random.default_rng(seed)
    lo, hi = surface_bounds(flat)
    diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    centre = rng.uniform(lo, hi, (n, 3))
    size = np.asarray(sizes, np.float64)[np.arange(n) % len(sizes)]
    off = rng.uniform(-1.0, 1.0, (n, 3, 3)) * (size * diag)[:, None, None]
    return np.ascontiguousarray((centre[:, None, :] + off).astype(np.float32).reshape(n, 9))


def record_vertices(tris):
    """[T, 3, 3]: q0 = p0, q1 = p0 + s1, q2 = p0 + s2 as the test forms them (binary32)"""
    return np.stack([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]], axis=1).astype(np.float32)


def anchored_triangles(flat, seed, n, sizes=(0.05, 0.1, 0.3)):
    """seeded queries made to sit ON the scene, in turn: a query vertex on a scene vertex; a query edge through a scene vertex (its two
    ends the vertex minus and plus one offset); the query in a scene triangle's plane - where the triangle's vertices share a coordinate
    exactly (a cube's faces) a query with that coordinate, else the triangle's own vertices.  A scene without triangles gets
    query_triangles'"""
    _, _, tris, _ = sections(flat)
    if not tris.shape[0]:
        return query_triangles(flat, seed, n, sizes)
    rng = np.random.default_rng(seed)
    lo, hi = surface_bounds(flat)
    diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    V = record_vertices(tris)
    out = np.zeros((n, 3, 3), np.float32)
    for i in range(n):
        v = V[int(rng.integers(0, V.shape[0]))]
        size = np.float32(diag * sizes[(i // 3) % len(sizes)])
        off = rng.uniform(-1.0, 1.0, (3, 3)).astype(np.float32) * size
        anchor = v[int(rng.integers(0, 3))]
        if i % 3 == 0:
            out[i] = (anchor, anchor + off[1], anchor + off[2])
        elif i % 3 == 1:
            out[i] = (anchor - off[0], anchor + off[0], anchor + off[2])
        else:
            shared = [a for a in range(3) if v[0, a] == v[1, a] == v[2, a]]
            if shared:
                q = v.mean(axis=0, dtype=np.float32)[None, :] + off
                q[:, shared[0]] = v[0, shared[0]]
                out[i] = q
            else:
                out[i] = v
    return np.ascontiguousarray(out.reshape(n, 9))


def mesh_counts(flat, detail):
    """per query the overlapping triangles that belong to a mesh, and the number of mesh triangles in the scene"""
    is_mesh = np.array([int(ob["type"]) == 5 for ob in flat["objects"]])
    cols = (detail["triangle"] >= 0) & is_mesh[detail["object"]]
    return detail["hit"][:, cols].sum(axis=1), int(cols.sum())


if __name__ == "__main__":
    import test_tritri_ref as T
    meta = T.measure_meta()
    with open(META, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(meta, indent=1, sort_keys=True))
