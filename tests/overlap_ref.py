"""The yardstick of the box-overlap queries (rt_overlap_boxes, include/rt_amd.h) in NumPy binary32: no product code, no pruning.

It reads a flattened scene (SceneObjects.debug_flatten() / Scene.debug_read()), walks each mesh's tree ONCE to give every triangle, for
every box, its path flag (every box on the path overlaps the query box, by compares alone), evaluates EVERY candidate of every box with
the header's tests - the sphere's two distances, the thirteen separating axes of a triangle record - and lists the overlapping ones in
(object, triangle) order.  Every operation is one NumPy float32 operation, so every intermediate is rounded once, as on the device
(nothing is fused there).

    overlap(flat, lo, hi, k=0, detail=None) -> (counts [n] int32, any [n] uint8, ids [n, k] of ID_DTYPE): byte for byte what the
                                                library must answer; detail, a dict, receives the [n, C] matrices (bare: the tests
                                                without the path rule) and the candidates' objects and triangles
    query_boxes(flat, seed, n)              -> (lo, hi): the seeded boxes of the tests

measure_meta() (tests/test_overlap_ref.py) is how tests/golden/overlap_meta.json was made (python tests/overlap_ref.py)."""
import json
import os

import numpy as np

from nearest_ref import OBJ_SPHERE, REF_LEAF, scene_bounds, sections, triangle_owners

ID_DTYPE = np.dtype([("object", np.int32), ("triangle", np.int32)])
OVERLAP_MAX = 8
CHUNK = 256             # boxes evaluated at once: bounds the [boxes, triangles] temporaries
F0, HALF = np.float32(0), np.float32(0.5)
META = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_meta.json")


def box_prep(lo, hi):
    """valid [n], centre [n, 3], half extents [n, 3] of the boxes (lo, hi) [n, 3]"""
    valid = np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1)
    return valid, lo * HALF + hi * HALF, hi * HALF - lo * HALF


def boxes_overlap(nlo, nhi, lo, hi):
    """the node box (nlo, nhi: 3 floats) against the boxes (lo, hi) [n, 3]: compares alone"""
    return ((nlo[None, :] <= hi) & (lo <= nhi[None, :])).all(axis=1)


def tree_paths(nodes, meshes, lo, hi, num_tris):
    """per box and triangle: does every box on the path from the mesh's root box to the triangle's leaf overlap the query box (True for a
    triangle of no mesh)"""
    ok = np.ones((lo.shape[0], num_tris), bool)
    refs = nodes.view(np.uint32)
    for m in range(meshes.shape[0]):
        stack = [(int(meshes[m].view(np.uint32)[6]), boxes_overlap(meshes[m, 0:3], meshes[m, 3:6], lo, hi))]
        while stack:
            ref, h = stack.pop()
            if ref & REF_LEAF:
                start, count = ref & 0xFFFFF, (ref >> 20) & 1023
                ok[:, start:start + count] = h[:, None]
                continue
            q = nodes[ref & 0x3FFFFFFF]
            for nlo, nhi, child in ((q[0:3], q[3:6], int(refs[ref & 0x3FFFFFFF, 12])), (q[6:9], q[9:12], int(refs[ref & 0x3FFFFFFF, 13]))):
                stack.append((child, h & boxes_overlap(nlo, nhi, lo, hi)))
    return ok


def sphere_test(c, r, lo, hi):
    """spheres c [S, 3], r [S] against boxes [n, 3] -> [n, S]: the nearest point of the box no farther than r, the farthest no nearer"""
    cs, l, h = c[None, :, :], lo[:, None, :], hi[:, None, :]
    e = np.fmax(np.fmax(l - cs, cs - h), F0)
    g = np.fmax(cs - l, h - cs)
    dmin2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    dmax2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    rr = (r * r)[None, :]
    return (dmin2 <= rr) & (dmax2 >= rr)


def axis_separates(p0, p1, p2, rad):
    neg = -rad
    return ((p0 > rad) & (p1 > rad) & (p2 > rad)) | ((p0 < neg) & (p1 < neg) & (p2 < neg))


def tri_test(t, lo, hi, c, h):
    """the thirteen axes for the records t [T, 12] and the boxes [n, 3] -> overlaps [n, T] (no axis separates)"""
    ax, ay, az, s1x, s1y, s1z, s2x, s2y, s2z = (t[None, :, k] for k in range(9))
    bx, by, bz, cx, cy, cz = ax + s1x, ay + s1y, az + s1z, ax + s2x, ay + s2y, az + s2z
    lox, loy, loz, hix, hiy, hiz = (a[:, k:k + 1] for a in (lo, hi) for k in range(3))
    ccx, ccy, ccz, hx, hy, hz = (a[:, k:k + 1] for a in (c, h) for k in range(3))
    sep = ((ax > hix) & (bx > hix) & (cx > hix)) | ((ax < lox) & (bx < lox) & (cx < lox))
    sep |= ((ay > hiy) & (by > hiy) & (cy > hiy)) | ((ay < loy) & (by < loy) & (cy < loy))
    sep |= ((az > hiz) & (bz > hiz) & (cz > hiz)) | ((az < loz) & (bz < loz) & (cz < loz))
    v = [(ax - ccx, ay - ccy, az - ccz), (bx - ccx, by - ccy, bz - ccz), (cx - ccx, cy - ccy, cz - ccz)]
    nx, ny, nz = s1y * s2z - s1z * s2y, s1z * s2x - s1x * s2z, s1x * s2y - s1y * s2x
    d = (nx * v[0][0] + ny * v[0][1]) + nz * v[0][2]
    r = (hx * np.abs(nx) + hy * np.abs(ny)) + hz * np.abs(nz)
    sep |= (d > r) | (d < -r)
    for fx, fy, fz in ((s1x, s1y, s1z), (s2x - s1x, s2y - s1y, s2z - s1z), (-s2x, -s2y, -s2z)):
        fax, fay, faz = np.abs(fx), np.abs(fy), np.abs(fz)
        sep |= axis_separates(*[w[2] * fy - w[1] * fz for w in v], hy * faz + hz * fay)
        sep |= axis_separates(*[w[0] * fz - w[2] * fx for w in v], hx * faz + hz * fax)
        sep |= axis_separates(*[w[1] * fx - w[0] * fy for w in v], hx * fay + hy * fax)
    return ~sep


def overlap(flat, lo, hi, k=0, detail=None):
    nodes, meshes, tris, objects = sections(flat)
    lo_all = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
    hi_all = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
    n, T = lo_all.shape[0], tris.shape[0]
    spheres = [i for i, ob in enumerate(objects) if ob["type"] == OBJ_SPHERE]
    owner = triangle_owners(objects, T)
    assert (owner >= 0).all(), "a triangle of the flattened scene that no object offers"
    sc = np.array([objects[i]["v"][0:3] for i in spheres], np.float32).reshape(-1, 3)
    sr = np.array([objects[i]["v"][3] for i in spheres], np.float32).reshape(-1)
    cand_obj = np.concatenate([np.asarray(spheres, np.int64), owner])
    cand_tri = np.concatenate([np.full(len(spheres), -1, np.int64), np.arange(T, dtype=np.int64)])
    order = np.lexsort((cand_tri, cand_obj))                      # the object, then the triangle
    cand_obj, cand_tri = cand_obj[order], cand_tri[order]
    C = cand_obj.shape[0]
    hits, bares = [], []
    with np.errstate(all="ignore"):
        for at in range(0, n, CHUNK):
            l, h = lo_all[at:at + CHUNK], hi_all[at:at + CHUNK]
            valid, c, half = box_prep(l, h)
            hs = sphere_test(sc, sr, l, h) if spheres else np.zeros((l.shape[0], 0), bool)
            bare_t = tri_test(tris, l, h, c, half) if T else np.zeros((l.shape[0], 0), bool)
            ht = bare_t & tree_paths(nodes, meshes, l, h, T) if T else bare_t
            hits.append((np.concatenate([hs, ht], axis=1) & valid[:, None])[:, order])
            bares.append((np.concatenate([hs, bare_t], axis=1) & valid[:, None])[:, order])
    hit = np.concatenate(hits) if hits else np.zeros((0, C), bool)
    counts = hit.sum(axis=1).astype(np.int32)
    ids = np.zeros((n, k), ID_DTYPE)
    ids["object"] = ids["triangle"] = -1
    rank = np.cumsum(hit, axis=1) - 1
    for q in range(k):
        col = np.argmax(hit & (rank == q), axis=1)
        rows = counts > q
        ids["object"][rows, q] = cand_obj[col[rows]]
        ids["triangle"][rows, q] = cand_tri[col[rows]]
    if detail is not None:
        detail.update(hit=hit, bare=np.concatenate(bares) if bares else hit, object=cand_obj, triangle=cand_tri)
    return counts, (counts > 0).astype(np.uint8), ids


# ---- the boxes of the tests ----------------------------------------------------------------------------------------------------------
def planes(flat):
    """per axis the coordinates a box face can be snapped to: every vertex coordinate as the test forms it (p0, p0 + s1, p0 + s2 in
    binary32) and every plane of a mesh's root box and of a node's child boxes; without triangles, the spheres' extremes"""
    nodes, meshes, tris, _ = sections(flat)
    out = []
    for a in range(3):
        vals = [tris[:, a], tris[:, a] + tris[:, 3 + a], tris[:, a] + tris[:, 6 + a], meshes[:, a], meshes[:, 3 + a], nodes[:, a], nodes[:, 3 + a],
                nodes[:, 6 + a], nodes[:, 9 + a]]
        v = np.unique(np.concatenate(vals).astype(np.float32))
        v = v[np.isfinite(v)]
        if not v.size:
            lo, hi = scene_bounds(flat)
            v = np.array([lo[a], hi[a]], np.float32)
        out.append(v)
    return out


def surface_bounds(flat):
    """(lo, hi) over the triangle vertices alone - what the meshes and the other triangle records span; the scene's bounds where there is
    no triangle.  Most scenes of the suite stand on a sphere of radius 100: their scene_bounds are 200 wide around meshes about 1 across"""
    _, _, tris, _ = sections(flat)
    if not tris.shape[0]:
        return scene_bounds(flat)
    corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
    return corners.min(axis=0), corners.max(axis=0)


def anchors(flat):
    """what a box face is snapped against together with where the box then has to be on the other two axes for the face to DECIDE the
    answer: (points [P, 3], boxes_lo [B, 3], boxes_hi [B, 3]) - every vertex as the test forms it, every mesh's root box and every
    node's two child boxes"""
    nodes, meshes, tris, _ = sections(flat)
    pts = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]]).astype(np.float32).reshape(-1, 3)
    blo = np.concatenate([meshes[:, 0:3], nodes[:, 0:3], nodes[:, 6:9]]).astype(np.float32).reshape(-1, 3)
    bhi = np.concatenate([meshes[:, 3:6], nodes[:, 3:6], nodes[:, 9:12]]).astype(np.float32).reshape(-1, 3)
    ok = np.isfinite(blo).all(axis=1) & np.isfinite(bhi).all(axis=1) & (blo <= bhi).all(axis=1)
    return pts, blo[ok], bhi[ok]


def query_boxes(flat, seed, n):
    """seeded boxes for a scene.  The first half: centres uniform in twice the scene's bounds, extents per axis log-uniform from 1e-3 to 1
    of its diagonal; every fourth of them is moved along one axis so that one of its faces coincides exactly with a vertex coordinate or
    a node-box plane of the scene (the closed <=).  The second half is drawn the same way from the bounds of the triangle records alone
    (surface_bounds: where the meshes are, whatever ground sphere the scene stands on), and every fourth of THOSE is snapped against an
    anchor - a vertex, a mesh's root box or a node's child box - and placed on the other two axes where the anchor is, so that the face
    that coincides is the one that decides whether the box touches: beside the anchor (touching only) or over it, in turn"""
    rng = np.random.default_rng(seed)
    n_scene = n - n // 2
    parts = []
    for (lo, hi), m in ((scene_bounds(flat), n_scene), (surface_bounds(flat), n // 2)):
        mid, half = (lo + hi) / np.float32(2), (hi - lo)
        diag = float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
        centre = rng.uniform(mid - half, mid + half, (m, 3))
        extent = diag * 10.0 ** rng.uniform(-3.0, 0.0, (m, 3))
        parts.append(((centre - extent / 2).astype(np.float32), (centre + extent / 2).astype(np.float32)))
    blo, bhi = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    pl = planes(flat)
    pts, alo, ahi = anchors(flat)
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    pick, where = rng.random(n), rng.uniform(-0.45, 0.45, (n, 3))
    for i in range(0, n, 4):
        a = int(axis[i])
        e = (bhi[i] - blo[i]).astype(np.float32)
        v = pl[a][int(pick[i] * pl[a].shape[0])]
        if i >= n_scene and pts.shape[0] + alo.shape[0]:
            j = int(pick[i] * (pts.shape[0] + alo.shape[0]))
            if j < pts.shape[0]:                                       # a vertex: the box reaches it on the other two axes
                v, c = pts[j, a], pts[j] + where[i] * e
            else:                                                      # a box of the tree: one of its two planes on this axis, the box somewhere over its face
                j -= pts.shape[0]
                v = (alo if (i // 4) % 2 else ahi)[j, a]
                c = alo[j] + (where[i] + 0.5) * (ahi[j] - alo[j])
            blo[i], bhi[i] = (c - e / 2).astype(np.float32), (c + e / 2).astype(np.float32)
        if side[i]:
            blo[i, a], bhi[i, a] = v, np.float32(v + e[a])
        else:
            blo[i, a], bhi[i, a] = np.float32(v - e[a]), v
    assert (blo <= bhi).all()
    return np.ascontiguousarray(blo), np.ascontiguousarray(bhi)


def mesh_counts(flat, detail):
    """per box the overlapping triangles that belong to a mesh, and the number of mesh triangles in the scene: a count strictly between 0
    and that number means a walk that entered the tree and pruned"""
    is_mesh = np.array([int(ob["type"]) == 5 for ob in flat["objects"]])
    cols = (detail["triangle"] >= 0) & is_mesh[detail["object"]]
    return detail["hit"][:, cols].sum(axis=1), int(cols.sum())


if __name__ == "__main__":
    import test_overlap_ref as T
    meta = T.measure_meta()
    with open(META, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(meta, indent=1, sort_keys=True))
