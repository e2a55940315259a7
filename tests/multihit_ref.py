"""The yardstick of the multi-hit ray queries (rt_trace_rays_multi, include/rt_amd.h) in NumPy binary32: no product code, no pruning.

It reads a flattened scene (SceneObjects.debug_flatten() / Scene.debug_read()), walks each mesh's tree ONCE to give every triangle, for
every ray, its path flag (every box on the path passes the strict slab test) and its path value B (the largest entry distance on it),
evaluates EVERY candidate of every ray with the header's tests, and sorts them by the header's order.  Every operation is one NumPy float32
operation, so every intermediate is rounded once, as on the device (nothing is fused there).

    candidates(flat, o, d, tmax=None) -> Candidates: per ray every candidate's key, t, object, triangle and whether it counts, sorted
    multi(flat, o, d, k, tmax=None)   -> (hits [n, k] of HIT_DTYPE, counts [n]): byte for byte what the library must answer,
                                         but for the u, v of a sphere whose material needs them (not restated here: `sphere_uv` marks
                                         those records, and the tests hold them to the oracle)

measure_meta() is how tests/golden/multihit_meta.json was made (python tests/multihit_ref.py)."""
import json
import os

import numpy as np

from nearest_ref import OBJ_CUBOID, OBJ_ONE_WAY_QUAD, OBJ_QUAD, OBJ_SPHERE, REF_LEAF, dot, scene_bounds, sections, triangle_owners

HIT_DTYPE = np.dtype([("t", np.float32), ("point", np.float32, (3,)), ("normal", np.float32, (3,)), ("object", np.int32),
                      ("triangle", np.int32), ("u", np.float32), ("v", np.float32), ("reserved", np.int32)])
MISS_T = np.float32(2.0 ** 30)
EPS = np.float32(0.000001)
MULTIHIT_MAX = 8
CHUNK = 256             # rays evaluated at once: bounds the [rays, triangles] temporaries
F0, F1, F2, F4 = np.float32(0), np.float32(1), np.float32(2), np.float32(4)
META = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multihit_meta.json")


def slab(lo, hi, o, inv):
    """BoundingBox::ray_hits for the box (lo, hi) and rays (o, inv) [n, 3] -> passed [n], entry distance [n]; min / max drop a NaN operand"""
    tmin, tmax = np.zeros(o.shape[0], np.float32), np.full(o.shape[0], MISS_T, np.float32)
    for a in range(3):
        t1, t2 = (lo[a] - o[:, a]) * inv[:, a], (hi[a] - o[:, a]) * inv[:, a]
        tmin = np.fmax(tmin, np.fmin(t1, t2))
        tmax = np.fmin(tmax, np.fmax(t1, t2))
    return (tmin < tmax) & (tmax > F0), tmin


def tree_paths(nodes, meshes, o, inv, num_tris):
    """per ray and triangle: does every box on the path from the mesh's root box to the triangle's leaf pass the slab test, and B, the
    largest entry distance over those boxes (True and 0 for a triangle of no mesh)"""
    n = o.shape[0]
    ok, B = np.ones((n, num_tris), bool), np.zeros((n, num_tris), np.float32)
    refs = nodes.view(np.uint32)
    for m in range(meshes.shape[0]):
        h, t = slab(meshes[m, 0:3], meshes[m, 3:6], o, inv)
        stack = [(int(meshes[m].view(np.uint32)[6]), h, t)]
        while stack:
            ref, h, key = stack.pop()
            if ref & REF_LEAF:
                start, count = ref & 0xFFFFF, (ref >> 20) & 1023
                ok[:, start:start + count] = h[:, None]
                B[:, start:start + count] = key[:, None]
                continue
            q = nodes[ref & 0x3FFFFFFF]
            for lo, hi, child in ((q[0:3], q[3:6], int(refs[ref & 0x3FFFFFFF, 12])), (q[6:9], q[9:12], int(refs[ref & 0x3FFFFFFF, 13]))):
                ch, ct = slab(lo, hi, o, inv)
                stack.append((child, h & ch, np.where(ct < key, key, ct)))
    return ok, B


def tri_test(t, o, d):
    """Triangle::hit for the records t [..., 12] and rays o, d [..., 3] (broadcast) -> accepted, dist, u, v"""
    p0x, p0y, p0z, s1x, s1y, s1z, s2x, s2y, s2z = (t[..., k] for k in range(9))
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    px, py, pz = dy * s2z - dz * s2y, dz * s2x - dx * s2z, dx * s2y - dy * s2x
    det = dot(s1x, s1y, s1z, px, py, pz)
    inv_det = F1 / det
    tx, ty, tz = o[..., 0] - p0x, o[..., 1] - p0y, o[..., 2] - p0z
    u = dot(tx, ty, tz, px, py, pz) * inv_det
    qx, qy, qz = ty * s1z - tz * s1y, tz * s1x - tx * s1z, tx * s1y - ty * s1x
    v = dot(dx, dy, dz, qx, qy, qz) * inv_det
    w = F1 - u - v
    dist = dot(s2x, s2y, s2z, qx, qy, qz) * inv_det
    return (dist > EPS) & (u >= F0) & (v >= F0) & (w >= F0), dist, u, v


def sphere_test(c, r, o, d):
    """Sphere::hit's near root for spheres c [..., 3], r [...] and rays (broadcast) -> accepted, dist"""
    qx, qy, qz = c[..., 0] - o[..., 0], c[..., 1] - o[..., 1], c[..., 2] - o[..., 2]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    qa = dot(dx, dy, dz, dx, dy, dz)
    qb = dot(dx, dy, dz, qx, qy, qz) * np.float32(-2.0)
    qc = dot(qx, qy, qz, qx, qy, qz) - r * r
    disc = qb * qb - F4 * qa * qc
    dist = (-qb - np.sqrt(disc)) / (F2 * qa)
    return (disc >= F0) & (dist > EPS), dist


class Candidates:
    """per ray the candidates in the header's order: key, t, obj, tri [n, C] and counts [n, C] (False from the first that does not count on)"""

    def __init__(self, key, t, obj, tri, counts):
        self.key, self.t, self.obj, self.tri, self.counts = key, t, obj, tri, counts
        self.total = counts.sum(axis=1).astype(np.int32)


def candidates(flat, origins, directions, tmax=None):
    nodes, meshes, tris, objects = sections(flat)
    o_all = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d_all = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    n, T = o_all.shape[0], tris.shape[0]
    lim_all = np.full(n, MISS_T, np.float32)
    if tmax is not None:
        tm = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        lim_all = np.where(tm < MISS_T, tm, MISS_T)
        lim_all = np.where(np.isnan(tm), np.float32(-1), lim_all)              # a NaN limit counts nothing (no key is below 0)
    spheres = [i for i, ob in enumerate(objects) if ob["type"] == OBJ_SPHERE]
    owner = triangle_owners(objects, T)
    assert (owner >= 0).all(), "a triangle of the flattened scene that no object offers"
    sc = np.array([objects[i]["v"][0:3] for i in spheres], np.float32).reshape(-1, 3)
    sr = np.array([objects[i]["v"][3] for i in spheres], np.float32).reshape(-1)
    cand_obj = np.concatenate([np.asarray(spheres, np.int64), owner])
    cand_tri = np.concatenate([np.full(len(spheres), -1, np.int64), np.arange(T, dtype=np.int64)])
    C = cand_obj.shape[0]
    # the quads: (first record, one-way normal or None) of every quad of either kind and of every cuboid face
    firsts = []
    one_way = []
    for i, ob in enumerate(objects):
        t, s = int(ob["type"]), int(ob["prim_start"])
        if t in (OBJ_QUAD, OBJ_ONE_WAY_QUAD):
            firsts.append(s)
            if t == OBJ_ONE_WAY_QUAD:
                one_way.append((s, ob["v"][0:3].astype(np.float32)))
        elif t == OBJ_CUBOID:
            firsts += [s + 2 * f for f in range(6)]
    firsts = np.asarray(firsts, np.int64)
    keys, ts, objs_o, tris_o, cnts = [], [], [], [], []
    with np.errstate(all="ignore"):
        for at in range(0, n, CHUNK):
            o, d, lim = o_all[at:at + CHUNK], d_all[at:at + CHUNK], lim_all[at:at + CHUNK]
            m = o.shape[0]
            inv = F1 / d
            nan_dir = np.isnan(d).any(axis=1)
            hs, ds = sphere_test(sc[None, :, :], sr[None, :], o[:, None, :], d[:, None, :]) if spheres else (np.zeros((m, 0), bool), np.zeros((m, 0), np.float32))
            if T:
                ht, dt, _, _ = tri_test(tris[None, :, :], o[:, None, :], d[:, None, :])
                ht = ht.copy()
                if firsts.size:                                                 # Quad::hit: the first record if it hits, else the second
                    ht[:, firsts + 1] &= ~ht[:, firsts]
                for s, nrm in one_way:                                          # a one-way quad seen from behind offers nothing
                    back = dot(d[:, 0], d[:, 1], d[:, 2], nrm[0], nrm[1], nrm[2]) < F0
                    ht[:, s] &= ~back
                    ht[:, s + 1] &= ~back
                ok, B = tree_paths(nodes, meshes, o, inv, T)
                ht &= ok
                kt = np.where(dt < B, B, dt)
            else:
                ht, dt, kt = np.zeros((m, 0), bool), np.zeros((m, 0), np.float32), np.zeros((m, 0), np.float32)
            hit = np.concatenate([hs, ht], axis=1) & ~nan_dir[:, None]
            key = np.concatenate([ds, kt], axis=1)
            t = np.concatenate([ds, dt], axis=1)
            counts = hit & (key <= lim[:, None])
            sort_key = np.where(counts, key, np.float32(np.inf))
            ob, tb = np.broadcast_to(cand_obj[None, :], (m, C)), np.broadcast_to(cand_tri[None, :], (m, C))
            order = np.lexsort((tb, -ob, sort_key), axis=1)                    # key, then the higher object, then the lower triangle
            take = lambda a: np.take_along_axis(a, order, axis=1)
            keys.append(take(sort_key)); ts.append(take(t)); objs_o.append(take(ob)); tris_o.append(take(tb)); cnts.append(take(counts))
    if not keys:
        z = np.zeros((0, C))
        return Candidates(z.astype(np.float32), z.astype(np.float32), z.astype(np.int64), z.astype(np.int64), z.astype(bool))
    return Candidates(np.concatenate(keys), np.concatenate(ts), np.concatenate(objs_o), np.concatenate(tris_o), np.concatenate(cnts))


def normalised(x, y, z):
    m = x * x + y * y + z * z
    inv = F1 / np.sqrt(m)
    return x * inv, y * inv, z * inv


def records(flat, origins, directions, k, cand):
    """(hits [n, k], counts [n], sphere_uv [n, k]) from the sorted candidates: the first k that count, formed as rt_trace_rays forms a record"""
    _, _, tris, objects = sections(flat)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    n = o.shape[0]
    hits = np.zeros((n, k), HIT_DTYPE)
    hits["t"] = MISS_T
    hits["object"] = hits["triangle"] = -1
    sphere_uv = np.zeros((n, k), bool)
    counts = cand.total.copy() if k == 0 else np.minimum(cand.total, k).astype(np.int32)
    need_uv = objects["need_uv"] != 0
    uv = flat.get("tri_uv")
    with np.errstate(all="ignore"):
        for q in range(min(k, cand.key.shape[1])):
            rows = np.nonzero(cand.counts[:, q])[0]
            if not rows.size:
                continue
            t, ob, tr = cand.t[rows, q], cand.obj[rows, q], cand.tri[rows, q]
            oo, dd = o[rows], d[rows]
            P = np.stack([dd[:, a] * t + oo[:, a] for a in range(3)], axis=-1)
            N = np.zeros_like(P)
            U, V = np.zeros(rows.size, np.float32), np.zeros(rows.size, np.float32)
            is_s = tr < 0
            if is_s.any():
                c = np.array([objects[i]["v"][0:3] for i in ob[is_s]], np.float32).reshape(-1, 3)
                nx, ny, nz = normalised(P[is_s, 0] - c[:, 0], P[is_s, 1] - c[:, 1], P[is_s, 2] - c[:, 2])
                N[is_s] = np.stack([nx, ny, nz], axis=-1)
                sphere_uv[rows[is_s], q] = need_uv[ob[is_s]]
            if (~is_s).any():
                rec = tris[tr[~is_s]]
                nrm = rec[:, 9:12]
                along = dot(nrm[:, 0], nrm[:, 1], nrm[:, 2], dd[~is_s, 0], dd[~is_s, 1], dd[~is_s, 2]) > F0
                N[~is_s] = np.where(along[:, None], -nrm, nrm)
                want = need_uv[ob[~is_s]]
                if want.any():
                    _, _, u, v = tri_test(rec, oo[~is_s], dd[~is_s])
                    w = F1 - u - v
                    c = uv[tr[~is_s]]
                    tu = c[:, 0] * w + c[:, 2] * u + c[:, 4] * v
                    tv = c[:, 1] * w + c[:, 3] * u + c[:, 5] * v
                    idx = np.nonzero(~is_s)[0]
                    U[idx] = np.where(want, tu, F0)
                    V[idx] = np.where(want, tv, F0)
            h = hits[:, q]
            h["t"][rows] = t
            h["point"][rows] = P
            h["normal"][rows] = N
            h["object"][rows] = ob
            h["triangle"][rows] = tr
            h["u"][rows] = U
            h["v"][rows] = V
    return hits, counts, sphere_uv


def multi(flat, origins, directions, k, tmax=None, cand=None):
    cand = cand if cand is not None else candidates(flat, origins, directions, tmax)
    hits, counts, _ = records(flat, origins, directions, k, cand)
    return hits, counts


# ---- the rays of the tests -----------------------------------------------------------------------------------------------------------
def query_rays(flat, seed, n):
    """seeded rays for a scene: origins on a sphere around the bounds of its triangles (of everything, without triangles); half of them
    aimed at uniform points inside the bounds, half through two anchors - sphere centres and triangle centroids, the second one jittered -
    so that many rays cross several surfaces; and a share of the committed fixture rays (tests/golden/ref)"""
    import reference_fixtures as RF
    rng = np.random.default_rng(seed)
    _, _, tris, objects = sections(flat)
    lo, hi = scene_bounds(flat)
    if tris.shape[0]:
        corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
    mid, half = (lo + hi) / np.float32(2), (hi - lo) / np.float32(2)
    radius = np.float32(1.5) * np.sqrt((half * half).sum(dtype=np.float32))
    n_fix = n // 8
    n_uni = (n - n_fix) // 2
    n_anc = n - n_fix - n_uni
    u = rng.normal(0, 1, (n_uni, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    org = (mid + radius * u).astype(np.float32)
    target = rng.uniform(mid - half * np.float32(0.8), mid + half * np.float32(0.8), (n_uni, 3)).astype(np.float32)
    dirs = (target - org).astype(np.float32)
    dirs[::3] *= np.float32(0.37)                                              # the direction is taken as given: not unit length
    anchors = [np.asarray(ob["v"][0:3], np.float32)[None, :] for ob in objects if ob["type"] == OBJ_SPHERE]
    if tris.shape[0]:
        anchors.append(tris[:, 0:3] + (tris[:, 3:6] + tris[:, 6:9]) / np.float32(3))
    anchors = np.concatenate(anchors).astype(np.float32)
    a = anchors[rng.integers(0, anchors.shape[0], n_anc)]
    b = anchors[rng.integers(0, anchors.shape[0], n_anc)] + rng.normal(0, 0.02, (n_anc, 3)) * half
    v = (b - a).astype(np.float64)
    v[np.linalg.norm(v, axis=1) < 1e-6] = (0.0, 0.0, 1.0)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    aorg = (a - (np.float32(2) * radius + np.linalg.norm(a - mid, axis=1, keepdims=True)) * v).astype(np.float32)
    adir = (v * rng.uniform(0.3, 2.5, (n_anc, 1))).astype(np.float32)
    fo, fd = RF.rays()
    pick = rng.choice(fo.shape[0], n_fix, replace=False)
    return np.ascontiguousarray(np.concatenate([org, aorg, fo[pick]])), np.ascontiguousarray(np.concatenate([dirs, adir, fd[pick]]))


def oracle_first(orc_scene, o, d):
    """(t as uint32, object) of trace_one per ray: -1 and MISS_T for a miss"""
    t = np.full(o.shape[0], MISS_T, np.float32)
    ob = np.full(o.shape[0], -1, np.int64)
    for i in range(o.shape[0]):
        hit, out = orc_scene.trace_one(o[i], d[i])
        if hit:
            t[i], ob[i] = out[0], int(out[7])
    return t.view(np.uint32), ob


def set_d(flat, orc_scene, o, d, cand=None):
    """the rays whose record 0 differs from the oracle's closest hit in t or object: ties inside a mesh, and where the clamp reorders"""
    cand = cand if cand is not None else candidates(flat, o, d)
    hits, _ = multi(flat, o, d, 1, cand=cand)
    t, ob = oracle_first(orc_scene, o, d)
    return (hits["t"][:, 0].view(np.uint32) != t) | (hits["object"][:, 0] != ob)


if __name__ == "__main__":
    import test_multihit_ref as T
    meta = T.measure_meta()
    with open(META, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(meta, indent=1, sort_keys=True))
