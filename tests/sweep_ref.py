"""The yardstick of the sphere-cast queries (rt_sweep_spheres, include/rt_amd.h) in NumPy binary32: no product code, no traversal.

It reads a flattened scene (SceneObjects.debug_flatten() / Scene.debug_read()), walks each mesh's tree ONCE to give every triangle, for
every ball, its path flag (every box on the path, inflated by the ball's radius, passes the slab test) and its path value B (the largest
entry distance on it), evaluates EVERY candidate of every ball - a sphere's root, a triangle's seven features - with the header's formulas
in the header's order, and applies the winner rule.  The start overlap is nearest_ref.nearest's answer, as the header defines it.  Every
operation is one NumPy float32 operation, so every intermediate is rounded once, as on the device (nothing is fused there).

    sweep(flat, origins, directions, radius, tmax=None) -> records of DTYPE, byte for byte what the library must answer
    kinds(flat, records, ...)                            -> what each query's outcome was, for the coverage conditions of the tests
    query_sweeps(flat, seed, n)                          -> the seeded balls of the tests: (origins, directions, radius)

sweep64 finds the first contact in binary64 by another method - conservative advancement on the point-triangle distance field, none of the
formulas here: what test_sweep_ref.py holds the yardstick's own error against."""
import numpy as np

import nearest_ref as NR
from nearest_ref import OBJ_MESH, OBJ_SPHERE, REF_LEAF, dot, scene_bounds, sections, triangle_owners

DTYPE = np.dtype([("t", np.float32), ("centre", np.float32, (3,)), ("point", np.float32, (3,)), ("object", np.int32), ("triangle", np.int32),
                  ("feature", np.int32), ("overlap", np.int32), ("reserved", np.int32)])
MISS_T = np.float32(2.0 ** 30)
CHUNK = 128             # balls evaluated at once: bounds the [balls, triangles] temporaries
F0, F1 = np.float32(0), np.float32(1)


def floor0(t):
    return np.where(t <= 0, np.zeros_like(t), t)


def ball(mx, my, mz, d, dd, rad, far=False):
    """a root of |m + t d| = rad, taken from the path's point nearest the centre (t0 on): the near one, offered while approaching, or the far
    one -> ok, t"""
    b = dot(mx, my, mz, d[0], d[1], d[2])
    t0 = -b / dd
    nx, ny, nz = d[0] * t0 + mx, d[1] * t0 + my, d[2] * t0 + mz
    b2 = dot(nx, ny, nz, d[0], d[1], d[2])
    c2 = dot(nx, ny, nz, nx, ny, nz) - rad * rad
    disc = b2 * b2 - dd * c2
    root = np.sqrt(disc)
    if far:
        return disc >= 0, floor0(t0 + (-b2 + root) / dd)
    return (disc >= 0) & (b < 0), floor0(t0 + (-b2 - root) / dd)


def sphere_cand(c, R, o, d, dd, r):
    """spheres c (3 arrays), R and balls (broadcast) -> ok, t"""
    mx, my, mz = o[0] - c[0], o[1] - c[1], o[2] - c[2]
    outside = dot(mx, my, mz, mx, my, mz) > R * R
    rad = np.where(outside, R + r, R - r)
    ok_o, t_o = ball(mx, my, mz, d, dd, rad)
    ok_i, t_i = ball(mx, my, mz, d, dd, rad, far=True)
    return np.where(outside, ok_o, ok_i & (rad > 0)), np.where(outside, t_o, t_i)


def edge(e, m, d, dd, rr):
    """the cylinder about the edge (A, e), m = o - A, the root taken from the foot of the common perpendicular -> ok, t, s"""
    ee, de, me = dot(e[0], e[1], e[2], e[0], e[1], e[2]), dot(d[0], d[1], d[2], e[0], e[1], e[2]), dot(m[0], m[1], m[2], e[0], e[1], e[2])
    md = dot(m[0], m[1], m[2], d[0], d[1], d[2])
    a, b = ee * dd - de * de, ee * md - de * me
    t0 = -b / a
    nx, ny, nz = d[0] * t0 + m[0], d[1] * t0 + m[1], d[2] * t0 + m[2]
    s0 = dot(nx, ny, nz, e[0], e[1], e[2]) / ee
    px, py, pz = nx - e[0] * s0, ny - e[1] * s0, nz - e[2] * s0
    me2, md2, mm2 = dot(px, py, pz, e[0], e[1], e[2]), dot(px, py, pz, d[0], d[1], d[2]), dot(px, py, pz, px, py, pz)
    b2, c2 = ee * md2 - de * me2, ee * (mm2 - rr) - me2 * me2
    disc = b2 * b2 - a * c2
    t1 = (-b2 - np.sqrt(disc)) / a
    t = floor0(t0 + t1)
    s = s0 + (me2 + t1 * de) / ee
    return (a > 0) & (disc >= 0) & (b < 0) & (s >= 0) & (s <= 1), t, s


def face(p0, s1, s2, ap, o, d, r):
    """-> ok, t, point (3 arrays)"""
    nx, ny, nz = s1[1] * s2[2] - s1[2] * s2[1], s1[2] * s2[0] - s1[0] * s2[2], s1[0] * s2[1] - s1[1] * s2[0]
    nn = dot(nx, ny, nz, nx, ny, nz)
    ln = np.sqrt(nn)
    h, dn = dot(ap[0], ap[1], ap[2], nx, ny, nz), dot(d[0], d[1], d[2], nx, ny, nz)
    neg = h < 0
    hs, ds = np.where(neg, -h, h), np.where(neg, -dn, dn)
    rl = r * ln
    t = floor0((rl - hs) / ds)
    cx, cy, cz = d[0] * t + o[0], d[1] * t + o[1], d[2] * t + o[2]
    k = r / ln
    ks = np.where(neg, -k, k)
    px, py, pz = cx - nx * ks, cy - ny * ks, cz - nz * ks
    wx, wy, wz = px - p0[0], py - p0[1], pz - p0[2]
    d00, d01, d11 = dot(s1[0], s1[1], s1[2], s1[0], s1[1], s1[2]), dot(s1[0], s1[1], s1[2], s2[0], s2[1], s2[2]), dot(s2[0], s2[1], s2[2], s2[0], s2[1], s2[2])
    d20, d21 = dot(wx, wy, wz, s1[0], s1[1], s1[2]), dot(wx, wy, wz, s2[0], s2[1], s2[2])
    vn, wn, den = d11 * d20 - d01 * d21, d00 * d21 - d01 * d20, d00 * d11 - d01 * d01
    return (nn > 0) & (hs >= rl) & (ds < 0) & (vn >= 0) & (wn >= 0) & (vn + wn <= den), t, (px, py, pz)


def _parts(t, o):
    p0, s1, s2 = (t[..., 0], t[..., 1], t[..., 2]), (t[..., 3], t[..., 4], t[..., 5]), (t[..., 6], t[..., 7], t[..., 8])
    ap = (o[0] - p0[0], o[1] - p0[1], o[2] - p0[2])
    bp = (ap[0] - s1[0], ap[1] - s1[1], ap[2] - s1[2])
    cp = (ap[0] - s2[0], ap[1] - s2[1], ap[2] - s2[2])
    e3 = (s2[0] - s1[0], s2[1] - s1[1], s2[2] - s1[2])
    return p0, s1, s2, ap, bp, cp, e3


def tri_features(t, o, d, dd, r):
    """the seven features of the records t [..., 12] for balls o, d (3 arrays each), dd, r (broadcast) -> list of (ok, t)"""
    p0, s1, s2, ap, bp, cp, e3 = _parts(t, o)
    rr = r * r
    fk, ft, _ = face(p0, s1, s2, ap, o, d, r)
    out = [(fk, ft)]
    for e, m in ((s1, ap), (s2, ap), (e3, bp)):
        ok, te, _ = edge(e, m, d, dd, rr)
        out.append((ok, te))
    for m in (ap, bp, cp):
        out.append(ball(m[0], m[1], m[2], d, dd, r))
    return out


def tri_cand(t, o, d, dd, r):
    """-> (smallest t, its feature): +Inf and -1 where no feature offers one; the lower index on equal t; a NaN is never smaller"""
    feats = tri_features(t, o, d, dd, r)
    shape = np.broadcast(feats[0][1], feats[6][1]).shape
    best, which = np.full(shape, np.inf, np.float32), np.full(shape, -1, np.int32)
    for k, (ok, tk) in enumerate(feats):
        take = ok & (tk < best)
        best, which = np.where(take, tk, best), np.where(take, np.int32(k), which)
    return best, which


def tri_point(t, o, d, dd, r, feature):
    """the contact point of the winners: records t [n, 12], one ball and one feature each -> [n, 3]"""
    p0, s1, s2, ap, bp, cp, e3 = _parts(t, o)
    _, _, fp = face(p0, s1, s2, ap, o, d, r)
    pts = [fp]
    rr = r * r
    for A, e, m in ((p0, s1, ap), (p0, s2, ap), ((p0[0] + s1[0], p0[1] + s1[1], p0[2] + s1[2]), e3, bp)):
        _, _, s = edge(e, m, d, dd, rr)
        pts.append((A[0] + e[0] * s, A[1] + e[1] * s, A[2] + e[2] * s))
    pts += [p0, (p0[0] + s1[0], p0[1] + s1[1], p0[2] + s1[2]), (p0[0] + s2[0], p0[1] + s2[1], p0[2] + s2[2])]
    out = np.zeros((feature.shape[0], 3), np.float32)
    for k in range(7):
        m = feature == k
        for a in range(3):
            out[m, a] = np.broadcast_to(pts[k][a], feature.shape)[m]
    return out


def tree_paths(nodes, meshes, o, inv, r, num_tris):
    """per ball and triangle: does every box on the path from the mesh's root box to the triangle's leaf, inflated by r, pass the slab test,
    and B, the largest entry distance over those boxes (True and 0 for a triangle of no mesh).  o, inv [n, 3], r [n]"""
    n = o.shape[0]
    ok, B = np.ones((n, num_tris), bool), np.zeros((n, num_tris), np.float32)
    refs = nodes.view(np.uint32)

    def inflated(lo, hi):
        return slab_rows(lo[None, :] - r[:, None], hi[None, :] + r[:, None], o, inv)
    for m in range(meshes.shape[0]):
        h, t = inflated(meshes[m, 0:3], meshes[m, 3:6])
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
                ch, ct = inflated(lo, hi)
                stack.append((child, h & ch, np.where(ct < key, key, ct)))
    return ok, B


def slab_rows(lo, hi, o, inv):
    """multihit_ref.slab with a box per ray: lo, hi [n, 3]"""
    tmin, tmax = np.zeros(o.shape[0], np.float32), np.full(o.shape[0], MISS_T, np.float32)
    for a in range(3):
        t1, t2 = (lo[:, a] - o[:, a]) * inv[:, a], (hi[:, a] - o[:, a]) * inv[:, a]
        tmin = np.fmax(tmin, np.fmin(t1, t2))
        tmax = np.fmin(tmax, np.fmax(t1, t2))
    return (tmin < tmax) & (tmax > F0), tmin


def _inputs(origins, directions, radius, tmax):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    n = o.shape[0]
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), (n,)))
    tm = None if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
    return o, d, r, tm, n


def valid_inputs(o, d, r, tm):
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & ~(d == 0).all(axis=1) & np.isfinite(r) & (r >= 0)
    lim = np.full(o.shape[0], MISS_T, np.float32)
    if tm is not None:
        with np.errstate(all="ignore"):
            ok &= tm > 0
            lim = np.where(tm < MISS_T, tm, MISS_T)
    return ok, lim


def sweep(flat, origins, directions, radius, tmax=None, detail=None):
    """the records the library must answer.  detail, a dict, receives "key" (the winner's K, NaN where there is none), "dropped" (a
    candidate existed but none within the limit) and "valid" (the input was one that is looked at)"""
    rec, det = sweep_many(flat, origins, directions, radius, [tmax])[0]
    if detail is not None:
        detail.update(det)
    return rec


def sweep_many(flat, origins, directions, radius, limits):
    """sweep for several limit settings (each None, a scalar or [n]) over one evaluation of the candidates -> [(records, detail)]"""
    nodes, meshes, tris, objects = sections(flat)
    T = tris.shape[0]
    runs = []
    for tmax in limits:
        o_all, d_all, r_all, tm_all, n = _inputs(origins, directions, radius, tmax)
        out = np.zeros(n, DTYPE)
        out["t"] = MISS_T
        out["object"] = out["triangle"] = out["feature"] = -1
        ok, lim = valid_inputs(o_all, d_all, r_all, tm_all)
        runs.append({"out": out, "ok": ok, "lim": lim, "key": np.full(n, np.nan, np.float32), "dropped": np.zeros(n, bool)})
    ok_geo, _ = valid_inputs(o_all, d_all, r_all, None)
    with np.errstate(all="ignore"):
        near = NR.nearest(flat, np.where(ok_geo[:, None], o_all, F0), np.where(ok_geo, r_all, np.float32(-1)))
    over_geo = ok_geo & (near["object"] >= 0)
    for run in runs:
        over, out = run["ok"] & over_geo, run["out"]
        out["t"][over] = F0
        out["centre"][over] = o_all[over]
        out["point"][over] = near["point"][over]
        out["object"][over] = near["object"][over]
        out["triangle"][over] = near["triangle"][over]
        out["overlap"][over] = 1
    spheres = [i for i, ob in enumerate(objects) if ob["type"] == OBJ_SPHERE]
    owner = triangle_owners(objects, T)
    assert (owner >= 0).all(), "a triangle of the flattened scene that no object offers"
    sc = np.array([objects[i]["v"][0:3] for i in spheres], np.float32).reshape(-1, 3)
    sr = np.array([objects[i]["v"][3] for i in spheres], np.float32).reshape(-1)
    cand_obj = np.concatenate([np.asarray(spheres, np.int64), owner])
    cand_tri = np.concatenate([np.full(len(spheres), -1, np.int64), np.arange(T, dtype=np.int64)])
    rank = cand_obj * (1 << 22) + (cand_tri + 1)                        # the tie order: object, then triangle
    is_mesh_tri = np.array([objects[i]["type"] == OBJ_MESH for i in owner], bool) if T else np.zeros(0, bool)
    todo = np.nonzero(ok_geo & ~over_geo)[0]
    with np.errstate(all="ignore"):
        for at in range(0, todo.size, CHUNK):
            rows = todo[at:at + CHUNK]
            o, d, r = o_all[rows], d_all[rows], r_all[rows]
            m = rows.size
            oc = tuple(o[:, a][:, None] for a in range(3))
            dc = tuple(d[:, a][:, None] for a in range(3))
            dd = dot(dc[0], dc[1], dc[2], dc[0], dc[1], dc[2])
            rc = r[:, None]
            if spheres:
                ks, ts = sphere_cand(tuple(sc[None, :, a] for a in range(3)), sr[None, :], oc, dc, dd, rc)
                ks, ts = np.broadcast_to(ks, (m, len(spheres))), np.broadcast_to(ts, (m, len(spheres)))
                fs = np.full((m, len(spheres)), -1, np.int32)
            else:
                ks, ts, fs = np.zeros((m, 0), bool), np.zeros((m, 0), np.float32), np.zeros((m, 0), np.int32)
            if T:
                tt, ft = tri_cand(tris[None, :, :], oc, dc, dd, rc)
                pk, B = tree_paths(nodes, meshes, o, F1 / d, r, T)
                kt = np.where(is_mesh_tri[None, :], pk, True)
                Kt = np.where((tt < B) & is_mesh_tri[None, :], B, tt)
            else:
                tt, ft, kt, Kt = np.zeros((m, 0), np.float32), np.zeros((m, 0), np.int32), np.zeros((m, 0), bool), np.zeros((m, 0), np.float32)
            okc = np.concatenate([ks, kt], axis=1)
            K = np.concatenate([ts, Kt], axis=1)
            t = np.concatenate([ts, tt], axis=1)
            f = np.concatenate([fs, ft], axis=1)
            if K.shape[1] == 0:
                continue
            exists = okc & ~np.isnan(K) & (K < np.float32(np.inf))
            for run in runs:
                out, lim = run["out"], run["lim"][rows]
                valid = exists & (K <= lim[:, None]) & run["ok"][rows][:, None]
                best = np.where(valid, K, np.float32(np.inf)).min(axis=1)
                tied = valid & (K == best[:, None])
                win = np.where(tied, rank[None, :], np.int64(1) << 62).argmin(axis=1)
                hit = valid.any(axis=1)
                run["dropped"][rows] = exists.any(axis=1) & ~hit & run["ok"][rows]
                sel = np.nonzero(hit)[0]
                if not sel.size:
                    continue
                w, g = win[sel], rows[sel]
                tw, fw = t[sel, w], f[sel, w]
                run["key"][g] = best[sel]
                og, dg, rg = o[sel], d[sel], r[sel]
                centre = np.stack([dg[:, a] * tw + og[:, a] for a in range(3)], axis=-1)
                pts = np.zeros((sel.size, 3), np.float32)
                is_s = w < len(spheres)
                if is_s.any():
                    _, pts[is_s] = NR.sphere_eval(sc[w[is_s]], sr[w[is_s]], centre[is_s])
                if (~is_s).any():
                    q = ~is_s
                    oq, dq = tuple(og[q, a] for a in range(3)), tuple(dg[q, a] for a in range(3))
                    pts[q] = tri_point(tris[w[q] - len(spheres)], oq, dq, dot(dq[0], dq[1], dq[2], dq[0], dq[1], dq[2]), rg[q], fw[q])
                out["t"][g] = tw
                out["centre"][g] = centre
                out["point"][g] = pts
                out["object"][g] = cand_obj[w]
                out["triangle"][g] = cand_tri[w]
                out["feature"][g] = fw
    return [(run["out"], {"key": run["key"], "dropped": run["dropped"], "valid": run["ok"]}) for run in runs]


# ---- what happened to each query: the coverage conditions of the tests ---------------------------------------------------------------
KINDS = ("face", "edge1", "edge2", "edge3", "vertex1", "vertex2", "vertex3", "sphere_outside", "sphere_inside", "overlap", "miss", "dropped")


def kinds(flat, rec, origins, detail):
    """per kind of outcome the share of the queries that had it"""
    _, _, _, objects = sections(flat)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    n = max(1, rec.shape[0])
    share = {}
    tri = (rec["overlap"] == 0) & (rec["triangle"] >= 0)
    for k, name in enumerate(KINDS[:7]):
        share[name] = float((tri & (rec["feature"] == k)).sum()) / n
    sph = np.nonzero((rec["overlap"] == 0) & (rec["object"] >= 0) & (rec["triangle"] < 0))[0]
    inside = np.zeros(rec.shape[0], bool)
    for i in sph:
        v = objects[rec["object"][i]]["v"]
        m = o[i] - v[0:3].astype(np.float32)
        inside[i] = not (dot(m[0], m[1], m[2], m[0], m[1], m[2]) > v[3] * v[3])
    share["sphere_inside"] = float(inside.sum()) / n
    share["sphere_outside"] = float(sph.size - inside.sum()) / n
    share["overlap"] = float((rec["overlap"] == 1).sum()) / n
    share["miss"] = float(((rec["object"] < 0) & detail["valid"] & ~detail["dropped"]).sum()) / n
    share["dropped"] = float(detail["dropped"].sum()) / n
    return share


def mesh_winner_share(flat, rec):
    _, _, _, objects = sections(flat)
    is_mesh = np.array([ob["type"] == OBJ_MESH for ob in objects], bool)
    hit = rec["object"] >= 0
    return float(is_mesh[rec["object"][hit]].sum()) / max(1, rec.shape[0])


# ---- binary64, from outside the formulas: the first time at which the scene's distance from the centre is r --------------------------------
def geometry64(objs, flat):
    """(spheres [S, 4], triangles [T, 9] as p0, s1, s2) in binary64.  From the object list itself where it gives the numbers - spheres
    (centre, radius) and meshes as vertex arrays, the differences formed in binary64 - else (files, quads, cuboids: what the library's loader
    and builders make of them) from the flattened records"""
    if objs is not None and all(ob[0] in ("sphere", "mesh") for ob in objs):
        sph = np.array([list(ob[1]) + [ob[2]] for ob in objs if ob[0] == "sphere"], np.float64).reshape(-1, 4)
        parts = [np.asarray(ob[1], np.float64).reshape(-1, 3, 3) for ob in objs if ob[0] == "mesh"]
        v = np.concatenate(parts) if parts else np.zeros((0, 3, 3))
        return sph, np.concatenate([v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]], axis=1)
    _, _, tris, objects = sections(flat)
    sph = np.array([ob["v"][0:4] for ob in objects if ob["type"] == OBJ_SPHERE], np.float64).reshape(-1, 4)
    return sph, tris[:, 0:9].astype(np.float64)


def distance64(sph, tri, p):
    """the distance from the points p [n, 3] to the surfaces: spheres |len(p - c) - R|, triangles by Ericson's point-triangle region test -
    nearest_ref's, which knows nothing of moving balls - all in binary64"""
    D = np.full(p.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for c in sph:
            D = np.minimum(D, np.abs(np.sqrt(((p - c[0:3]) ** 2).sum(axis=1)) - c[3]))
        for at in range(0, tri.shape[0], 2048):
            t = np.concatenate([tri[at:at + 2048], np.zeros((min(2048, tri.shape[0] - at), 3))], axis=1)
            d2, _ = NR.tri_eval(t[None, :, :], p[:, None, :])
            D = np.minimum(D, np.sqrt(np.where(np.isnan(d2), np.inf, d2).min(axis=1)))
    return D


def sweep64(flat, origins, directions, radius, tmax=None, objs=None, steps=400, tol=1e-10):
    """(t [n], M [n], settled [n]) by conservative advancement in binary64: from t = 0 the centre moves by (distance - r) / |d| until the distance
    is within tol * M of r.  No formula of the sweep is used: the time found is the first at which the binary64 distance field reaches r, +Inf
    once the ball is past its limit or out of the scene's reach, NaN for an invalid input or a ball that starts within r.  `settled` is False
    where `steps` did not suffice (a ball that grazes creeps)."""
    sph, tri = geometry64(objs, flat)
    o32, d32, r32, tm32, n = _inputs(origins, directions, radius, tmax)
    ok, lim = valid_inputs(o32, d32, r32, tm32)
    o, d, r = o32.astype(np.float64), d32.astype(np.float64), r32.astype(np.float64)
    lo, hi = scene_bounds(flat)
    big = float(max(np.abs(lo).max(), np.abs(hi).max()))
    M = np.maximum(np.abs(o).max(axis=1), big)
    speed = np.sqrt((d * d).sum(axis=1))
    reach = (np.sqrt(((o - (lo + hi) / 2.0) ** 2).sum(axis=1)) + np.linalg.norm(hi - lo) + r) / np.where(speed > 0, speed, 1.0)
    stop = np.minimum(lim.astype(np.float64), reach)
    t = np.zeros(n)
    out = np.full(n, np.nan)
    settled = np.ones(n, bool)
    live = np.nonzero(ok)[0]
    D0 = distance64(sph, tri, o[live])
    live = live[D0 > r[live]]                                                # (a ball that starts within r: an overlap, NaN)
    for _ in range(steps):
        if not live.size:
            break
        gap = distance64(sph, tri, o[live] + d[live] * t[live, None]) - r[live]
        hit = gap <= tol * M[live]
        out[live[hit]] = t[live[hit]]
        live, gap = live[~hit], gap[~hit]
        t[live] += gap / speed[live]
        gone = t[live] > stop[live]
        out[live[gone]] = np.inf
        live = live[~gone]
    settled[live] = False
    return out, M, settled


# ---- the balls of the tests ------------------------------------------------------------------------------------------------------------
def query_sweeps(flat, seed, n):
    """seeded balls for a scene -> (origins, directions, radius).  Origins uniform in twice the scene's bounds (around its triangles where it
    has some); a third aimed from outside at sampled vertices, a third at points on sampled edges, the rest at triangle interiors, at
    sphere centres and at random; some origins inside scene spheres, some within r of the surface; radii 0, a small fraction of the mean
    edge length, about an edge length, and larger than the whole mesh; the direction is taken as given: a third are not of unit length"""
    rng = np.random.default_rng(seed)
    _, _, tris, objects = sections(flat)
    lo, hi = scene_bounds(flat)
    sph = np.array([ob["v"][0:4] for ob in objects if ob["type"] == OBJ_SPHERE], np.float32).reshape(-1, 4)
    edge_len = np.float32(1)
    if tris.shape[0]:
        corners = np.concatenate([tris[:, 0:3], tris[:, 0:3] + tris[:, 3:6], tris[:, 0:3] + tris[:, 6:9]])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        edge_len = np.float32(np.mean([np.linalg.norm(tris[:, 3:6], axis=1).mean(), np.linalg.norm(tris[:, 6:9], axis=1).mean()]))
    elif sph.shape[0]:
        edge_len = np.float32(np.median(sph[:, 3]))
    mid, half = (lo + hi) / np.float32(2), (hi - lo)
    diag = np.float32(np.linalg.norm(hi - lo))
    org = rng.uniform(mid - half, mid + half, (n, 3)).astype(np.float32)
    target = rng.uniform(mid - half / 2, mid + half / 2, (n, 3)).astype(np.float32)
    kind = rng.integers(0, 12, n)
    if tris.shape[0]:
        which_tri = rng.integers(0, tris.shape[0], n)
        mesh_tris = np.nonzero(np.array([objects[i]["type"] == OBJ_MESH for i in triangle_owners(objects, tris.shape[0])], bool))[0]
        if mesh_tris.size:                                                     # half of the aimed balls at a mesh, however many other triangles there are
            which_tri = np.where(rng.integers(0, 2, n) == 0, mesh_tris[rng.integers(0, mesh_tris.size, n)], which_tri)
        pick = tris[which_tri]
        a, s1, s2 = pick[:, 0:3], pick[:, 3:6], pick[:, 6:9]
        which = rng.integers(0, 3, n)[:, None]
        vert = np.where(which == 0, a, np.where(which == 1, a + s1, a + s2))
        u = rng.uniform(0.05, 0.95, (n, 1)).astype(np.float32)
        on_edge = np.where(which == 0, a + s1 * u, np.where(which == 1, a + s2 * u, (a + s1) + (s2 - s1) * u))
        bu, bv = rng.uniform(0.1, 0.45, (n, 1)).astype(np.float32), rng.uniform(0.1, 0.45, (n, 1)).astype(np.float32)
        inner = a + s1 * bu + s2 * bv
        target = np.where((kind < 4)[:, None], vert, np.where((kind < 8)[:, None], on_edge, np.where((kind < 10)[:, None], inner, target)))
        # aimed from outside: along the triangle's normal, tilted
        nrm = np.cross(s1, s2)
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)
        side = np.where(rng.integers(0, 2, (n, 1)) == 0, -1.0, 1.0)
        tilt = rng.normal(0, 0.6, (n, 3))
        away = nrm * side + tilt
        away /= np.maximum(np.linalg.norm(away, axis=1, keepdims=True), 1e-20)
        aimed = kind < 10
        # from far outside, or - every other ball - from nearby, so that a mesh inside a room of quads is reached before the walls are
        start = np.where(rng.integers(0, 2, (n, 1)) == 0, rng.uniform(0.6, 1.6, (n, 1)), rng.uniform(0.03, 0.25, (n, 1)))
        org[aimed] = (target + away * start * diag)[aimed].astype(np.float32)
    if sph.shape[0]:
        s = sph[rng.integers(0, sph.shape[0], n)]
        at_sphere = kind == 10
        target[at_sphere] = s[at_sphere, 0:3]
        inside = rng.integers(0, 16, n) == 0                                   # origins inside a scene sphere
        org[inside] = (s[:, 0:3] + rng.uniform(-0.5, 0.5, (n, 3)) * s[:, 3:4])[inside].astype(np.float32)
    d = (target - org).astype(np.float64)
    d[np.linalg.norm(d, axis=1) < 1e-9] = (0.0, 0.0, 1.0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    scale = np.where(rng.integers(0, 3, (n, 1)) == 0, rng.uniform(0.3, 2.5, (n, 1)), 1.0)
    dirs = (d * scale).astype(np.float32)
    rk = rng.integers(0, 16, n)
    radius = np.where(rk < 3, 0.0, np.where(rk < 8, rng.uniform(0.01, 0.1, n) * edge_len, np.where(rk < 14, rng.uniform(0.5, 1.5, n) * edge_len, rng.uniform(1.0, 1.5, n) * diag)))
    radius = radius.astype(np.float32)
    # a ball of radius 0 aimed exactly at a vertex or an edge asks a question whose answer is discontinuous in its input (rounding the direction
    # decides whether the feature or what lies behind it is met): those balls get a small radius, radius 0 goes to the others
    if tris.shape[0]:
        sharp = (kind < 8) & (radius == 0)
        radius[sharp] = (rng.uniform(0.01, 0.1, n) * edge_len).astype(np.float32)[sharp]
    # within r of the surface: the start of some balls moved next to their target
    close = (rng.integers(0, 12, n) == 0) & (radius > 0)
    org[close] = (target - d * (radius[:, None] * rng.uniform(0.2, 0.9, (n, 1))))[close].astype(np.float32)
    return np.ascontiguousarray(org), np.ascontiguousarray(dirs), np.ascontiguousarray(radius)
