"""The ray and point kernels past one chunk per wave: closest hit, any hit, multi-hit, nearest surface, winding number and the first-hit
planes' tile front, each on a batch of TWICE as many 64-item chunks as the device can hold resident waves, every output record compared as
bytes with the family's own yardstick.

Why: the launchers size the grid as one wave per 64 items up to the resident grid, and the largest batch any other file sends is a few
thousand items.  There every wave takes one chunk, all 64 lanes start together and each answers one item.  What the kernels were written
for - a lane answering item after item on the same registers, stack column and buffer; lanes freeing up at different times; one FETCH
handing out the tail of one chunk and the head of the next; the refill yield firing until the counter is exhausted; the second trip of
rt_multihit_uv_kernel's grid-stride loop - runs here and nowhere else in the suite.

How large: n = 2 * 64 * cus * waves_cap + 37 (`batch_size`), cus and waves_cap (resident waves per CU) read from the device's properties,
never written down: whatever occupancy a shape gets, at least half of all chunks go to a wave that has answered one already.  37: the last
chunk is ragged.

The yardstick at that size: an item's answer does not depend on its place in the batch, so the big batch is a seeded draw, with
repetition, from the family's base batch (a few thousand items), and the expectation is the same draw from the yardstick's answers on the
base batch - the CPU oracle's trace_one / trace_one_uv, tests/multihit_ref.py, tests/nearest_ref.py, tests/winding_ref.py, computed once per
scene as in the families' own files.  The draw mixes two classes of the base batch, told apart BY THE YARDSTICK ALONE, so that the lanes of
a wave finish at different times: each slot is, with probability 1/4, a cheap item (one answered without a walk: a ray the yardstick says
meets nothing - which a NaN direction and a limit that is 0, negative or NaN bring about too -, a point that is not finite or whose limit
is 0 or negative) and otherwise, uniformly, a walker (an item with a mesh triangle in its answer; for the occlusion byte: a ray whose
closest hit lies on a mesh and whose limit is positive; for the winding number, a sum over every mesh triangle: a finite point).  Both
classes must be non-empty and the drawn shares within 0.02 of 1/4 and 3/4.  Items of the base batch in neither class are not drawn.

Scenes and placements: those of tests/test_gpu_random_scenes.py, committed through its Case.commit (the placement asserted from
scene.info()): seed 13 (five meshes) on its own shape, forced to 1024 threads, from global memory behind FILLER, and the hybrid soup -
scene modes 1, 0, 2 and two workgroup sizes.  The winding number has no placement: seed 14 (two meshes) and monkey.

The big batches go through the device forms, are filled with a pattern first (an id that is never answered shows) and copied back once;
the host form runs at full size once per family (its staging buffers grow to this size).

Two identities between device paths, named where they are made: (1) the view case holds the depth, normal and object planes of a ragged
view of more than 2 * cus * waves_cap tiles to rt_trace_rays on the view's own ray plane - a plain yardstick for the planes is per-pixel
Python; rt_trace_rays at this size is held to the oracle by the cases above, and the ray plane itself to the NumPy expression
(test_gpu_query.primaries); (2) the u, v of a sphere record that is not its ray's closest hit, which neither yardstick restates, are those
of the base batch's own run.  Out of scope, knowingly: the visibility and ambient-occlusion planes at this size (their yardsticks are
per-pixel Python, and nothing replicates a view exactly).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import multihit_ref as MR
import multihit_scenes as MS
import nearest_ref as NR
import test_gpu_multihit as M
import test_gpu_nearest as N
import test_gpu_winding as WT
import winding_ref as WR
from random_scenes import MESH_KINDS
from test_gpu_occlusion import expected as occlusion_expected, limit_sets
from test_gpu_query import assert_equal_to_oracle, assert_triangles_and_uv, primaries, u32
from test_gpu_random_scenes import Case, oracle_of, ray_records, ref, uv_records

pytestmark = pytest.mark.gpu

F = np.float32
PATTERN = 0xA5                      # what every output buffer holds before a launch
P_CHEAP, SHARE_TOL = 0.25, 0.02
K = 3                               # the multi-hit k: a tenth of seed 13's rays have more candidates (tests/multihit_scenes.py)
N_BASE_LARGE = 2048                 # rays / uniform points of a base batch on a scene of thousands of triangles, as the families' files keep it
PLACEMENTS = [Case("random", 13), Case("random", 13, "threads1024"), Case("random", 13, "global"), Case("soup", 0, "hybrid")]
UV_CASE = Case("random", 15)        # its tenth object is a sphere with a gradient: the one kind of record rt_multihit_uv_kernel writes
WINDING_SCENES = ("random14", "monkey")
# rays that no scene here meets, whatever it holds: directions with a NaN, and rays that start beyond everything and point further away
AWAY_O = np.array([(0, 0, 0), (0.1, 0.2, 2.0), (0, 0, 0), (0.3, -0.1, 1.5), (0, 300, 2), (500, 300, 2), (0, 250, -400), (-300, 400, 900)], F)
AWAY_D = np.array([(np.nan, 0, 1), (0, np.nan, 0), (np.nan, np.nan, np.nan), (0.2, 0.1, np.nan), (0, 1, 0), (1, 1, 0), (0, 0.5, -1), (-1, 2, 1)], F)


# ---- the size and the draw -----------------------------------------------------------------------------------------------------------
def device_waves():
    """(cus, resident waves per CU) of device 0: the library's num_cus is the first"""
    import torch
    props = torch.cuda.get_device_properties(0)
    return int(props.multi_processor_count), int(props.max_threads_per_multi_processor) // 64


def batch_size():
    cus, waves_cap = device_waves()
    n = 2 * 64 * cus * waves_cap + 37
    assert n // 64 >= 2 * cus * waves_cap and n % 64, (n, cus, waves_cap)
    return n


def draw(cheap, walker, n, seed, what):
    """n indices into the base batch: each slot a cheap item with probability 1/4, else a walker, uniformly within its class"""
    c, w = np.flatnonzero(cheap), np.flatnonzero(walker)
    assert c.size and w.size and not (cheap & walker).any(), (what, c.size, w.size)
    rng = np.random.default_rng(seed)
    is_cheap = rng.random(n) < P_CHEAP
    idx = np.where(is_cheap, c[rng.integers(0, c.size, n)], w[rng.integers(0, w.size, n)])
    assert abs(cheap[idx].mean() - P_CHEAP) <= SHARE_TOL and abs(walker[idx].mean() - (1 - P_CHEAP)) <= SHARE_TOL, (what, cheap[idx].mean(), walker[idx].mean())
    return idx


def on_mesh(case, obj):
    """which of the object indices (any shape; -1: none) name a mesh"""
    kinds = np.array([o[0] in MESH_KINDS for o in case.objs] + [False])
    return kinds[np.where(obj >= 0, obj, len(case.objs))]


# ---- the device forms: a filled buffer, one launch, one copy back --------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def filled(shape, dtype=None):
    import torch
    t = torch.full(shape, PATTERN, dtype=torch.uint8, device="cuda:0")
    return t if dtype is None else t.view(dtype)


def trace_device(rt, ctx, scene, o, d):
    import torch
    n = len(o)
    t_o, t_d, out = dev(o), dev(d), filled((n, rt.HIT_DTYPE.itemsize))
    torch.cuda.synchronize()
    rt.trace_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), n, out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy().view(rt.HIT_DTYPE).reshape(n)


def occluded_device(rt, ctx, scene, o, d, tmax):
    import torch
    n = len(o)
    t_o, t_d, out = dev(o), dev(d), filled((n,))
    t_t = dev(tmax) if tmax is not None else None
    torch.cuda.synchronize()
    rt.occluded_rays_device(ctx, scene, t_o.data_ptr(), t_d.data_ptr(), t_t.data_ptr() if tmax is not None else None, n, out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


def multi_device(rt, ctx, scene, o, d, k, tmax):
    import torch
    n = len(o)
    hits = filled((n, k, rt.HIT_DTYPE.itemsize)) if k else None
    counts = filled((n, 4)).view(torch.int32).reshape(n)
    torch.cuda.synchronize()
    rt.trace_rays_multi_device(ctx, scene, dev(o), dev(d), k, dev(tmax) if tmax is not None else None, hits=hits, counts=counts)
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(rt.HIT_DTYPE)[..., 0] if k else np.zeros((n, 0), rt.HIT_DTYPE)
    return got, counts.cpu().numpy()


def nearest_device(rt, ctx, scene, pts, lim):
    import torch
    out = filled((len(pts), rt.NearestRecord.itemsize))
    torch.cuda.synchronize()
    rt.nearest_points_device(ctx, scene, dev(pts), dev(lim) if lim is not None else None, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(rt.NearestRecord).reshape(-1)


# ---- the base batches and the yardsticks' answers, once per scene ---------------------------------------------------------------------
def ray_base(orc, models_dir, case):
    """tests/test_gpu_random_scenes.py's rays of the scene (2,000 scattered ones and a 40 x 30 primary grid) followed by AWAY_O / AWAY_D,
    with the oracle's closest hit of each from trace_one and from trace_one_uv"""
    def make():
        q = ray_records(orc, models_dir, case)
        oracle = oracle_of(orc, models_dir, case)
        hit_uv, rec = uv_records(oracle, AWAY_O, AWAY_D)
        hit, out = np.zeros(len(AWAY_O), bool), np.zeros((len(AWAY_O), 8), F)
        for i in range(len(AWAY_O)):
            hit[i], out[i] = oracle.trace_one(AWAY_O[i], AWAY_D[i])
        b = dict(o=np.concatenate([q["o"], AWAY_O]), d=np.concatenate([q["d"], AWAY_D]), hit=np.concatenate([q["hit"], hit]), out=np.concatenate([q["out"], out]),
                 hit_uv=np.concatenate([q["hit_uv"], hit_uv]), rec=np.concatenate([q["rec"], rec]))
        assert np.array_equal(b["hit_uv"], b["hit"]) and np.array_equal(u32(b["rec"][:, :8]), u32(b["out"]))       # the oracle's two queries agree
        return b
    return ref(case, "refill rays", make)


def multihit_base(rt, models_dir, case):
    """dict(flat, o, d, cand, lim, cand_lim): tests/test_gpu_multihit.py's own reference where it has the scene, else one made the same way
    (multihit_ref.query_rays, 2,048 rays); the limits are that file's limits_for"""
    def make():
        name = "random%d" % case.seed
        if case.name == name and name in MS.SCENES:
            b = M.reference(rt, models_dir, name)
        else:
            flat = rt.SceneObjects(case.objs, models_dir).debug_flatten()
            o, d = MR.query_rays(flat, 100 + case.seed, N_BASE_LARGE)
            b = {"flat": flat, "o": o, "d": d, "cand": MR.candidates(flat, o, d)}
        if "lim" not in b:                                       # (as test_gpu_multihit.want makes them)
            b["lim"] = M.limits_for(b["cand"])
            b["cand_lim"] = MR.candidates(b["flat"], b["o"], b["d"], b["lim"])
        return b
    return ref(case, "refill multihit", make)


def multihit_want(rt, models_dir, case, k, limited):
    """(hits, counts, sphere_uv) of the yardstick on the base batch"""
    b = multihit_base(rt, models_dir, case)
    return ref(case, ("refill multihit records", k, limited), lambda: MR.records(b["flat"], b["o"], b["d"], k, b["cand_lim"] if limited else b["cand"]))


def nearest_base(rt, models_dir, case):
    """(points, records without a limit, limits, records under them): tests/test_gpu_nearest.py's own reference where it has the scene, else
    one made the same way"""
    def make():
        name = "random%d" % case.seed
        if case.name == name:
            return N.reference(rt, models_dir, name)
        flat = rt.SceneObjects(case.objs, models_dir).debug_flatten()
        pts = np.concatenate([NR.query_points(flat, 100 + case.seed, 1700), WT.BAD])
        assert pts.shape[0] <= N_BASE_LARGE
        free = NR.nearest(flat, pts)
        lim = N.limits_for(free["distance"])
        return pts, free, lim, NR.nearest(flat, pts, lim)
    return ref(case, "refill nearest", make)


# ---- the families: check_<family>(rt, orc, ctx, models_dir, case, scene, n, host) ------------------------------------------------------
def check_trace_rays(rt, orc, ctx, models_dir, case, scene, n, host):
    """rt_trace_rays_device: the record against trace_one (assert_equal_to_oracle), u and v against trace_one_uv on every hit, and the
    triangle index against the base batch's - which assert_triangles_and_uv holds to the flattened layout on every hit that is no sphere's"""
    b = ray_base(orc, models_dir, case)
    hit, mesh = b["hit"], b["hit"] & on_mesh(case, np.where(b["hit"], b["out"][:, 7], -1).astype(np.int32))
    idx = draw(~hit, mesh, n, 1300 + case.seed, case.id)

    def triangles():
        small = rt.trace_rays(ctx, scene, b["o"], b["d"])
        assert_equal_to_oracle(small, hit, b["out"], case.id + ", the base batch")
        assert assert_triangles_and_uv(rt, case.objs, models_dir, b["o"], b["d"], small, case.id, sample=len(hit)) > 0
        return small["triangle"].copy()
    tri = ref(case, "refill triangles", triangles)
    o, d = b["o"][idx], b["d"][idx]
    hits = trace_device(rt, ctx, scene, o, d)
    h = hit[idx]
    assert_equal_to_oracle(hits, h, b["out"][idx], case.id)
    rec = b["rec"][idx]
    bad = (u32(hits["u"][h]) != u32(rec[h, 8])) | (u32(hits["v"][h]) != u32(rec[h, 9]))
    assert not bad.any(), (case.id, "u, v", int(bad.sum()), np.flatnonzero(h)[bad][:5].tolist())
    bad = hits["triangle"] != tri[idx]
    assert not bad.any() and not hits["reserved"].any(), (case.id, "triangle", int(bad.sum()), np.flatnonzero(bad)[:5].tolist())
    if host:
        assert rt.trace_rays(ctx, scene, o, d).tobytes() == hits.tobytes(), (case.id, "the host form")


def occlusion_limits(hit, t):
    """per ray, in turn, one of tests/test_gpu_occlusion.py's limit sets: t, the floats below and above it, t / 2, MISS_T, +inf, NaN, 0, negative"""
    sets = limit_sets(hit, t)
    rows = np.stack([sets[k] for k in sets])
    at = np.arange(len(hit))
    return np.ascontiguousarray(rows[at % len(rows), at])


def check_occluded_rays(rt, orc, ctx, models_dir, case, scene, n, host):
    """rt_occluded_rays_device without limits and with occlusion_limits: expected = `hit and t <= tmax` from the oracle's closest hit"""
    b = ray_base(orc, models_dir, case)
    hit, t = b["hit"], b["out"][:, 0].copy()
    mesh = hit & on_mesh(case, np.where(hit, b["out"][:, 7], -1).astype(np.int32))
    idx = draw(~hit, mesh, n, 1400 + case.seed, case.id)
    o, d = b["o"][idx], b["d"][idx]
    got = occluded_device(rt, ctx, scene, o, d, None)
    want = hit.astype(np.uint8)[idx]
    assert got.tobytes() == want.tobytes(), (case.id, "no limits", int((got != want).sum()), np.flatnonzero(got != want)[:5].tolist())
    if host:
        assert rt.occluded_rays(ctx, scene, o, d).tobytes() == want.tobytes(), (case.id, "the host form")
    lim = occlusion_limits(hit, t)
    with np.errstate(invalid="ignore"):
        positive = lim > 0
    idx = draw(~hit | ~positive, mesh & positive, n, 1500 + case.seed, case.id + ", limits")
    want = occlusion_expected(hit, t, lim)[idx]
    assert 0.1 < want.mean() < 0.9                                     # the limits decide: below t, t / 2 free a walker, the others do not
    got = occluded_device(rt, ctx, scene, b["o"][idx], b["d"][idx], lim[idx])
    assert got.tobytes() == want.tobytes(), (case.id, "limits", int((got != want).sum()), np.flatnonzero(got != want)[:5].tolist())


def multihit_draw(rt, models_dir, case, n, limited, seed):
    """the draw of a multi-hit batch: cheap = no candidate counts, walker = a mesh triangle among the first K records"""
    b = multihit_base(rt, models_dir, case)
    w_hits = multihit_want(rt, models_dir, case, K, limited)[0]
    total = (b["cand_lim"] if limited else b["cand"]).total
    return draw(total == 0, on_mesh(case, w_hits["object"]).any(axis=1), n, seed + case.seed, "%s, limits %s" % (case.id, limited))


def check_trace_rays_multi(rt, orc, ctx, models_dir, case, scene, n, host):
    """rt_trace_rays_multi_device, k = 3, without limits and with limits_for's: test_gpu_multihit.same on every record and count"""
    b = multihit_base(rt, models_dir, case)
    for limited in (False, True):
        idx = multihit_draw(rt, models_dir, case, n, limited, 1600 + limited)
        w = multihit_want(rt, models_dir, case, K, limited)
        o, d, lim = b["o"][idx], b["d"][idx], b["lim"][idx] if limited else None
        got = multi_device(rt, ctx, scene, o, d, K, lim)
        M.same(got, (w[0][idx], w[1][idx], w[2][idx]), "%s, k=%d, limits %s" % (case.id, K, limited))
        if host and not limited:
            again = rt.trace_rays_multi(ctx, scene, o, d, K)
            assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes(), (case.id, "the host form")


def check_count_hits(rt, orc, ctx, models_dir, case, scene, n, host):
    """count-only (k = 0) through the device form, without and with limits, and count_hits: all the candidates that count, as bytes"""
    b = multihit_base(rt, models_dir, case)
    for limited in (False, True):
        idx = multihit_draw(rt, models_dir, case, n, limited, 1700 + limited)
        w = multihit_want(rt, models_dir, case, 0, limited)
        o, d, lim = b["o"][idx], b["d"][idx], b["lim"][idx] if limited else None
        M.same(multi_device(rt, ctx, scene, o, d, 0, lim), (w[0][idx], w[1][idx], w[2][idx]), "%s, k=0, limits %s" % (case.id, limited))
        if host and limited:
            got = rt.count_hits(ctx, scene, o, d, lim)
            assert got.tobytes() == b["cand_lim"].total[idx].tobytes(), (case.id, "count_hits", int((got != b["cand_lim"].total[idx]).sum()))


def check_nearest_points(rt, orc, ctx, models_dir, case, scene, n, host):
    """rt_nearest_points_device without limits and with limits_for's: test_gpu_nearest.same on every record"""
    pts, free, lim, limited = nearest_base(rt, models_dir, case)
    finite = np.isfinite(pts).all(axis=1)
    idx = draw(~finite, on_mesh(case, free["object"]) & (free["triangle"] >= 0), n, 1800 + case.seed, case.id)
    got = nearest_device(rt, ctx, scene, pts[idx], None)
    N.same(got, free[idx], case.id + ", no limits")
    if host:
        N.same(rt.nearest_points(ctx, scene, pts[idx]), free[idx], case.id + ", the host form")
    cheap = ~finite | (lim <= 0)                                       # (a point ON a surface is answered under the limit 0: cheap by its input all the same)
    idx = draw(cheap, on_mesh(case, limited["object"]) & (limited["triangle"] >= 0) & ~cheap, n, 1900 + case.seed, case.id + ", limits")
    N.same(nearest_device(rt, ctx, scene, pts[idx], lim[idx]), limited[idx], case.id + ", limits")


FAMILIES = {"trace_rays": check_trace_rays, "occluded_rays": check_occluded_rays, "trace_rays_multi": check_trace_rays_multi, "count_hits": check_count_hits,
            "nearest_points": check_nearest_points}
CASES = [(f, c) for c in PLACEMENTS for f in FAMILIES]


@pytest.mark.parametrize("family,case", CASES, ids=["%s-%s" % (f, c.id) for f, c in CASES])
def test_family_equals_its_yardstick_past_one_chunk_per_wave(rt, orc, ctx, models_dir, monkeypatch, family, case):
    scene = case.commit(rt, ctx, monkeypatch, models_dir)
    FAMILIES[family](rt, orc, ctx, models_dir, case, scene, batch_size(), host=case.placement == "own")


# ---- the u, v pass's second trip ---------------------------------------------------------------------------------------------------------
def test_sphere_texture_coordinates_past_one_trip_of_the_uv_pass(rt, orc, ctx, models_dir, monkeypatch):
    """rt_multihit_uv_kernel's grid is capped at 8 blocks of 256 threads per CU: with n * K records it goes round its grid-stride loop
    more than twice.  At least 1 % of the expected records lie on a sphere whose material needs u, v.  test_gpu_multihit.same takes those
    u, v from the device; they are held (a) where the record is its ray's closest hit, to the oracle's trace_one_uv on the base batch -
    tests/test_gpu_multihit.py::test_texture_coordinates_equal_the_oracle's rule - and (b) elsewhere to the base batch's own run, one
    trip of the loop (an identity between two device runs: no yardstick restates a sphere's u, v behind another surface)."""
    case = UV_CASE
    scene = case.commit(rt, ctx, monkeypatch, models_dir)
    n = batch_size()
    cus, _ = device_waves()
    assert n * K >= 2 * 2048 * cus
    b = multihit_base(rt, models_dir, case)
    need = b["flat"]["objects"]["need_uv"] != 0
    assert any(o[0] == "sphere" and need[i] for i, o in enumerate(case.objs)), case.id
    w_hits, w_counts, sphere_uv = multihit_want(rt, models_dir, case, K, False)
    idx = multihit_draw(rt, models_dir, case, n, False, 2000)
    assert sphere_uv[idx].sum() >= 0.01 * w_counts[idx].sum(), (sphere_uv[idx].sum(), w_counts[idx].sum())

    def oracle_uv():
        """per base ray: is record 0 a sphere's that needs u, v AND the oracle's closest hit; the oracle's u, v there"""
        oracle = oracle_of(orc, models_dir, case)
        closest, uv = np.zeros(len(b["o"]), bool), np.zeros((len(b["o"]), 2), F)
        for r in np.flatnonzero(sphere_uv[:, 0]):
            hit, out = oracle.trace_one_uv(b["o"][r], b["d"][r])
            closest[r] = hit and u32(out[0:1])[0] == u32(w_hits["t"][r, 0:1])[0] and int(out[7]) == int(w_hits["object"][r, 0])
            uv[r] = out[8:10]
        return closest, uv
    closest, uv = ref(case, "refill sphere uv", oracle_uv)
    assert closest.sum() >= sphere_uv[:, 0].sum() // 2 > 0 and closest[idx].sum() >= 1000, (closest.sum(), sphere_uv[:, 0].sum())
    small = rt.trace_rays_multi(ctx, scene, b["o"], b["d"], K)
    M.same(small, (w_hits, w_counts, sphere_uv), case.id + ", the base batch")
    hits, counts = multi_device(rt, ctx, scene, b["o"][idx], b["d"][idx], K, None)
    M.same((hits, counts), (w_hits[idx], w_counts[idx], sphere_uv[idx]), "%s, k=%d" % (case.id, K))
    first = closest[idx]
    bad = (u32(hits["u"][first, 0]) != u32(uv[idx][first, 0])) | (u32(hits["v"][first, 0]) != u32(uv[idx][first, 1]))
    assert not bad.any(), (case.id, "u, v against the oracle", int(bad.sum()), np.flatnonzero(first)[bad][:5].tolist())
    su = sphere_uv[idx]
    for f in ("u", "v"):
        bad = u32(hits[f])[su] != u32(small[0][f][idx])[su]
        assert not bad.any(), (case.id, f + " against the base batch's run", int(bad.sum()))


# ---- the winding number and the signed distance ----------------------------------------------------------------------------------------
def winding_draw(pts, n, seed, what):
    finite = np.isfinite(pts).all(axis=1)
    return draw(~finite, finite, n, seed, what)


@pytest.mark.parametrize("name", WINDING_SCENES)
def test_winding_numbers_past_one_chunk_per_wave(rt, ctx, models_dir, name):
    """rt_winding_numbers_device with both outputs against tests/winding_ref.py: floats as uint32, the containment bytes"""
    import torch
    flat, pts, want = WT.reference(rt, models_dir, name)
    assert flat["num_triangles"] > 0
    n = batch_size()
    idx = winding_draw(pts, n, 2100, name)
    scene = ctx.commit(rt.SceneObjects(WT.objects_of(rt, name), models_dir))
    w, flags = filled((n, 4), torch.float32).reshape(n), filled((n,))
    torch.cuda.synchronize()
    rt.winding_numbers_device(ctx, scene, dev(pts[idx]), winding=w, inside=flags)
    torch.cuda.synchronize()
    WT.same(w.cpu().numpy(), want[idx], name + ": winding")
    WT.same(flags.cpu().numpy(), WR.inside(want)[idx], name + ": inside")
    if name == WINDING_SCENES[0]:
        w, flags = rt.winding_numbers(ctx, scene, pts[idx], inside=True)
        WT.same(w, want[idx], name + ": winding, the host form")
        WT.same(flags, WR.inside(want)[idx], name + ": inside, the host form")


@pytest.mark.parametrize("name", WINDING_SCENES)
def test_signed_distance_past_one_chunk_per_wave(rt, ctx, models_dir, name):
    """rt_signed_distance_device without a record buffer of the caller's: the nearest launch and then the winding launch on the context's
    own records, which grow to this size.  sdf against winding_ref.sdf of the two yardsticks; the host form's records against nearest_ref."""
    import torch
    flat, pts, w = WT.reference(rt, models_dir, name)
    if ("nearest", name) not in WT._REFS:
        WT._REFS[("nearest", name)] = NR.nearest(flat, pts)
    free = WT._REFS[("nearest", name)]
    want = WR.sdf(w, free["distance"])
    n = batch_size()
    idx = winding_draw(pts, n, 2200, name)
    scene = ctx.commit(rt.SceneObjects(WT.objects_of(rt, name), models_dir))
    sdf = filled((n, 4), torch.float32).reshape(n)
    torch.cuda.synchronize()
    _, none = rt.signed_distance_device(ctx, scene, dev(pts[idx]), sdf=sdf)
    torch.cuda.synchronize()
    assert none is None
    WT.same(sdf.cpu().numpy(), want[idx], name + ": sdf")
    if name == WINDING_SCENES[0]:
        got, rec = rt.signed_distance(ctx, scene, pts[idx])
        WT.same(got, want[idx], name + ": sdf, the host form")
        WT.same(rec, free[idx], name + ": the records, the host form")


# ---- the view front: more tiles than twice the resident waves ---------------------------------------------------------------------------
def view_size():
    """(W, H) = (8a + 3, 8b + 5): ragged against the 8 x 8 tiles, (a + 1) * (b + 1) >= 2 * cus * waves_cap tiles"""
    cus, waves_cap = device_waves()
    a = int(np.ceil(np.sqrt(2 * cus * waves_cap)))
    W, H = 8 * a + 3, 8 * a + 5
    assert ((W + 7) // 8) * ((H + 7) // 8) >= 2 * cus * waves_cap and W % 8 and H % 8
    return W, H


@pytest.mark.parametrize("case", PLACEMENTS, ids=[c.id for c in PLACEMENTS])
def test_first_hit_planes_of_a_view_of_many_tiles(rt, ctx, models_dir, monkeypatch, case):
    """rt_render_aov's front hands out 8 x 8 tiles, and a slot outside the image stays in FETCH.  The ray plane equals the primary-ray
    expression (NumPy, test_gpu_query.primaries).  Depth, normal and object equal rt_trace_rays on that ray plane, record for record: an
    IDENTITY BETWEEN TWO DEVICE PATHS, not a yardstick - acceptable here because rt_trace_rays at this size is held to the oracle by
    test_family_equals_its_yardstick_past_one_chunk_per_wave on the same scenes and placements."""
    scene = case.commit(rt, ctx, monkeypatch, models_dir)
    W, H = view_size()
    cam = rt.Camera(W, H)
    aov = rt.render_aov(ctx, scene, cam, (0.25, 0.5, 0.75), planes=("depth", "normal", "object", "ray"))
    assert np.array_equal(u32(aov["ray"]), u32(primaries(cam.floats(), W, H))), case.id
    d = aov["ray"].reshape(-1, 3)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(cam.floats()[0:3], F), d.shape))
    hits = trace_device(rt, ctx, scene, o, d)
    assert (hits["object"] >= 0).any() and (hits["object"] < 0).any(), case.id
    assert np.array_equal(u32(hits["t"]), u32(aov["depth"].reshape(-1))), case.id
    assert np.array_equal(hits["object"], aov["object"].reshape(-1)), case.id
    assert np.array_equal(u32(hits["normal"]), u32(aov["normal"].reshape(-1, 3))), case.id


def test_every_family_runs_on_every_placement():
    ran = {(f, c.kind, c.seed, c.placement) for f, c in CASES}
    wanted = [("random", 13, "own"), ("random", 13, "threads1024"), ("random", 13, "global"), ("soup", 0, "hybrid")]
    assert all((f, *p) in ran for f in ("trace_rays", "occluded_rays", "trace_rays_multi", "count_hits", "nearest_points") for p in wanted)
    assert [(c.kind, c.seed, c.placement) for c in PLACEMENTS] == wanted and WINDING_SCENES == ("random14", "monkey")
