"""The primary-ray cull (ray-tracer_amd/csrc/rt_cull.h) held to the oracle across views, scene shapes, image sizes, plane lifetimes and every
way a pixel's id reaches memory.  rt_traits_kernel<1024, true, LDS> skips the mesh for the primary rays of every pixel whose bit is set in the
view's cull plane; a pixel flagged wrongly loses the mesh silently, so every frame here is compared as uint32 with the frame rendered without
the plane (RT_AMD_PRIMARY_CULL=0), with the generic kernel's (RT_AMD_KERNEL_VARIANT=generic at commit) and with the CPU oracle's (MATH_DET).
Nothing has a tolerance.  Every scene is committed with RT_AMD_THREADS=1024 and each case first asserts, from scene.info(), 1024 threads, the
scene in LDS and the traits kernel, and from primary_cull_plane(ctx) that the launch was handed a plane where the cull is on.  The inputs
(cameras, scenes, sizes) are built by the functions at the top, which need no GPU: tests/test_primary_cull.py asserts on the CPU that they
still are what the cases below rely on.

Case by case, the fault each would catch:

1. test_a_view (14 random cameras of the monkey and four named views, antialias on and off)
   (a) frames, batch and per-frame with d_prev: a pixel flagged although one of its primary rays hits a triangle (a margin of rt_cull.h too
       small for the device's arithmetic in px_fetch, px_gen, box_enter, box_enter_med3) differs from the frame without the plane and from
       the generic kernel's; the oracle (named views, views 0, 3, 5, 9) catches a fault all three device frames share.
   (b) plane: the pre-pass (rt_cull_kernel.h) computing something else than the host evaluates with the same header - contraction,
       another operation order, a wrong node or mesh offset.
   (c) rim pixels: independent of both kernels.  For every flagged pixel with an unflagged 4-neighbour the oracle traces the pixel's centre
       ray and the eight corners of its jitter cube; the mesh must win none.  A NECESSARY condition, not a proof: nine rays of a continuum,
       and a ray that enters a leaf without hitting a triangle is not seen.  It catches a predicate that is unsound where it matters most,
       at the silhouette, even if a kernel fault hid it from (a).  On the far and the near view every flagged pixel is checked.
   axis-aligned camera: zero direction components (0 * inf in a slab) against node boxes of zero thickness, where a conservative bound on
       an interval product degenerates.  The slab test enters no box of zero thickness, so the oracle sees this grid in no pixel: the weight
       is on (b) and on NaNs; the same camera over a scattered mesh with a third of its vertices in the planes x == 0 and y == 0, which is
       seen, puts the zero components against triangles that are hit.  far camera: the whole mesh inside a pixel or two, the cone wider than
       the root box; near camera: the root box a few centimetres away, where the entry distances are tiny and absolute margins dominate.
2. test_the_meshs_place_in_the_object_list: rt_traits_args.mesh_obj - the sphere loop skipping the wrong object, or the winner's index off
   by the mesh's place, for a mesh in the middle, last, alone, and with an emissive material (which ends the path at the mesh).
3. test_an_image_size: pixel counts that are no multiple of 32 or 64 - the last word's tail bits, a word index past the plane, a row
   stride taken from the tile grid instead of the image; the plane's word count and its clear tail.
4. test_lifetime_*: the plane the context keeps between launches (rt_cull_host::Plan through the C ABI and bind_cull's event order)
   antialias: Key::same without `antialias` reuses the plane computed without jitter for jittered rays (unsound) and the other way round.
   two scenes: Key::same without `scene_uid` reuses scene A's plane for scene B: B's mesh vanishes where A's plane is set.
   transposed size: a key of the word count or pixel count instead of width and height.
   shrink and grow: cap_words bookkeeping - a plane kept after the shrink but read with the old size, or freed under a reader on the grow.
   generic scene in between: used_last and valid left over from the plane user before it.
   streams: a reuse on another stream without the wait for the pre-pass's event reads a plane that is still being written.
   update then launch: a mesh update on one stream and a launch on another: the pre-pass walking the old or half-built BVH.
   pipelined: a camera change rewriting the plane under frames still in flight (the hipEventSynchronize branch of bind_cull).
5. test_every_way_*: a consumer of Px::id that does not mask PX_NOCULL (bit 31) places an unflagged pixel 2^31 ids away - bands, compact
   bands, tile lists, compact output, rt_render_multi_device's ranks and a pipelined frame's plane each compute their address from the id
   in their own way; pixels a launch does not own must keep the buffer's prior value.

Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from test_gpu_descend_pop import context_with, mismatches
from test_gpu_primary_cull import GREY, GROUND, SKY, eq, soup
from test_gpu_query import primaries
from test_gpu_shapes import commit_as

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, LIMIT = 96, 64, 8, 8
TIMES = [7001, 7002, 7003]
GARBAGE = 7.0
JITTER = F(0.001)                     # RT_CULL_JITTER (rt_cull.h), rt_jitter's range
N_SWEEP = 14
ORACLE_VIEWS = (0, 3, 5, 9)           # the random views whose oracle render is compared
NAMED = ["axis-aligned camera", "axis-aligned camera, scattered mesh", "far camera", "near camera"]
VIEW_NAMES = ["view %d" % i for i in range(N_SWEEP)] + NAMED
PLACES = ["first", "middle", "last", "only", "emissive"]
SIZES = [(5, 3), (8, 8), (13, 5), (33, 2), (65, 1), (101, 67)]
WORDS = {(5, 3): 2, (8, 8): 2, (13, 5): 4, (33, 2): 4, (65, 1): 4, (101, 67): 212}     # ((W * H + 63) // 64) * 2, evaluated by hand
ID_SIZES = [(96, 64), (100, 67)]
BAND = dict(band_rows=8, band_first=1, band_stride=3)
LAMP = ("sphere", (-0.5, 0.3, 1.5), 0.25, ("emissive", (1.0, 0.9, 0.8), 4))
MONKEY_BOX = ((-0.2046, -0.3936, 1.2891), (0.4851, 0.1953, 2.0058))                   # the monkey's root box, to four places
NEAR_POS, NEAR_FOCAL = (-0.2346, -0.1, 1.259), 0.05                                   # 3 cm outside the box's -x face and its -z face
FAR_POS = (0.0, 0.0, -400.0)

_CTX, _SCENES, _WANT = {}, {}, {}
TALLY = {"rim pixels": 0, "rays": 0}


# ---------------------------------------------------------------- inputs (no GPU)

def sweep_cameras():
    """(pos, rot, fov) of the 14 random views: np.random.default_rng(2024), per view pos, then rot, then fov"""
    rng = np.random.default_rng(2024)
    out = []
    for _ in range(N_SWEEP):
        pos = rng.uniform([-0.8, -0.5, -0.8], [0.8, 0.5, 0.5])
        rot = rng.uniform(-0.3, 0.3, 3)
        fov = rng.uniform(0.6, 1.6)
        out.append((tuple(float(x) for x in pos), tuple(float(x) for x in rot), float(fov)))
    return out


def flat_grid(nx=12, ny=10, z=-4.0):
    """2 nx ny triangles in the plane z = const over [-1.5, 1.5] x [-1, 1]: the root box and every node box have zero thickness"""
    xs, ys = np.linspace(-1.5, 1.5, nx + 1).astype(F), np.linspace(-1.0, 1.0, ny + 1).astype(F)
    t = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = (xs[i], ys[j], z), (xs[i + 1], ys[j], z), (xs[i + 1], ys[j + 1], z), (xs[i], ys[j + 1], z)
            t += [a + b + c, a + c + d]
    return np.array(t, F)


def scattered_mesh(n=160):
    """zero_direction_scene's mesh (tests/test_gpu_kernel_variants.py): triangles scattered around (0, 0, -4), a third of their vertices moved into
    the plane x == 0 and a third into y == 0"""
    rng = np.random.default_rng(5)
    tris = (rng.normal(0, 0.9, (n, 1, 3)) + rng.normal(0, 0.35, (n, 3, 3))).astype(F)
    tris[..., 2] -= 4.0
    tris[rng.random((n, 3)) < 0.35, 0] = 0.0
    tris[rng.random((n, 3)) < 0.35, 1] = 0.0
    return tris.reshape(n, 9)


def view(rt, name):
    """(objects, sky, the camera's 12 floats) of a view of section 1"""
    if name.startswith("axis-aligned camera"):
        # zero_direction_scene's camera (tests/test_gpu_kernel_variants.py) for 96 x 64: column 48 has direction x == 0, row 32 has y == 0
        ground = ("sphere", (0.0, -102.0, -4.0), 100, ("standard", (0.6, 0.6, 0.6), 1.0))
        mesh = flat_grid() if name == "axis-aligned camera" else scattered_mesh()
        return [("mesh", mesh, ("standard", (0.8, 0.6, 0.4), 0.9)), ground], SKY, np.array([0, 0, 0, -6.0, 4.0, -8.0, 0.125, 0, 0, 0, -0.125, 0], F)
    objs, sky = rt.scenes.monkey()
    if name == "far camera":
        return objs, sky, rt.Camera(W, H, pos=FAR_POS).floats()
    if name == "near camera":
        return objs, sky, rt.Camera(W, H, pos=NEAR_POS, focal_len=NEAR_FOCAL).floats()
    pos, rot, fov = sweep_cameras()[int(name.split()[1])]
    return objs, sky, rt.Camera(W, H, pos=pos, fov=fov, rot=rot).floats()


def scene_key(name):
    return {"axis-aligned camera": "flat grid", "axis-aligned camera, scattered mesh": "scattered mesh"}.get(name, "monkey")


def place(where):
    """the soup of tests/test_gpu_primary_cull.py at five places of the object list.  All five carry all three traits (spheres only, one mesh,
    plain materials - an emissive material is plain: it needs no texture coordinates and does not refract), so each runs rt_traits_kernel"""
    s = soup(3, 300, (0.2, 0.1, 1.4))
    return {"first": [("mesh", s, GREY), LAMP, GROUND], "middle": [LAMP, ("mesh", s, GREY), GROUND], "last": [LAMP, GROUND, ("mesh", s, GREY)],
            "only": [("mesh", s, GREY)], "emissive": [("mesh", s, ("emissive", (1.0, 0.8, 0.6), 3)), GROUND]}[where]


def mesh_index(objs):
    (k,) = [i for i, o in enumerate(objs) if o[0] in ("mesh", "obj")]
    return k


def left_and_right():
    """the two soups of test_a_mesh_update_moves_the_mesh_into_flagged_pixels"""
    return soup(11, 400, (-0.45, 0.0, 1.6)), soup(11, 400, (0.45, 0.0, 1.6))


def two_meshes():
    return [("mesh", soup(3, 300, (0.0, 0.0, 1.4)), GREY), ("mesh", soup(4, 500, (0.05, 0.05, 2.6), 0.3), GREY), GROUND]


def rim_pixels(bits):
    """flagged pixels with an unflagged 4-neighbour, as a boolean (H, W) array"""
    un = bits == 0
    nb = np.zeros_like(un)
    nb[1:, :] |= un[:-1, :]
    nb[:-1, :] |= un[1:, :]
    nb[:, 1:] |= un[:, :-1]
    nb[:, :-1] |= un[:, 1:]
    return (bits == 1) & nb


def cone_directions(P, antialias):
    """normalised(P + off) in binary32 with the kernel's operation order (px_gen, rt_vec.h normalised: v * (1 / sqrt((x*x + y*y) + z*z))), off the
    eight corners of [-J, J]^3 and zero; without antialias the kernel traces P itself"""
    P = np.asarray(P, F)
    if not antialias:
        return P[None, :].copy()
    offs = [(0, 0, 0)] + [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    v = (P[None, :] + (np.array(offs, F) * JITTER).astype(F)).astype(F)
    sq = (v * v).astype(F)
    m = ((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)
    inv = (F(1.0) / np.sqrt(m).astype(F)).astype(F)
    return (v * inv[:, None]).astype(F)


def mesh_winners(oracle, cam12, pixels, antialias, mesh_obj, w=W, h=H):
    """check (c): [(px, py, direction index)] of the rays of `pixels` (a boolean (h, w) array) whose winner the oracle reports as the mesh, and
    the number of rays traced"""
    P = primaries(cam12, w, h)
    origin = np.asarray(cam12[0:3], F)
    bad, rays = [], 0
    for py, px in zip(*np.nonzero(pixels)):
        for k, d in enumerate(cone_directions(P[py, px], antialias)):
            hit, out = oracle.trace_one(origin, d)
            rays += 1
            if hit and int(out[7]) == mesh_obj:
                bad.append((int(px), int(py), k))
    return bad, rays


def band_rows_owned(h):
    return [y for b in range((h + 7) // 8) if b % BAND["band_stride"] == BAND["band_first"] for y in range(b * 8, min(h, b * 8 + 8))]


def random_tile_list(w, h, seed=17):
    """tiles drawn with repeats, the repeats removed, in a random order"""
    rng = np.random.default_rng(seed)
    n = ((w + 7) // 8) * ((h + 7) // 8)
    return rng.permutation(np.unique(rng.integers(0, n, n))).astype(np.uint32)


def tile_mask(w, h, tiles):
    tx = (w + 7) // 8
    m = np.zeros((h, w), bool)
    for t in tiles:
        y, x = int(t) // tx * 8, int(t) % tx * 8
        m[y:y + 8, x:x + 8] = True
    return m


# ---------------------------------------------------------------- the device side

def shared_ctx(rt, monkeypatch, switch):
    """one context with the cull on ("1") and one with it off ("0") for sections 1, 2, 3 and 5: their plane cache then sees every view"""
    if switch not in _CTX:
        _CTX[switch] = context_with(rt, monkeypatch, {"RT_AMD_PRIMARY_CULL": switch})
    return _CTX[switch]


def traits_scene(rt, ctx, monkeypatch, objs, models_dir):
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": "1024"})
    info = scene.info()
    assert info["threads_per_block"] == 1024 and info["scene_in_lds"] == 1 and info["kernel_variant"] == "traits", info
    return scene


def generic_scene(rt, ctx, monkeypatch, objs, models_dir):
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": "1024", "RT_AMD_KERNEL_VARIANT": "generic"})
    info = scene.info()
    assert info["threads_per_block"] == 1024 and info["scene_in_lds"] == 1 and info["kernel_variant"] == "generic", info
    return scene


def three_scenes(rt, monkeypatch, models_dir, key, objs):
    """{"on", "off", "generic"}: (context, scene) - the traits kernel with and without the plane, and the generic kernel (on the context with
    the cull on: it is handed no plane there either)"""
    if key not in _SCENES:
        on, off = shared_ctx(rt, monkeypatch, "1"), shared_ctx(rt, monkeypatch, "0")
        _SCENES[key] = {"on": (on, traits_scene(rt, on, monkeypatch, objs, models_dir)), "off": (off, traits_scene(rt, off, monkeypatch, objs, models_dir)),
                        "generic": (on, generic_scene(rt, on, monkeypatch, objs, models_dir))}
    return _SCENES[key]


def buffer(w, h, value=0.0):
    import torch
    return torch.full((h, w, 3), float(value), dtype=torch.float32, device="cuda:0")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def stream_of(s=None):
    import torch
    return (torch.cuda.current_stream() if s is None else s).cuda_stream


def batch_and_per_frame(rt, ctx, scene, cam, rd, w=W, h=H):
    """the three progressive frames through render_device_batch and through one launch per frame with d_prev; whether both were handed a plane"""
    batch = buffer(w, h)
    rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, batch.data_ptr())
    used_batch = rt.primary_cull_plane(ctx)[0]
    a, b = buffer(w, h), buffer(w, h)
    for i, t in enumerate(TIMES):
        rt.render_device(ctx, scene, cam, rd, t, i, b.data_ptr(), d_prev=a.data_ptr())
        a, b = b, a
    return {"batch": host(batch), "per frame": host(a)}, (used_batch, rt.primary_cull_plane(ctx)[0])


def device_plane(rt, ctx, scene, cam, antialias):
    """the plane the context's last launch was handed, asserted to be the host's for `cam` on the scene as it is on the device; -> words"""
    used, pw, ph, words = rt.primary_cull_plane(ctx)
    assert used and (pw, ph) == (cam.width, cam.height), (used, pw, ph)
    want, stats = rt.primary_cull_host(scene, cam, antialias)
    assert words.size == want.size == stats["words"] == rt.cull.plane_words(cam.width, cam.height), (words.size, want.size)
    assert np.array_equal(words, want), "%d words of the device's plane differ from the host's" % int((words != want).sum())
    return words


def oracle_frames(orc, models_dir, key, objs, cam12, w, h, sky, antialias=True, times=TIMES):
    """the oracle's progressive frames [after 1, after 2, ...], once per case"""
    if key not in _WANT:
        o = orc.Scene(objs, orc.MATH_DET, models_dir)
        out, prev = [], None
        for i, t in enumerate(times):
            prev = o.render(cam12, w, h, SPP, LIMIT, sky, time_ms=t, frame_num=i, antialias=antialias, prev=prev)
            out.append(prev.copy())
        _WANT[key] = out
    return _WANT[key]


def three_way(rt, orc, monkeypatch, models_dir, key, objs, sky, cam, antialias, what, with_oracle=True):
    """(a): both forms on the traits kernel with the plane, without it and on the generic kernel, equal as uint32, and the oracle's frames;
    -> (context, scene) with the plane, whose last launch was of `cam`"""
    rd = rt.RenderData(SPP, LIMIT, antialias, sky)
    sc = three_scenes(rt, monkeypatch, models_dir, key, objs)
    got = {}
    for kind in ("off", "generic", "on"):                         # "on" last: the context's plane is then this view's
        got[kind], used = batch_and_per_frame(rt, *sc[kind], cam, rd)
        assert used == ((kind == "on"),) * 2, (what, kind, used)
    for form in ("batch", "per frame"):
        for kind in ("off", "generic"):
            assert eq(got["on"][form], got[kind][form]), (what, form, "plane on against " + kind, mismatches(got["on"][form], got[kind][form]))
    if with_oracle:
        want = oracle_frames(orc, models_dir, (what, antialias), objs, cam.floats(), W, H, sky, antialias)[-1]
        for form in ("batch", "per frame"):
            assert eq(got["on"][form], want), (what, form, "against the oracle", mismatches(got["on"][form], want))
    return sc["on"]


# ---------------------------------------------------------------- 1. a sweep of views

@pytest.mark.parametrize("antialias", [True, False], ids=["antialias", "no antialias"])
@pytest.mark.parametrize("name", VIEW_NAMES)
def test_a_view(rt, orc, models_dir, monkeypatch, name, antialias):
    """(a) frames, (b) plane, (c) rim pixels (a necessary condition, not a proof: nine rays per pixel of a continuum of them, and only
    triangle hits are seen, not leaves entered) - see the file's docstring"""
    objs, sky, cam12 = view(rt, name)
    cam = rt.Camera(W, H, floats=cam12)
    with_oracle = name in NAMED or int(name.split()[1]) in ORACLE_VIEWS
    ctx, scene = three_way(rt, orc, monkeypatch, models_dir, scene_key(name), objs, sky, cam, antialias, name, with_oracle)
    bits = rt.cull.plane_bits(device_plane(rt, ctx, scene, cam, antialias), W, H)
    pixels = bits == 1 if name in ("far camera", "near camera") else rim_pixels(bits)
    bad, rays = mesh_winners(orc.Scene(objs, orc.MATH_DET, models_dir), cam12, pixels, antialias, mesh_index(objs))
    TALLY["rim pixels"] += int(pixels.sum())
    TALLY["rays"] += rays
    print("%s, antialias %d: %d of %d pixels flagged, check (c) on %d pixels with %d rays; so far %s" % (name, antialias, int(bits.sum()), bits.size, int(pixels.sum()), rays, TALLY))
    assert not bad, (name, antialias, "the oracle has the mesh win rays of flagged pixels (px, py, direction)", bad[:10], len(bad))


# ---------------------------------------------------------------- 2. the mesh's place in the object list

@pytest.mark.parametrize("where", PLACES)
def test_the_meshs_place_in_the_object_list(rt, orc, models_dir, monkeypatch, where):
    """every placement has all three traits (see place()), so every one is asserted to run rt_traits_kernel and to be handed a plane"""
    objs = place(where)
    cam = rt.Camera(W, H)
    ctx, scene = three_way(rt, orc, monkeypatch, models_dir, "soup " + where, objs, SKY, cam, True, "soup " + where)
    bits = rt.cull.plane_bits(device_plane(rt, ctx, scene, cam, True), W, H)
    assert 0.3 < bits.mean() < 0.9, bits.mean()                   # the soup covers about a third of the image: the plane decides something


# ---------------------------------------------------------------- 3. image sizes

@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_an_image_size(rt, orc, models_dir, monkeypatch, w, h):
    objs, sky = rt.scenes.monkey()
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, LIMIT, True, sky)
    sc = three_scenes(rt, monkeypatch, models_dir, "monkey", objs)
    want = oracle_frames(orc, models_dir, ("size", w, h), objs, cam.floats(), w, h, sky)
    got = {}
    for kind in ("off", "on"):
        ctx, scene = sc[kind]
        one, many = buffer(w, h, GARBAGE), buffer(w, h, GARBAGE)
        rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, one.data_ptr())
        used_one = rt.primary_cull_plane(ctx)[0]
        assert ctx.max_batch_frames(w, h) >= len(TIMES)
        rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, many.data_ptr())
        assert (used_one, rt.primary_cull_plane(ctx)[0]) == ((kind == "on"),) * 2
        got[kind] = {"one frame": host(one), "three frames": host(many)}
    for form, ref in (("one frame", want[0]), ("three frames", want[2])):
        assert eq(got["on"][form], got["off"][form]), (w, h, form, "plane on against off", mismatches(got["on"][form], got["off"][form]))
        assert eq(got["on"][form], ref), (w, h, form, "against the oracle", mismatches(got["on"][form], ref))
    words = device_plane(rt, *sc["on"], cam, True)
    assert words.size == WORDS[(w, h)] == rt.cull.plane_words(w, h), (words.size, WORDS[(w, h)])
    tail = np.unpackbits(words.view(np.uint8), bitorder="little")[w * h:]
    assert not tail.any(), "bits past the image are set in the device's plane"


# ---------------------------------------------------------------- 4. plane lifetimes through the C ABI

def fresh_reference(rt, monkeypatch, models_dir, objs, launch):
    """launch(ctx, scene) on a fresh context with the cull off, its scene committed like the sequence's"""
    ctx = context_with(rt, monkeypatch, {"RT_AMD_PRIMARY_CULL": "0"})
    scene = commit_as(rt, ctx, monkeypatch, objs, models_dir, {"RT_AMD_THREADS": "1024"})
    out = launch(ctx, scene)
    assert rt.primary_cull_plane(ctx) == (False, 0, 0, None)
    return out


def batch_frame(rt, cam, antialias, sky, stream=None):
    """a launch: the three progressive frames of `cam` in one render_device_batch, on `stream`; -> the frame's tensor (not waited for)"""
    def launch(ctx, scene):
        out = buffer(cam.width, cam.height, GARBAGE)
        import torch
        torch.cuda.synchronize()                                  # (the fill ran on torch's stream)
        rt.render_device_batch(ctx, scene, cam, rt.RenderData(SPP, LIMIT, antialias, sky), TIMES, 0, out.data_ptr(), stream=None if stream is None else stream.cuda_stream)
        return out
    return launch


def run_sequence(rt, monkeypatch, models_dir, ctx, steps):
    """steps: [(what, objects, scene on ctx, camera, antialias, sky, plane expected)].  After every launch the frame is the fresh cull-off
    context's and the plane read back is the host's for that launch's view"""
    for what, objs, scene, cam, antialias, sky, planned in steps:
        got = host(batch_frame(rt, cam, antialias, sky)(ctx, scene))
        if planned:
            device_plane(rt, ctx, scene, cam, antialias)
        else:
            assert rt.primary_cull_plane(ctx) == (False, 0, 0, None), what
        want = host(fresh_reference(rt, monkeypatch, models_dir, objs, batch_frame(rt, cam, antialias, sky)))
        assert eq(got, want), (what, mismatches(got, want))


def host_bits(rt, objs, cam, antialias=True, models_dir=None):
    return rt.primary_cull_host(rt.SceneObjects(objs, models_dir), cam, antialias)[0]


def sequence_ctx(rt, monkeypatch):
    return context_with(rt, monkeypatch, {"RT_AMD_PRIMARY_CULL": "1"})


def test_lifetime_antialias_off_on_off(rt, models_dir, monkeypatch):
    objs, sky = rt.scenes.monkey()
    cam = rt.Camera(W, H)
    assert not np.array_equal(host_bits(rt, objs, cam, False, models_dir), host_bits(rt, objs, cam, True, models_dir)), "the two planes must differ"
    ctx = sequence_ctx(rt, monkeypatch)
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    run_sequence(rt, monkeypatch, models_dir, ctx, [("antialias %d (step %d)" % (aa, i), objs, scene, cam, aa, sky, True) for i, aa in enumerate((False, True, False))])


def test_lifetime_two_scenes_alternate(rt, models_dir, monkeypatch):
    left, right = left_and_right()
    a, b = [("mesh", left, GREY), GROUND], [("mesh", right, GREY), GROUND]
    cam = rt.Camera(W, H)
    assert not np.array_equal(host_bits(rt, a, cam), host_bits(rt, b, cam)), "the two planes must differ"
    ctx = sequence_ctx(rt, monkeypatch)
    sa, sb = traits_scene(rt, ctx, monkeypatch, a, models_dir), traits_scene(rt, ctx, monkeypatch, b, models_dir)
    run_sequence(rt, monkeypatch, models_dir, ctx, [("scene A", a, sa, cam, True, SKY, True), ("scene B", b, sb, cam, True, SKY, True), ("scene A again", a, sa, cam, True, SKY, True)])


def test_lifetime_transposed_size(rt, models_dir, monkeypatch):
    objs, sky = rt.scenes.monkey()
    wide, tall = rt.Camera(96, 64), rt.Camera(64, 96)
    pw, pt = host_bits(rt, objs, wide, True, models_dir), host_bits(rt, objs, tall, True, models_dir)
    assert pw.size == pt.size and not np.array_equal(pw, pt), "the same word count, two planes"
    ctx = sequence_ctx(rt, monkeypatch)
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    run_sequence(rt, monkeypatch, models_dir, ctx, [("%d x %d (step %d)" % (c.width, c.height, i), objs, scene, c, True, sky, True) for i, c in enumerate((wide, tall, wide))])


def test_lifetime_shrink_and_grow(rt, models_dir, monkeypatch):
    objs, sky = rt.scenes.monkey()
    cams = [rt.Camera(96, 64), rt.Camera(24, 16), rt.Camera(192, 128)]
    sizes = [host_bits(rt, objs, c, True, models_dir).size for c in cams]
    assert sizes[1] < sizes[0] < sizes[2], sizes                  # the allocation is kept on the shrink and grows on the last
    ctx = sequence_ctx(rt, monkeypatch)
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    run_sequence(rt, monkeypatch, models_dir, ctx, [("%d x %d" % (c.width, c.height), objs, scene, c, True, sky, True) for c in cams])


def test_lifetime_a_generic_scene_between_two_plane_users(rt, models_dir, monkeypatch):
    objs, sky = rt.scenes.monkey()
    two = two_meshes()
    cam = rt.Camera(W, H)
    ctx = sequence_ctx(rt, monkeypatch)
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    generic = commit_as(rt, ctx, monkeypatch, two, models_dir, {"RT_AMD_THREADS": "1024"})
    assert generic.info()["kernel_variant"] == "generic" and generic.info()["threads_per_block"] == 1024, generic.info()
    run_sequence(rt, monkeypatch, models_dir, ctx, [("monkey", objs, scene, cam, True, sky, True), ("two meshes", two, generic, cam, True, SKY, False),
                                                    ("monkey again", objs, scene, cam, True, sky, True)])


@pytest.mark.parametrize("waits", [True, False], ids=["plane read after every launch", "launches back to back"])
def test_lifetime_two_streams_share_a_plane(rt, models_dir, monkeypatch, waits):
    """camera a on s1, a on s2 (a reuse on another stream: bind_cull's wait for the pre-pass's event), camera b on s2, b on s1, a on s1.  Reading
    the plane waits for the device, so the second form queues each pair back to back and reads the plane once per pair: only then can a
    missing wait show"""
    import torch
    objs, sky = rt.scenes.monkey()
    cam_a, cam_b = rt.Camera(W, H), rt.Camera(W, H, pos=(0.6, 0.2, 0.3))
    assert not np.array_equal(host_bits(rt, objs, cam_a, True, models_dir), host_bits(rt, objs, cam_b, True, models_dir)), "the two planes must differ"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = sequence_ctx(rt, monkeypatch)
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    want = {id(c): host(fresh_reference(rt, monkeypatch, models_dir, objs, batch_frame(rt, c, True, sky))) for c in (cam_a, cam_b)}
    outs = [buffer(W, H, GARBAGE) for _ in range(5)]
    torch.cuda.synchronize()
    rd = rt.RenderData(SPP, LIMIT, True, sky)
    plan = [(cam_a, s1), (cam_a, s2), (cam_b, s2), (cam_b, s1), (cam_a, s1)]
    for i, (cam, s) in enumerate(plan):
        rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, outs[i].data_ptr(), stream=s.cuda_stream)
        if waits or i in (1, 3, 4):
            device_plane(rt, ctx, scene, cam, True)
    for i, (cam, _) in enumerate(plan):
        got = host(outs[i])
        assert eq(got, want[id(cam)]), (i, mismatches(got, want[id(cam)]))


def test_lifetime_a_mesh_update_then_a_launch_on_another_stream(rt, models_dir, monkeypatch):
    import torch
    left, right = left_and_right()
    a, b = [("mesh", left, GREY), GROUND], [("mesh", right, GREY), GROUND]
    cam = rt.Camera(W, H)
    assert not np.array_equal(host_bits(rt, a, cam), host_bits(rt, b, cam)), "the two planes must differ"
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = sequence_ctx(rt, monkeypatch)
    scene = traits_scene(rt, ctx, monkeypatch, a, models_dir)
    run_sequence(rt, monkeypatch, models_dir, ctx, [("before the update", a, scene, cam, True, SKY, True)])
    moved = torch.from_numpy(right).to("cuda:0")
    out = buffer(W, H, GARBAGE)
    torch.cuda.synchronize()
    scene.update_mesh_device(0, moved, stream=s1.cuda_stream)
    rt.render_device_batch(ctx, scene, cam, rt.RenderData(SPP, LIMIT, True, SKY), TIMES, 0, out.data_ptr(), stream=s2.cuda_stream)
    got = host(out)
    words = device_plane(rt, ctx, scene, cam, True)
    want = host(fresh_reference(rt, monkeypatch, models_dir, b, batch_frame(rt, cam, True, SKY)))
    assert eq(got, want), mismatches(got, want)
    assert not np.array_equal(words, host_bits(rt, a, cam)), "the plane is still the one of the mesh before the update"


def per_frame_reference(rt, cam, rd, times):
    def launch(ctx, scene):
        a, b = buffer(cam.width, cam.height), buffer(cam.width, cam.height)
        for i, t in enumerate(times):
            rt.render_device(ctx, scene, cam, rd, t, i, b.data_ptr(), d_prev=a.data_ptr())
            a, b = b, a
        return a
    return launch


def test_lifetime_pipelined_frames(rt, models_dir, monkeypatch):
    """four frames of camera a in flight, two collected; two frames of camera b submitted while two of a are still in flight - rt_frame_submit
    accepts a changed camera (include/rt_amd.h: the host waits for the frames in flight before it rewrites what they read), which is asserted
    by the calls succeeding; the rest collected; then an ordinary render_device of camera a"""
    import torch
    objs, sky = rt.scenes.monkey()
    cam_a, cam_b = rt.Camera(W, H), rt.Camera(W, H, pos=(0.6, 0.2, 0.3))
    assert not np.array_equal(host_bits(rt, objs, cam_a, True, models_dir), host_bits(rt, objs, cam_b, True, models_dir)), "the two planes must differ"
    rd = rt.RenderData(SPP, LIMIT, True, sky)
    ctx = sequence_ctx(rt, monkeypatch)
    scene = traits_scene(rt, ctx, monkeypatch, objs, models_dir)
    st = stream_of()
    times_a, times_b = [8101, 8102, 8103, 8104], [8201, 8202]
    fr_a, fr_b, last = buffer(W, H, GARBAGE), buffer(W, H, GARBAGE), buffer(W, H, GARBAGE)
    rt.frame_depth(ctx, 4)
    for t in times_a:
        rt.frame_submit(ctx, scene, cam_a, rd, t)
    assert rt.frames_pending(ctx) == 4
    rt.frame_collect(ctx, 0, fr_a.data_ptr(), stream=st)
    rt.frame_collect(ctx, 1, fr_a.data_ptr(), stream=st)
    for t in times_b:
        rt.frame_submit(ctx, scene, cam_b, rd, t)                 # two frames of a are in flight
    assert rt.frames_pending(ctx) == 4
    rt.frame_collect(ctx, 2, fr_a.data_ptr(), stream=st)
    rt.frame_collect(ctx, 3, fr_a.data_ptr(), stream=st)
    device_plane(rt, ctx, scene, cam_b, True)
    rt.frame_collect(ctx, 0, fr_b.data_ptr(), stream=st)
    rt.frame_collect(ctx, 1, fr_b.data_ptr(), stream=st)
    assert rt.frames_pending(ctx) == 0
    rt.frame_wait(ctx)
    rt.render_device(ctx, scene, cam_a, rd, TIMES[0], 0, last.data_ptr(), stream=st)
    device_plane(rt, ctx, scene, cam_a, True)
    for what, got, cam, times in (("camera a", fr_a, cam_a, times_a), ("camera b", fr_b, cam_b, times_b), ("render_device", last, cam_a, TIMES[:1])):
        want = host(fresh_reference(rt, monkeypatch, models_dir, objs, per_frame_reference(rt, cam, rd, times)))
        assert eq(host(got), want), (what, mismatches(host(got), want))


# ---------------------------------------------------------------- 5. every way a pixel's id reaches memory

def id_case(rt, orc, models_dir, monkeypatch, w, h):
    objs, sky = rt.scenes.monkey()
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, LIMIT, True, sky)
    want = oracle_frames(orc, models_dir, ("size", w, h), objs, cam.floats(), w, h, sky)
    return objs, sky, cam, rd, three_scenes(rt, monkeypatch, models_dir, "monkey", objs), want


def on_and_off(rt, sc, cam, launch):
    """launch(ctx, scene) -> a frame (numpy) for the context with the plane and the one without, equal as uint32; -> the one with the plane"""
    got = {}
    for kind in ("off", "on"):
        ctx, scene = sc[kind]
        got[kind] = launch(ctx, scene)
        assert rt.primary_cull_plane(ctx)[0] == (kind == "on"), kind
    device_plane(rt, *sc["on"], cam, True)
    assert eq(got["on"], got["off"]), ("plane on against off", mismatches(got["on"], got["off"]))
    return got["on"]


@pytest.mark.parametrize("compact", [False, True], ids=["in place", "compact"])
@pytest.mark.parametrize("batch", [False, True], ids=["render_device", "render_device_batch"])
@pytest.mark.parametrize("w,h", ID_SIZES, ids=lambda v: str(v))
def test_every_way_bands(rt, orc, models_dir, monkeypatch, w, h, batch, compact):
    objs, sky, cam, rd, sc, want = id_case(rt, orc, models_dir, monkeypatch, w, h)
    rows = band_rows_owned(h)
    assert len(rows) == rt.tile_owned_rows(h, **BAND) and 0 < len(rows) < h

    def launch(ctx, scene):
        out = buffer(w, h, GARBAGE)
        if batch:
            rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, out.data_ptr(), compact=compact, **BAND)
        else:
            rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, out.data_ptr(), compact=compact, **BAND)
        return host(out)
    got = on_and_off(rt, sc, cam, launch)
    ref = want[2] if batch else want[0]
    written = np.zeros(h, bool)
    written[:len(rows)] = True
    if not compact:
        written[:] = False
        written[rows] = True
    assert eq(got[written], ref[rows]), ("owned rows against the oracle", mismatches(got[written], ref[rows]))
    assert np.all(got[~written].view(np.uint32) == F(GARBAGE).view(np.uint32)), "rows the launch does not own were written"


@pytest.mark.parametrize("w,h", ID_SIZES, ids=lambda v: str(v))
def test_every_way_a_shuffled_tile_list(rt, orc, models_dir, monkeypatch, w, h):
    """in place and compact (tile k of the list at floats [192 k, 192 k + 192), rt_tiles_copy_device puts them back), one frame and a batch"""
    objs, sky, cam, rd, sc, want = id_case(rt, orc, models_dir, monkeypatch, w, h)
    tiles = random_tile_list(w, h)
    n_all = ((w + 7) // 8) * ((h + 7) // 8)
    assert 0 < tiles.size < n_all and np.unique(tiles).size == tiles.size and not np.array_equal(tiles, np.sort(tiles))
    mask = tile_mask(w, h, tiles)
    for batch in (False, True):
        for compact in (False, True):
            def launch(ctx, scene):
                out = buffer(w, h, GARBAGE)
                dst = buffer(tiles.size * 64, 1, GARBAGE) if compact else out
                if batch:
                    rt.render_device_batch(ctx, scene, cam, rd, TIMES, 0, dst.data_ptr(), compact=compact, tile_list=tiles)
                else:
                    rt.render_device(ctx, scene, cam, rd, TIMES[0], 0, dst.data_ptr(), compact=compact, tile_list=tiles)
                if compact:
                    rt.tiles_copy_device(ctx, dst.data_ptr(), out.data_ptr(), w, h, tiles, to_frame=True, stream=stream_of())
                return host(out)
            got = on_and_off(rt, sc, cam, launch)
            ref = want[2] if batch else want[0]
            assert eq(got[mask], ref[mask]), (batch, compact, "listed tiles against the oracle", mismatches(got[mask], ref[mask]))
            assert np.all(got[~mask].view(np.uint32) == F(GARBAGE).view(np.uint32)), (batch, compact, "pixels of tiles that are not listed were written")


@pytest.mark.parametrize("w,h", ID_SIZES, ids=lambda v: str(v))
def test_every_way_a_pipelined_frame_with_a_tile_list(rt, orc, models_dir, monkeypatch, w, h):
    objs, sky, cam, rd, sc, want = id_case(rt, orc, models_dir, monkeypatch, w, h)
    tiles = random_tile_list(w, h, seed=18)
    mask = tile_mask(w, h, tiles)

    def launch(ctx, scene):
        out = buffer(w, h, GARBAGE)
        for t in TIMES:
            rt.frame_submit(ctx, scene, cam, rd, t, tile_list=tiles)
        for i in range(len(TIMES)):
            rt.frame_collect(ctx, i, out.data_ptr(), stream=stream_of())
        rt.frame_wait(ctx)
        return host(out)
    got = on_and_off(rt, sc, cam, launch)
    assert eq(got[mask], want[2][mask]), ("listed tiles against the oracle", mismatches(got[mask], want[2][mask]))


@pytest.mark.parametrize("band_rows", [8, 0], ids=["bands of 8 rows", "balanced tile lists"])
@pytest.mark.parametrize("w,h", ID_SIZES, ids=lambda v: str(v))
def test_every_way_render_multi_device(rt, orc, models_dir, monkeypatch, w, h, band_rows):
    """four contexts on device 0 stand in for four GPUs (tests/test_gpu_multi.py); the cull is on in all four or off in all four, and with it
    on every context is asserted to have been handed a plane of its own, equal to the host's"""
    objs, sky = rt.scenes.monkey()
    cam, rd = rt.Camera(w, h), rt.RenderData(SPP, LIMIT, True, sky)
    want = oracle_frames(orc, models_dir, ("size", w, h), objs, cam.floats(), w, h, sky)[2]
    got = {}
    for switch in ("0", "1"):
        ctxs = [context_with(rt, monkeypatch, {"RT_AMD_PRIMARY_CULL": switch}) for _ in range(4)]
        scenes = [traits_scene(rt, c, monkeypatch, objs, models_dir) for c in ctxs]
        frame = buffer(w, h, GARBAGE)
        rt.render_multi_device(ctxs, scenes, cam, rd, TIMES[:1], 0, frame.data_ptr(), band_rows=band_rows, stream=stream_of())
        rt.render_multi_device(ctxs, scenes, cam, rd, TIMES[1:], 1, frame.data_ptr(), band_rows=band_rows, stream=stream_of())
        for c in ctxs:
            c.synchronize()
        got[switch] = host(frame)
        if switch == "1":
            for c, s in zip(ctxs, scenes):
                device_plane(rt, c, s, cam, True)
        else:
            planes = [rt.primary_cull_plane(c) for c in ctxs]
            assert all(p == (False, 0, 0, None) for p in planes), planes
    assert eq(got["1"], got["0"]), ("plane on against off", mismatches(got["1"], got["0"]))
    assert eq(got["1"], want), ("against the oracle", mismatches(got["1"], want))
