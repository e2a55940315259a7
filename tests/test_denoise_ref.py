"""Properties of the denoiser's yardstick alone (tests/denoise_ref.py, the definition of rt_denoise in NumPy float32): fixed points, what
never crosses an edge, what the albedo plane buys, and - from the CPU oracle alone - that the default parameters lower the error of a
4-spp frame against a 1024-spp target on the three config scenes.  CPU tests: the library is not called."""
import numpy as np
import pytest

from denoise_ref import DEFAULTS, H5, denoise_ref

F = np.float32
PARAMETER_SETS = [dict(DEFAULTS), dict(DEFAULTS, iterations=8), dict(DEFAULTS, iterations=1, normal_power_log2=0),
                  dict(DEFAULTS, sigma_colour=0.25, sigma_depth=1.0, normal_power_log2=8), dict(DEFAULTS, iterations=3, sigma_colour=1e6)]


def u32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def guides(H, W, seed=0):
    """a bumpy surface seen head on: unit normals that vary smoothly, depths around 2, three objects in vertical bands"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    n = np.stack([0.3 * np.sin(x / 7.0), 0.3 * np.cos(y / 5.0), -np.ones_like(x)], axis=2).astype(F)
    n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    z = (2.0 + 0.01 * x + 0.02 * y + 0.001 * rng.normal(size=(H, W))).astype(F)
    o = (x * 3 // W).astype(np.int32)
    return n, z, o


def test_spline_constants():
    assert np.array_equal(H5, np.array([1 / 6, 2 / 3, 1, 2 / 3, 1 / 6], F)) and H5[2] == 1.0


@pytest.mark.parametrize("value", [0.5, 1.0])
@pytest.mark.parametrize("params", PARAMETER_SETS)
def test_a_constant_image_is_a_fixed_point(value, params):
    """w * c is exact for c = 0.5 or 1, so acc and wsum stay in exact proportion (not so for every constant: 0.3 comes back one ulp off in places)"""
    H, W = 37, 53
    n, z, o = guides(H, W)
    c = np.full((H, W, 3), value, F)
    for obj in (None, o):
        out = denoise_ref(c, n, z, obj, None, **params)
        assert np.array_equal(u32(out), u32(c))


def test_nothing_crosses_an_object_edge():
    H, W = 24, 40
    n = np.zeros((H, W, 3), F)
    n[..., 2] = -1.0
    z = np.full((H, W), 2.0, F)
    o = np.zeros((H, W), np.int32)
    o[:, W // 2:] = 1
    c = np.zeros((H, W, 3), F)
    c[:, W // 2:] = 1.0
    # a colour tolerance that would let the two sides mix, were it not for the ids
    out = denoise_ref(c, n, z, o, None, iterations=5, sigma_colour=100.0, sigma_depth=1.0, normal_power_log2=0)
    assert np.array_equal(u32(out), u32(c))
    mixed = denoise_ref(c, n, z, None, None, iterations=5, sigma_colour=100.0, sigma_depth=1.0, normal_power_log2=0)
    assert not np.array_equal(u32(mixed), u32(c))


def test_a_tiny_colour_tolerance_changes_nothing():
    H, W = 33, 47
    n, z, o = guides(H, W, 1)
    c = np.random.default_rng(2).random((H, W, 3), dtype=F) + F(0.25)
    # every pair of different pixels is further apart than sigma_colour: k is 0 for all of them, and an equal neighbour adds w * c to
    # acc and w to wsum - which is not bit-exact in general, so make sure there is none
    assert len(np.unique(u32(c).reshape(-1, 3), axis=0)) == H * W
    out = denoise_ref(c, n, z, o, None, iterations=5, sigma_colour=1e-6, sigma_depth=1.0, normal_power_log2=0)
    assert np.array_equal(u32(out), u32(c))


def test_a_miss_and_a_non_finite_pixel_stay_put():
    H, W = 20, 20
    n, z, o = guides(H, W, 3)
    n[5:9, 5:9] = 0.0                                   # misses: normal (0, 0, 0)
    z[5:9, 5:9] = 2.0 ** 30
    o[5:9, 5:9] = -1
    c = np.random.default_rng(4).random((H, W, 3), dtype=F)
    c[12, 12, 1] = np.inf
    c[14, 3, 0] = np.nan
    out = denoise_ref(c, n, z, o, None, **DEFAULTS)
    assert np.array_equal(u32(out[5:9, 5:9]), u32(c[5:9, 5:9]))
    bad = ~np.isfinite(out).all(axis=2)
    assert bad.sum() == 2 and bad[12, 12] and bad[14, 3]      # nothing spreads
    assert np.array_equal(u32(out[12, 12]), u32(c[12, 12])) and np.array_equal(u32(out[14, 3]), u32(c[14, 3]))


def test_albedo_keeps_texture_detail():
    """C = A * L with a checkerboard A and a smooth, noisy L: filtering C / A and multiplying back keeps the checkerboard's edges,
    filtering C directly (with a tolerance wide enough to remove the noise) blurs them"""
    H, W = 48, 64
    n = np.zeros((H, W, 3), F)
    n[..., 2] = -1.0
    z = np.full((H, W), 3.0, F)
    y, x = np.mgrid[0:H, 0:W]
    A = np.where((((x // 4) + (y // 4)) % 2 == 0)[..., None], F(0.9), F(0.3)).astype(F) * np.ones(3, F)
    L = (0.5 + 0.3 * x / W)[..., None].astype(F) * np.ones(3, F)
    noise = (0.1 * np.random.default_rng(5).normal(size=(H, W, 3))).astype(F)
    clean = (A * L).astype(F)
    C = (A * (L + noise)).astype(F)
    p = dict(iterations=4, sigma_colour=2.0, sigma_depth=1.0, normal_power_log2=0, albedo_floor=0.01)
    with_a = denoise_ref(C, n, z, None, A, **p)
    without = denoise_ref(C, n, z, None, None, **p)
    err = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - clean) ** 2)))
    print("rmse against the clean image: noisy %.4f, filtered with albedo %.4f, without %.4f" % (err(C), err(with_a), err(without)))
    assert err(with_a) < err(C) and err(with_a) < 0.5 * err(without)
    # the checkerboard's contrast across an edge survives with the albedo and shrinks without it
    contrast = lambda img: float(np.mean(np.abs(img[:, 3:W - 4:4].astype(np.float64) - img[:, 4:W - 3:4])))
    assert contrast(with_a) > 0.9 * contrast(clean) and contrast(without) < 0.5 * contrast(clean)


def oracle_planes(oracle, cam, W, H):
    """normal, depth, object of the oracle's trace_one on the primary rays (antialiasing off; rt_render_aov's expression)"""
    pos, tl, du, dv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    N = np.zeros((H, W, 3), F)
    Z = np.full((H, W), 2.0 ** 30, F)
    O = np.full((H, W), -1, np.int32)
    for y in range(H):
        for x in range(W):
            a = ((tl + (du * F(x) + dv * F(y))) - pos).astype(F)
            m = F(F(a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
            hit, out = oracle.trace_one(pos, a * (F(1.0) / np.sqrt(m)))
            if hit:
                Z[y, x], N[y, x], O[y, x] = out[0], out[4:7], int(out[7])
    return N, Z, O


@pytest.mark.parametrize("name", ["three_sphere", "cube", "monkey"])
def test_defaults_lower_the_error_against_a_converged_frame(rt, orc, models_dir, name):
    """the oracle at 4 spp x 1 frame filtered with the default parameters is closer (RMSE) to the oracle at 1024 spp than the unfiltered
    frame; the ratio is printed, only "strictly lower" is asserted.  Measured when the defaults were chosen: three_sphere 0.0657 -> 0.0184,
    cube 0.0363 -> 0.0134, monkey 0.3267 -> 0.1887."""
    W = H = 128
    objs, sky = rt.scenes.CONFIG_SCENES[name]()
    oracle = orc.Scene(objs, orc.MATH_DET, models_dir)
    cam = orc.camera_default(W, H)
    noisy = oracle.render(cam, W, H, 4, 8, sky, nthreads=16)
    target = oracle.render(cam, W, H, 1024, 8, sky, time_ms=777, nthreads=16)
    N, Z, O = oracle_planes(oracle, cam, W, H)
    out = denoise_ref(noisy, N, Z, O, None, **DEFAULTS)
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - target) ** 2)))
    changed = float((u32(out) != u32(noisy)).any(axis=2).mean())
    print("%s: rmse noisy %.4f -> denoised %.4f (ratio %.2f), %.0f %% of the pixels changed" % (name, rmse(noisy), rmse(out), rmse(out) / rmse(noisy), 100 * changed))
    assert np.isfinite(out).all()
    assert rmse(out) < rmse(noisy)


def test_defaults_are_the_librarys(rt):
    """the yardstick's defaults and rt_denoise_params_default agree (the quality test above then speaks for the library's defaults)"""
    p = rt.DenoiseParams().as_dict()
    assert p["iterations"] == DEFAULTS["iterations"] and p["normal_power_log2"] == DEFAULTS["normal_power_log2"]
    for k in ("sigma_colour", "sigma_depth", "albedo_floor"):
        assert F(p[k]) == F(DEFAULTS[k]), k
