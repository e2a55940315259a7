"""The yardstick of the edge-avoiding a-trous denoiser (rt_denoise, include/rt_amd.h): the definition in NumPy binary32, vectorised
over the pixels with a loop over levels and taps.  Every operation is one float32 operation on float32 arrays, in the order the
definition gives, so the result is what a scalar binary32 implementation without fused multiply-add computes, bit for bit.

It includes none of the product's headers and calls nothing in the library: the tests compare the device code with this, never with
itself.  Test infrastructure, not product code."""
import numpy as np

F = np.float32
ONE, ZERO = F(1.0), F(0.0)
# the B3-spline 1:4:6:4:1 scaled so that the centre is exactly 1: {1/6, 2/3, 1, 2/3, 1/6} as the nearest binary32 values
H5 = np.array([0x3E2AAAAB, 0x3F2AAAAB, 0x3F800000, 0x3F2AAAAB, 0x3E2AAAAB], np.uint32).view(F)

DEFAULTS = dict(iterations=5, sigma_colour=4.0, sigma_depth=0.02, normal_power_log2=5, albedo_floor=0.01)


def _k(x):
    """k(x) = (x < 1) ? (1 - x) * (1 - x) : 0; a NaN compares false and gives 0"""
    t = ONE - x
    return np.where(x < ONE, t * t, ZERO)


def _window(n, off):
    """the centre indices [lo, hi) along an axis of n pixels whose tap at +off lies inside it (empty: lo >= hi)"""
    return max(0, -off), min(n, n - off)


def denoise_ref(colour, normal, depth, object=None, albedo=None, iterations=5, sigma_colour=4.0, sigma_depth=0.02, normal_power_log2=5,
                albedo_floor=0.01):
    """colour, normal, albedo [H, W, 3] float32, depth [H, W] float32, object [H, W] int32 -> [H, W, 3] float32"""
    C = np.ascontiguousarray(colour, F)
    N = np.ascontiguousarray(normal, F)
    Z = np.ascontiguousarray(depth, F)
    H, W = Z.shape
    assert C.shape == (H, W, 3) and N.shape == (H, W, 3)
    O = None if object is None else np.ascontiguousarray(object, np.int32)
    assert 1 <= iterations <= 8 and 0 <= normal_power_log2 <= 8
    with np.errstate(all="ignore"):
        M = None
        if albedo is not None:
            A = np.ascontiguousarray(albedo, F)
            M = np.where(A > F(albedo_floor), A, F(albedo_floor))
            Fi = C / M
        else:
            Fi = C.copy()
        kz = ONE / (F(sigma_depth) * Z)
        for level in range(iterations):
            s = 1 << level
            sc = F(sigma_colour) * F(2.0 ** -level)
            kc = ONE / (sc * sc)
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            for dy in range(-2, 3):
                y0, y1 = _window(H, dy * s)
                for dx in range(-2, 3):
                    x0, x1 = _window(W, dx * s)
                    if y0 >= y1 or x0 >= x1:
                        continue                      # the tap is outside the image for every centre
                    p = (slice(y0, y1), slice(x0, x1))
                    q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    Fq, Fp = Fi[q], Fi[p]
                    if dx == 0 and dy == 0:
                        w = np.full((y1 - y0, x1 - x0), ONE, F)
                    else:
                        hw = H5[dy + 2] * H5[dx + 2]
                        Np, Nq = N[p], N[q]
                        dn = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                        wn = np.where(dn > ZERO, dn, ZERO)
                        for _ in range(normal_power_log2):
                            wn = wn * wn
                        r = max(abs(dx), abs(dy)) * s
                        g = ((Z[q] - Z[p]) * kz[p]) * (ONE / F(r))
                        wz = _k(g * g)
                        d = Fq - Fp
                        x = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * kc
                        wc = _k(x)
                        w = hw * ((wn * wz) * wc)
                        if O is not None:
                            w = np.where(O[q] == O[p], w, ZERO)
                    take = w != ZERO                  # a tap with w == 0 is skipped: nothing behind a zero weight spreads
                    acc[p] = np.where(take[..., None], acc[p] + w[..., None] * Fq, acc[p])
                    wsum[p] = np.where(take, wsum[p] + w, wsum[p])
            Fi = acc / wsum[..., None]
        out = Fi * M if M is not None else Fi
    assert out.dtype == F
    return out
