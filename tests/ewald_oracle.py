"""numpy oracles of nbkd_gravity_ewald shared by its two test files: the
float64 Ewald sums of nbkd.h (alpha = 2, |n_i| <= 4, |h|^2 <= 16, no table) and
the trilinear interpolation of the exported table in the stated float32 steps."""
import numpy as np

try:
    from scipy.special import erfc as _erfc
except ImportError:  # the same function, slower
    import math
    _erfc = np.frompyfunc(math.erfc, 1, 1)

ALPHA = 2.0
C0 = -2.8372975  # C_phi at the origin
N = 64

_r = np.arange(-4, 5)
IMAGES = np.stack(np.meshgrid(_r, _r, _r, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
_h2 = (IMAGES * IMAGES).sum(1)
H = IMAGES[(_h2 > 0) & (_h2 <= 16)]
H2 = (H * H).sum(1)
HW = np.exp(-np.pi ** 2 * H2 / ALPHA ** 2) / H2


def erfc(x):
    return np.asarray(_erfc(x), dtype=np.float64)


def corrections(x, images=None):
    """(C_phi (m,), C_a (m, 3)) in float64 at the offsets x (m, 3) in units of
    the box, |x_i| <= 1/2: psi(x) - 1/|x| and -grad psi(x) - x/|x|^3, the
    nearest image's own term taken as -erf(a r)/r (its limit at x = 0).
    images: the real-space images summed (default: all with |n_i| <= 4)."""
    IMAGES = globals()["IMAGES"] if images is None else np.asarray(images, np.float64)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    cphi, ca = np.empty(len(x)), np.empty((len(x), 3))
    g0 = 2.0 * ALPHA / np.sqrt(np.pi)
    for a in range(0, len(x), 1024):
        xs = x[a:a + 1024]
        d = xs[:, None, :] - IMAGES[None, :, :]
        r2 = (d * d).sum(2)
        zero = r2 == 0
        r = np.sqrt(np.where(zero, 1.0, r2))
        e = erfc(ALPHA * r)
        # the nearest image (n = 0) without its Newtonian part
        own = (IMAGES == 0).all(1)[None, :]
        e = np.where(own, e - 1.0, e)
        g = g0 * np.exp(-ALPHA ** 2 * r2)
        p = np.where(zero, -g0, e / r)
        w = np.where(zero, 0.0, (e + g * r) / np.where(zero, 1.0, r2 * r))
        arg = 2.0 * np.pi * (xs @ H.T)
        cphi[a:a + 1024] = p.sum(1) + (HW * np.cos(arg)).sum(1) / np.pi - np.pi / ALPHA ** 2
        ca[a:a + 1024] = (w[:, :, None] * d).sum(1) + 2.0 * ((HW * np.sin(arg)) @ H)
    return cphi, ca


def interpolate(table, d, L):
    """the correction (C_phi, C_ax, C_ay, C_az) of the wrapped float32 offsets d
    (m, 3) in a box of size L, in nbkd.h's float32 steps: (values (m, 4)
    float32, cmax (m, 4) = the largest corner magnitude per channel)"""
    f32 = np.float32
    d = np.asarray(d, f32).reshape(-1, 3)
    iL = f32(1.0) / f32(L)
    sc = f32(128.0) * iL
    t = np.abs(d) * sc
    assert t.dtype == f32
    i = np.minimum(t.astype(np.int32), N - 1)
    f = t - i.astype(f32)

    def corner(ox, oy, oz):
        return table[i[:, 0] + ox, i[:, 1] + oy, i[:, 2] + oz]

    def lerp(a, b, w):
        r = a + w[:, None] * (b - a)
        assert r.dtype == f32
        return r

    c = {(ox, oy, oz): corner(ox, oy, oz) for ox in (0, 1) for oy in (0, 1) for oz in (0, 1)}
    cmax = np.max(np.abs(np.stack(list(c.values()))), axis=0)
    v = {(oy, oz): lerp(c[0, oy, oz], c[1, oy, oz], f[:, 0]) for oy in (0, 1) for oz in (0, 1)}
    w = {oz: lerp(v[0, oz], v[1, oz], f[:, 1]) for oz in (0, 1)}
    out = lerp(w[0], w[1], f[:, 2])
    out[:, 1:] = np.where(d < 0, -out[:, 1:], out[:, 1:])
    return out, cmax
