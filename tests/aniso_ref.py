"""Brute-force reference of the anisotropic pair counts (nbkd_query_ball_hist2),
plain helpers, no tests.  The per-axis squares are formed exactly as
tests/parity.py::d2_ref forms them and returned per axis; the definitions of
include/nbkd.h are then applied with float32 numpy arrays, threshold by
threshold, with the test written `~(x <= t)`."""
import numpy as np

RPPI, SMU = 0, 1
FLT_MAX = np.finfo(np.float32).max


def axes_ref(q, p, boxsize=None):
    """the float32 per-axis squares d2_ref adds up, shape (..., 3)"""
    q = np.asarray(q, np.float32)
    p = np.asarray(p, np.float32)
    d = p - q
    if boxsize is not None:
        L = np.float32(boxsize)
        dm = d - L
        dp = d + L
        return np.minimum(np.minimum(d * d, dm * dm), dp * dp)
    return d * d


def thresholds(edges):
    """fl(e * e) in float32, a product that overflows counting as FLT_MAX"""
    e = np.asarray(edges, np.float32)
    with np.errstate(over="ignore"):
        return np.minimum(e * e, FLT_MAX)


def coords(a, mode, los):
    """(first-axis coordinate, pi2, s2) of the per-axis squares a (..., 3)"""
    u, v = [x for x in range(3) if x != los]
    pi2 = a[..., los]
    rp2 = a[..., u] + a[..., v]
    s2 = (a[..., 0] + a[..., 1]) + a[..., 2]
    assert rp2.dtype == np.float32 and s2.dtype == np.float32
    return (rp2 if mode == RPPI else s2), pi2, s2


def bins(a, t1, t2, mode, los):
    """(b1, b2) of every pair of the per-axis squares a (..., 3)"""
    x1, pi2, s2 = coords(a, mode, los)
    b1 = np.zeros(x1.shape, np.int64)
    for t in t1:
        b1 += ~(x1 <= t)
    b2 = np.zeros(x1.shape, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in t2:
            b2 += ~(pi2 <= (t * s2 if mode == SMU else t))
    return b1, b2


def hist2_ref(pts, q, edges1, edges2, mode, los, boxsize=None, chunk=256):
    """the (n1, n2) uint64 counts of queries q against points pts"""
    pts = np.asarray(pts, np.float32)
    q = np.asarray(q, np.float32)
    t1, t2 = thresholds(edges1), thresholds(edges2)
    n1, n2 = len(t1), len(t2)
    out = np.zeros(n1 * n2, np.uint64)
    for i in range(0, len(q), chunk):
        a = axes_ref(q[i:i + chunk, None, :], pts[None, :, :], boxsize)
        b1, b2 = bins(a, t1, t2, mode, los)
        ok = (b1 < n1) & (b2 < n2)
        out += np.bincount((b1 * n2 + b2)[ok], minlength=n1 * n2).astype(np.uint64)
    return out.reshape(n1, n2)


def tie_counts(pts, q, edges1, edges2, mode, los, boxsize=None):
    """how many pairs sit exactly on each threshold: (first axis, second axis),
    one count per edge; the second axis among the pairs inside the last
    first-axis edge"""
    t1, t2 = thresholds(edges1), thresholds(edges2)
    a = axes_ref(np.asarray(q, np.float32)[:, None, :], np.asarray(pts, np.float32)[None, :, :],
                 boxsize)
    x1, pi2, s2 = coords(a, mode, los)
    inside = x1 <= t1[-1]
    first = [int((x1 == t).sum()) for t in t1]
    second = [int(((pi2 == (t * s2 if mode == SMU else t)) & inside).sum()) for t in t2]
    return first, second
