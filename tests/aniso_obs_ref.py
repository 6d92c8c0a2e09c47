"""Brute-force references of the observer-frame pair counts
(nbkd_query_ball_hist2_obs), plain helpers, no tests.

hist2_obs_ref applies the definitions of include/nbkd.h with float32 numpy
arrays, operation by operation (numpy neither fuses a multiply into an add nor
flushes denormals, and its float32 division is the IEEE one), threshold by
threshold, with the test written `~(x <= t)`.  hist2_obs_geo is the geometry in
float64 (pi = |s . l| / |l|, rp = sqrt(s^2 - pi^2), mu = pi / s), which also
counts the pairs that lie within a relative 1e-4 of an edge: the float32
definitions may put those, and only those, into a neighbouring bin."""
import numpy as np

from tests.aniso_ref import RPPI, SMU, thresholds


def coords_obs(q, p, o):
    """(s2, pi2, rp2, clamped) of float32 queries q (..., 3) against points p
    (..., 3), observer o (3,); clamped: where fl(x / l2) > s2 and the clamp
    fired"""
    q = np.asarray(q, np.float32)
    p = np.asarray(p, np.float32)
    o = np.asarray(o, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        s = p - q
        s2 = (s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2]
        l = (p - o) + (q - o)
        dot = (s[..., 0] * l[..., 0] + s[..., 1] * l[..., 1]) + s[..., 2] * l[..., 2]
        l2 = (l[..., 0] * l[..., 0] + l[..., 1] * l[..., 1]) + l[..., 2] * l[..., 2]
        x = dot * dot
        quot = x / l2
        # (fminf: the other operand where one is NaN)
        pi2 = np.where(l2 > 0, np.fmin(quot, s2), np.float32(0))
        rp2 = s2 - pi2
        clamped = (l2 > 0) & (quot > s2)
    assert s2.dtype == pi2.dtype == rp2.dtype == np.float32
    return s2, pi2, rp2, clamped


def bins_obs(s2, pi2, rp2, t1, t2, mode):
    x1 = rp2 if mode == RPPI else s2
    b1 = np.zeros(x1.shape, np.int64)
    for t in t1:
        b1 += ~(x1 <= t)
    b2 = np.zeros(x1.shape, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in t2:
            b2 += ~(pi2 <= (t * s2 if mode == SMU else t))
    return b1, b2


def hist2_obs_ref(pts, q, edges1, edges2, mode, observer, chunk=256):
    """the (n1, n2) uint64 counts of queries q against points pts"""
    pts = np.asarray(pts, np.float32)
    q = np.asarray(q, np.float32)
    t1, t2 = thresholds(edges1), thresholds(edges2)
    n1, n2 = len(t1), len(t2)
    out = np.zeros(n1 * n2, np.uint64)
    for i in range(0, len(q), chunk):
        s2, pi2, rp2, _ = coords_obs(q[i:i + chunk, None, :], pts[None, :, :], observer)
        b1, b2 = bins_obs(s2, pi2, rp2, t1, t2, mode)
        ok = (b1 < n1) & (b2 < n2)
        out += np.bincount((b1 * n2 + b2)[ok], minlength=n1 * n2).astype(np.uint64)
    return out.reshape(n1, n2)


def clamp_count(pts, q, observer, chunk=256):
    """how many pairs have fl(x / l2) > s2"""
    pts = np.asarray(pts, np.float32)
    q = np.asarray(q, np.float32)
    return sum(int(coords_obs(q[i:i + chunk, None, :], pts[None, :, :], observer)[3].sum())
               for i in range(0, len(q), chunk))


def tie_counts_obs(pts, q, edges1, edges2, mode, observer, chunk=256):
    """how many pairs sit exactly on each threshold: (first axis, second axis,
    pairs with s2 > 0 and l2 == 0); the second axis among the pairs inside the
    last first-axis edge"""
    pts = np.asarray(pts, np.float32)
    q = np.asarray(q, np.float32)
    o = np.asarray(observer, np.float32)
    t1, t2 = thresholds(edges1), thresholds(edges2)
    first, second, mirror = np.zeros(len(t1), np.int64), np.zeros(len(t2), np.int64), 0
    for i in range(0, len(q), chunk):
        qq, pp = q[i:i + chunk, None, :], pts[None, :, :]
        s2, pi2, rp2, _ = coords_obs(qq, pp, o)
        x1 = rp2 if mode == RPPI else s2
        inside = x1 <= t1[-1]
        first += [int((x1 == t).sum()) for t in t1]
        second += [int(((pi2 == (t * s2 if mode == SMU else t)) & inside).sum()) for t in t2]
        l = (pp - o) + (qq - o)
        mirror += int((np.all(l == 0, axis=-1) & (s2 > 0)).sum())
    return first.tolist(), second.tolist(), mirror


def hist2_obs_geo(pts, q, edges1, edges2, mode, observer, rel=1e-4, chunk=256):
    """float64 geometry on the same float32 inputs: ((n1, n2) uint64 counts, the
    number of pairs with a coordinate within rel * (its axis' last edge) of one
    of that axis' edges).  Bins as in the header with `>` on the coordinates
    themselves: b = #{k : x > e[k]}."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    q = np.asarray(q, np.float32).astype(np.float64)
    o = np.asarray(observer, np.float32).astype(np.float64)
    e1 = np.asarray(edges1, np.float32).astype(np.float64)
    e2 = np.asarray(edges2, np.float32).astype(np.float64)
    n1, n2 = len(e1), len(e2)
    out = np.zeros(n1 * n2, np.uint64)
    near = 0
    for i in range(0, len(q), chunk):
        qq, pp = q[i:i + chunk, None, :], p[None, :, :]
        s = pp - qq
        l = (pp - o) + (qq - o)
        sn2 = (s * s).sum(-1)
        ln2 = (l * l).sum(-1)
        dot = (s * l).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            pi = np.where(ln2 > 0, np.abs(dot) / np.sqrt(ln2), 0.0)
            pi = np.minimum(pi, np.sqrt(sn2))
            sn = np.sqrt(sn2)
            if mode == RPPI:
                x1, x2 = np.sqrt(np.maximum(sn2 - pi * pi, 0.0)), pi
            else:
                x1, x2 = sn, np.where(sn > 0, pi / sn, 0.0)
        b1 = (x1[..., None] > e1).sum(-1)
        b2 = (x2[..., None] > e2).sum(-1)
        ok = (b1 < n1) & (b2 < n2)
        out += np.bincount((b1 * n2 + b2)[ok], minlength=n1 * n2).astype(np.uint64)
        close = (np.abs(x1[..., None] - e1) <= rel * e1[-1]).any(-1)
        close |= (np.abs(x2[..., None] - e2) <= rel * e2[-1]).any(-1)
        # (a pair far outside the first axis is in no bin either way)
        near += int((close & (x1 <= e1[-1] * (1 + rel))).sum())
    return out.reshape(n1, n2), near
