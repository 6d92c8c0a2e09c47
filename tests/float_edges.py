"""Plain reference of the radius family at the float32 edges: radii whose
square underflows, overflows or is not a number, and queries with NaN,
infinite or huge coordinates.  Helpers only, no tests; numpy alone (no GPU, no
oracle).  The metric is tests/parity.py::d2_ref (float32, no FMA), the
threshold follows tests/aniso_ref.py::thresholds, and the predicate is the
one include/nbkd.h states: a point is inside iff d2 <= T in float32 with
T = min(fl(r*r), FLT_MAX); a NaN on either side of `<=` is outside."""
import numpy as np

from tests.parity import d2_ref

FLT_MAX = float(np.finfo(np.float32).max)
INF, NAN = float("inf"), float("nan")

# name -> radius.  The float32 squares are asserted in
# tests/test_float_edges_host.py::test_squares.
R_ZERO, R_NEG_ZERO, R_UNDERFLOW = 0.0, -0.0, 1e-30  # 1e-30^2 underflows to 0: coincident points only
R_SMALL, R_NEG_SMALL, R_ALL = 0.05, -0.05, 2.0
R_LAST_FINITE, R_FIRST_OVERFLOW = 1.8e19, 1.9e19     # squares 3.24e38 (finite) and 3.61e38 (inf)
R_HUGE = 3e38
RADII_EDGE = (R_ZERO, R_NEG_ZERO, R_UNDERFLOW, R_SMALL, R_NEG_SMALL, R_ALL, R_LAST_FINITE,
              R_FIRST_OVERFLOW, R_HUGE, FLT_MAX, INF, -INF, NAN)
# the radii whose fl(r*r) overflows: T = FLT_MAX, every finite d2 is inside
RADII_OVERFLOW = (R_FIRST_OVERFLOW, R_HUGE, FLT_MAX, INF, -INF)
# nbkd_query_ball_hist's radii: ascending, finite, not negative
RADII_HIST = (R_ZERO, R_UNDERFLOW, R_SMALL, R_ALL, R_LAST_FINITE, R_FIRST_OVERFLOW, R_HUGE,
              FLT_MAX)


def thr(r):
    """T = min(fl(r*r), FLT_MAX) in float32 (scalar or array); NaN stays NaN"""
    r = np.asarray(r, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = r * r
    return np.where(r2 > np.float32(FLT_MAX), np.float32(FLT_MAX), r2).astype(np.float32)


def d2_matrix(pts, q, box=None, chunk=512):
    """(m, n) float32 squared distances of queries q to points pts"""
    pts = np.asarray(pts, np.float32)
    q = np.asarray(q, np.float32).reshape(-1, 3)
    out = np.empty((len(q), len(pts)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(q), chunk):
            out[a:a + chunk] = d2_ref(q[a:a + chunk, None, :], pts[None, :, :], box)
    return out


def inside(pts, q, r, box=None):
    """(m, n) bool: point j is in the ball of radius r about query i"""
    with np.errstate(invalid="ignore"):
        return d2_matrix(pts, q, box) <= thr(r)


def ball_rows(pts, q, r, box=None):
    """one ascending uint32 array of point rows per query"""
    return [np.flatnonzero(row).astype(np.uint32) for row in inside(pts, q, r, box)]


def ball_counts(pts, q, r, box=None):
    return inside(pts, q, r, box).sum(axis=1).astype(np.uint32)


def hist_counts(pts, q, radii, box=None):
    """(m, nr) uint32: column j = ball_counts(pts, q, radii[j]) (cumulative)"""
    d2 = d2_matrix(pts, q, box)
    with np.errstate(invalid="ignore"):
        return np.stack([(d2 <= t).sum(axis=1) for t in thr(radii)], axis=1).astype(np.uint32)


def fof_one_group(n):
    """(labels, sizes, ngroups) of n points that are all friends"""
    sizes = np.zeros(n, np.uint32)
    sizes[0] = n
    return np.zeros(n, np.uint32), sizes, 1


def poison_rows(L=1.0):
    """the (8, 3) float32 poisoned queries for a box of side L"""
    h = L / 2
    return np.array([
        (NAN, NAN, NAN),
        (h, NAN, h),
        (INF, h, h),
        (h, h, -INF),
        (FLT_MAX, h, h),
        (-FLT_MAX, -FLT_MAX, -FLT_MAX),
        (1e20, h, h),   # every d2 overflows
        (1e18, h, h),   # every d2 rounds to one finite float32 value: an n-way exact tie
    ], np.float32)


POISON_NAN, POISON_TIE = 0, 7  # rows of poison_rows(): all-NaN; the 1e18 tie query


def poison(q, L=1.0):
    """(copy of q with the poisoned rows written at fixed, spread positions,
    their positions `bad` in the order of poison_rows(), the other positions
    `ok`).  The positions share 64- and 128-lane packets with finite rows at
    the front, in the middle and at the end of the array."""
    q = np.array(q, np.float32, copy=True)
    m = len(q)
    assert m >= 200
    bad = np.array([0, 1, 63, 64, 100, 127, m - 2, m - 1])
    q[bad] = poison_rows(L)
    ok = np.setdiff1d(np.arange(m), bad)
    return q, bad, ok
