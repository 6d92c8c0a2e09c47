"""The float32 edges of the radius family on the CPU: the plain reference of
tests/float_edges.py against the C oracle (brute force and tree), for every
edge radius and with the poisoned queries present; and the oracle's kNN rows
of those queries.  No GPU."""
import functools

import numpy as np
import pytest

from tests import float_edges as fe
from tests.golden.inputs import uniform
from tests.parity import PAD, assert_knn_equal

N, M = 1003, 130
SQRT_MAX = np.sqrt(np.float32(fe.FLT_MAX))


@functools.lru_cache(maxsize=None)
def inputs():
    pts = uniform(N, 304)
    q = np.concatenate([uniform(M, 305), np.zeros((70, 3), np.float32) + pts[:70]])
    qp, bad, ok = fe.poison(q, 1.0)
    for a in (pts, q, qp, bad, ok):
        a.setflags(write=False)
    return pts, q, qp, bad, ok


def test_squares():
    """What each named radius squares to in float32, and the threshold."""
    f32 = np.float32
    with np.errstate(over="ignore", under="ignore"):
        sq = lambda r: f32(r) * f32(r)
        assert sq(fe.R_ZERO) == 0 and sq(fe.R_NEG_ZERO) == 0 and not np.signbit(sq(fe.R_NEG_ZERO))
        assert f32(fe.R_UNDERFLOW) > 0 and sq(fe.R_UNDERFLOW) == 0
        assert sq(fe.R_SMALL) == sq(fe.R_NEG_SMALL) == f32(0.05) * f32(0.05) > 0
        assert sq(fe.R_ALL) == 4
        assert np.isfinite(sq(fe.R_LAST_FINITE)) and 3.23e38 < sq(fe.R_LAST_FINITE) < 3.25e38
        for r in fe.RADII_OVERFLOW:
            assert np.isinf(sq(r)) and sq(r) > 0, r
            assert fe.thr(r) == f32(fe.FLT_MAX)
        assert np.isnan(sq(fe.NAN)) and np.isnan(fe.thr(fe.NAN))
    for r in (fe.R_ZERO, fe.R_NEG_ZERO, fe.R_UNDERFLOW):
        assert fe.thr(r) == 0
    assert fe.thr(fe.R_LAST_FINITE) == sq(fe.R_LAST_FINITE) < f32(fe.FLT_MAX)
    assert fe.thr(fe.R_NEG_SMALL) == fe.thr(fe.R_SMALL)
    assert fe.thr(fe.RADII_EDGE).dtype == np.float32
    assert set(fe.RADII_OVERFLOW) < set(fe.RADII_EDGE) and len(fe.RADII_EDGE) == 13
    h = np.asarray(fe.RADII_HIST, np.float32)
    assert np.all(np.diff(h) > 0) and h[0] == 0 and np.all(h <= f32(fe.FLT_MAX))


def test_poison_layout():
    pts, q, qp, bad, ok = inputs()
    assert len(bad) == 8 and len(ok) == len(q) - 8 and not np.intersect1d(bad, ok).size
    assert np.array_equal(qp[ok], q[ok]) and np.all(np.isfinite(qp[ok]))
    assert np.array_equal(qp[bad], fe.poison_rows(1.0), equal_nan=True)
    assert np.all(np.isnan(qp[bad[fe.POISON_NAN]]))
    d2 = fe.d2_matrix(pts, qp[bad], None)
    # NaN rows, rows of +inf, and the one finite value of the tie row
    assert np.all(np.isnan(d2[:2])) and np.all(np.isposinf(d2[2:7]))
    assert np.isfinite(d2[fe.POISON_TIE, 0]) and np.all(d2[fe.POISON_TIE] == d2[fe.POISON_TIE, 0])
    assert np.array_equal(fe.d2_matrix(pts, qp[bad], 1.0), d2, equal_nan=True)


@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("r", fe.RADII_EDGE, ids=lambda r: f"r={r!r}")
def test_counts_match_the_oracle(oracle, box, r):
    """ball_counts == the oracle's brute force == the oracle's tree walk, the
    poisoned queries included (the oracle clamps fl(r*r) at FLT_MAX)."""
    pts, q, qp, bad, ok = inputs()
    ref = fe.ball_counts(pts, qp, r, box)
    assert np.array_equal(oracle.ball_count_brute(pts, qp, r, box), ref)
    for leaf in (16, 64):
        assert np.array_equal(oracle.ball_count(oracle.tree(pts, leaf, box), qp, r), ref), leaf
    # the contract in words
    assert not ref[bad[:7]].any()  # NaN or d2 = inf: in no ball
    if r in fe.RADII_OVERFLOW:
        assert np.all(ref[ok] == N) and ref[bad[fe.POISON_TIE]] == N
    if r != r:
        assert not ref.any()
    if r in (fe.R_ZERO, fe.R_NEG_ZERO, fe.R_UNDERFLOW):  # the coincident points only
        assert np.array_equal(ref[ok], (np.arange(len(q)) >= M)[ok].astype(np.uint32))
    rows = fe.ball_rows(pts, qp, r, box)
    assert np.array_equal([len(x) for x in rows], ref)
    if r in fe.RADII_HIST:
        h = fe.hist_counts(pts, qp, fe.RADII_HIST, box)
        assert np.array_equal(h[:, fe.RADII_HIST.index(r)], ref)


@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("k", [1, 4, 40])
def test_oracle_knn_rows_of_poisoned_queries(oracle, box, k):
    """All padding (sqrtf(FLT_MAX), 0xFFFFFFFF), except the 1e18 row: an
    n-way exact tie, equal between the tree and the brute force up to the
    choice among tied points."""
    pts, q, qp, bad, ok = inputs()
    d, i = oracle.tree(pts, 16, box).query(qp, k)
    assert np.all(d[bad[:7]] == SQRT_MAX) and np.all(i[bad[:7]] == PAD)
    assert np.all(i[ok] != PAD) and np.all(i[bad[fe.POISON_TIE]] != PAD)
    tie = bad[fe.POISON_TIE:fe.POISON_TIE + 1]
    db, ib = oracle.knn_brute(pts, qp[tie], k, box)
    assert np.all(db == db[0, 0]) and np.isfinite(db[0, 0]) and db[0, 0] < SQRT_MAX
    assert_knn_equal(d[tie], i[tie], db, ib, pts, qp[tie], box)
    # the finite rows are those of the finite-only call
    d0, i0 = oracle.tree(pts, 16, box).query(q[ok], k)
    assert np.array_equal(d[ok], d0) and np.array_equal(i[ok], i0)
