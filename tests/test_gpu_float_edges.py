"""The float32 edges of radii and queries on the GPU, against the plain
reference of tests/float_edges.py (and the C oracle for kNN rows).

Radii: fl(r*r) that underflows to 0, that overflows (the threshold is then
FLT_MAX: every point at a finite distance is inside, the padding points and
the kernels' filler lanes at d2 = inf are not), negative radii, NaN.
Queries: NaN, infinite and huge coordinates sharing a call -- and so the
packets, the walk, the votes, the staging and the seed / retry machinery --
with finite queries, whose rows must not change.

Trees: n = 9 and 1003 (7 and 5 padding rows, a padded partial last leaf),
n = 64 (no padding), leaf sizes 16 and 64, and n = 5000 with leaf size 128
(two staged chunks per leaf), each plain and periodic.  Every comparison is
exact equality."""
import functools

import numpy as np
import pytest

from tests import aniso_ref
from tests import float_edges as fe
from tests.golden.inputs import uniform
from tests.parity import PAD, assert_knn_equal

pytestmark = pytest.mark.gpu

L = 1.0
TREES = [(9, 16), (9, 64), (64, 16), (64, 64), (1003, 16), (1003, 64), (5000, 128)]
CASES = [(n, leaf, box) for n, leaf in TREES for box in (None, L)]
case = pytest.mark.parametrize("n,leaf,box", CASES)
GUARD = 64
DEAD = 0xDEADBEEF
SQRT_MAX = np.sqrt(np.float32(fe.FLT_MAX))


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(points, finite queries, queries with the poisoned rows, bad, ok)"""
    pts = uniform(n, 304)
    q = np.concatenate([uniform(200, 305), pts[:40]])
    qp, bad, ok = fe.poison(q, L)
    for a in (pts, q, qp, bad, ok):
        a.setflags(write=False)
    return pts, q, qp, bad, ok


@functools.lru_cache(maxsize=None)
def ref_counts(n, box, which):
    """(rows, 13) counts at RADII_EDGE of the finite ("q"), the poisoned ("qp")
    or the self ("pts") queries: one distance matrix for all the radii"""
    pts, q, qp, _, _ = inputs(n)
    out = fe.hist_counts(pts, {"q": q, "qp": qp, "pts": pts[:self_rows(n)]}[which],
                         fe.RADII_EDGE, box)
    out.setflags(write=False)
    return out


def self_rows(n):
    """the self queries: the whole build array (the tree's own order), or on
    the largest tree a prefix of it (the order is then gathered from a bitmap)"""
    return n if n <= 1003 else 1000


def counts_of(n, box, r, which="q"):
    """the column of radius r (found by its bits: NaN and -0.0 are radii of their own)"""
    bits = np.asarray(fe.RADII_EDGE, np.float32).view(np.uint32)
    j = int(np.flatnonzero(bits == np.float32(r).view(np.uint32))[0])
    return ref_counts(n, box, which)[:, j]


@pytest.fixture
def knobs(gpu):
    names = ("host_batch", "knn_seed_margin", "self_order")
    saved = {k: gpu.get_tuning(k) for k in names}
    yield gpu
    for k, v in saved.items():
        gpu.set_tuning(k, v)
    gpu.timing_enable(False)


def guarded(size):
    from nbodyhpc_amd import hip
    return hip.DeviceArray.from_numpy(np.full(size + GUARD, DEAD, np.uint32))


def split_guard(d, size):
    a = d.numpy()
    assert np.all(a[size:] == DEAD), "a word past the output was written"
    return a[:size]


# ================================================================== radii
@case
def test_ball_count_radii(knobs, n, leaf, box):
    """Host call, device call, three or more host batches and the self-order
    path (the queries are the build array) equal the reference at every edge
    radius; an overflowing radius gives exactly n."""
    from nbodyhpc_amd import hip
    gpu = knobs
    pts, q, _, _, _ = inputs(n)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    dq = hip.DeviceArray.from_numpy(q)
    dp = hip.DeviceArray.from_numpy(pts)
    ts = gpu.Tree(n=n, dev_ptr=dp.ptr, leafsize=leaf, boxsize=box)
    gpu.timing_enable(True)
    for r in fe.RADII_EDGE:
        ref = counts_of(n, box, r)
        if r in fe.RADII_OVERFLOW:
            assert np.all(ref == n)
        got = t.ball_count(q, r)
        assert np.array_equal(got, ref), (r, np.flatnonzero(got != ref)[:5], got.max())
        dc = guarded(len(q))
        t.ball_count_device(dq.ptr, len(q), r, dc.ptr)
        hip.synchronize()
        assert np.array_equal(split_guard(dc, len(q)), ref), r
        gpu.set_tuning("host_batch", 64)  # 64 + 64 + 64 + the rest
        try:
            assert np.array_equal(t.ball_count(q, r), ref), r
        finally:
            gpu.set_tuning("host_batch", 0)
        # the self-order path
        sref = counts_of(n, box, r, "pts")
        ms = self_rows(n)
        ds = guarded(ms)
        gpu.timing_reset()
        ts.ball_count_device(dp.ptr, ms, r, ds.ptr)
        hip.synchronize()
        if n >= 1003:  # (a one-leaf tree has no split heap and takes the sorted path)
            assert gpu.timing_read("self_order")[1] > 0
        got = split_guard(ds, ms)
        assert np.array_equal(got, sref), (r, np.flatnonzero(got != sref)[:5])
        if r in fe.RADII_OVERFLOW:
            assert np.all(got == n)


@case
def test_ball_csr_radii(gpu, n, leaf, box):
    """Offsets are the reference counts, sorted rows the reference rows
    (arange(n) at an overflowing radius), unsorted rows the same sets, no id
    is >= n, and a device-output call writes nothing past offsets[m]."""
    from nbodyhpc_amd import hip
    pts, q, _, _, _ = inputs(n)
    m = len(q)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    dq = hip.DeviceArray.from_numpy(q)
    for r in fe.RADII_EDGE:
        cnt = counts_of(n, box, r).astype(np.int64)
        rows = fe.ball_rows(pts, q, r, box)
        flat = np.concatenate(rows) if cnt.sum() else np.empty(0, np.uint32)
        if r in fe.RADII_OVERFLOW:
            assert np.array_equal(flat, np.tile(np.arange(n, dtype=np.uint32), m))
        off, idx = t.ball_csr(q, r, sorted=True)
        assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), cnt), r
        assert idx.size == cnt.sum() and (idx.size == 0 or idx.max() < n), r
        assert np.array_equal(idx, flat), r
        off2, idx2 = t.ball_csr(q, r, sorted=False)
        assert np.array_equal(off2, off) and idx2.size == idx.size, r
        assert idx2.size == 0 or idx2.max() < n, r
        # rows as sets: sort (row, id) pairs
        rowid = np.repeat(np.arange(m), cnt)
        assert np.array_equal(idx2[np.lexsort((idx2, rowid))], flat), r
        # device queries, device ids behind guard words
        nnz = int(off[-1])
        doff = np.empty(m + 1, np.uint64)
        for srt in (True, False):
            di = guarded(nnz)
            t.ball_csr_device(dq.ptr, m, r, doff, di.ptr, nnz, sorted=srt)
            hip.synchronize()
            got = split_guard(di, nnz)
            assert np.array_equal(doff, off), r
            assert np.array_equal(got if srt else got[np.lexsort((got, rowid))], flat), (r, srt)


@case
def test_ball_hist_radii(gpu, n, leaf, box):
    """Rows are the reference's cumulative counts, column j is
    ball_count(q, radii[j]), totals are the column sums; on the periodic tree
    some queries lie outside [0, L]^3 (the brute-force kernel)."""
    from nbodyhpc_amd import hip
    pts, q, _, _, _ = inputs(n)
    q = q.copy()
    if box is not None:
        q[:7] += np.float32(1.5)
        q[100:105] -= np.float32(0.7)
        q[239 if len(q) > 239 else -1, 1] = np.float32(-3.25)
    radii = np.asarray(fe.RADII_HIST, np.float32)
    ref = fe.hist_counts(pts, q, radii, box)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    c, tot = t.ball_hist(q, radii)
    assert np.array_equal(c, ref), np.argwhere(c != ref)[:5]
    assert np.array_equal(tot, ref.sum(axis=0, dtype=np.uint64))
    for j, r in enumerate(radii):
        assert np.array_equal(t.ball_count(q, r), ref[:, j]), r
    assert np.all(ref[:, 4:] == n)  # every finite d2 is inside from 1.8e19 on
    # totals alone; device rows behind guard words
    _, tot2 = t.ball_hist(q, radii, counts=False)
    assert np.array_equal(tot2, tot)
    dq = hip.DeviceArray.from_numpy(q)
    dc = guarded(ref.size)
    tot3 = t.ball_hist_device(dq.ptr, len(q), radii, dc.ptr)
    hip.synchronize()
    assert np.array_equal(split_guard(dc, ref.size).reshape(ref.shape), ref)
    assert np.array_equal(tot3, tot)


@case
def test_fof_overflowing_b(gpu, n, leaf, box):
    """A finite b whose square overflows (or nearly does) links every real
    point and no padding position: one group, nothing written at or past n."""
    from nbodyhpc_amd import hip
    pts = inputs(n)[0]
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    rl, rs, rg = fe.fof_one_group(n)
    for b in (fe.R_LAST_FINITE, fe.R_FIRST_OVERFLOW, fe.FLT_MAX):
        lab, siz, ng = t.fof(b)
        assert ng == rg and np.array_equal(lab, rl) and np.array_equal(siz, rs), b
        dl, dz = guarded(n), guarded(n)
        t.fof_device(b, dl.ptr, dz.ptr)
        hip.synchronize()
        assert np.array_equal(split_guard(dl, n), rl), b
        assert np.array_equal(split_guard(dz, n), rs), b


@pytest.mark.parametrize("n,leaf,box", [(9, 16, None), (1003, 16, L), (1003, 64, None)])
def test_python_surface_infinite_radius(gpu, n, leaf, box):
    from nbodyhpc_amd.kdtree import KDTree
    pts, q, _, _, _ = inputs(n)
    t = KDTree(pts, leafsize=leaf, boxsize=box)
    rows = t.query_ball(q, np.inf)
    assert rows.shape == (len(q),)
    for row in rows:
        assert np.array_equal(row, np.arange(n))
    assert np.all(t.query_ball(q, np.inf, return_length=True) == n)
    assert np.all(t.query_ball(q, -np.inf, return_length=True) == n)
    assert not t.query_ball(q, np.nan, return_length=True).any()
    off, idx = t.query_ball(q, np.nan, return_csr=True)
    assert not off.any() and idx.size == 0


# ================================================================== poisoned queries
def query_sets(n):
    """(name, queries, rows of the whole poisoned array they are) of the three
    calls each poisoned-query test makes"""
    _, _, qp, bad, _ = inputs(n)
    return (("all", qp, np.arange(len(qp))), ("bad only", qp[bad], bad),
            ("one NaN row", qp[bad[:1]], bad[:1]))


@pytest.mark.parametrize("k", [1, 4, 40, 100, 1500])
@case
def test_knn_poisoned(knobs, oracle, n, leaf, box, k):
    """query and query_kth, plain, squared and with a seed margin so small
    that the retry rounds run: the finite rows are bit for bit those of the
    finite-only call and match the oracle; the poisoned rows are the oracle's
    (all padding, but for the n-way tie of the 1e18 row)."""
    gpu = knobs
    pts, q, qp, bad, ok = inputs(n)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    otree = oracle.tree(pts, leaf, box)
    oref = {sq: otree.query(qp, k, sqrt=not sq) for sq in (False, True)}
    for name, squared, margin in (("plain", False, None), ("squared", True, None),
                                  ("retry", False, 0.05)):
        if margin is not None and k > 1024:
            continue  # the lane-per-query kernel takes every row: no seed, no retry
        if margin is not None:
            gpu.set_tuning("knn_seed_margin", margin)
        dr, ir = oref[squared]
        padv = np.float32(fe.FLT_MAX) if squared else SQRT_MAX
        assert np.all(ir[bad[:7]] == PAD) and np.all(dr[bad[:7]] == padv)
        nreal = min(k, n)
        assert np.all(ir[bad[7], :nreal] != PAD) and np.all(dr[bad[7], :nreal] == dr[bad[7], 0])
        d0, i0 = t.query(q[ok], k, squared=squared)
        for what, qq, rows in query_sets(n):
            tag = (name, what)
            d, i = t.query(qq, k, squared=squared)
            assert_knn_equal(d, i, dr[rows], ir[rows], pts, qq, box, sqrt=not squared)
            if not squared:
                kth = t.query_kth(qq, k)
                assert np.array_equal(kth.view(np.uint32), d[:, k - 1].view(np.uint32)), tag
            if what == "all":
                assert np.array_equal(d[ok].view(np.uint32), d0.view(np.uint32)), tag
                assert_knn_equal(d[ok], i[ok], d0, i0, pts, q[ok], box, sqrt=not squared)
                assert np.all(i[bad[:7]] == PAD) and np.all(d[bad[:7]] == padv), tag
            else:
                assert np.all(i[:1] == PAD) and np.all(d[:1] == padv), tag


@case
def test_radius_family_poisoned(gpu, n, leaf, box):
    """ball_count, ball_csr and ball_hist with the poisoned rows present: the
    reference at every row (a NaN or d2 = inf query: an empty ball), and the
    finite rows those of the finite-only call."""
    pts, q, qp, bad, ok = inputs(n)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    # nbkd_query_ball_hist takes finite radii: FLT_MAX stands for inf (T = FLT_MAX)
    hr = np.array([fe.R_SMALL, fe.R_ALL, fe.FLT_MAX], np.float32)
    href = fe.hist_counts(pts, qp, hr, box)
    assert not href[bad[:7]].any() and np.all(href[bad[7]] == (0, 0, n))
    for what, qq, rows in query_sets(n):
        for j, r in enumerate((fe.R_SMALL, fe.R_ALL, fe.INF)):
            ref = counts_of(n, box, r, "qp")[rows]
            assert np.array_equal(ref, href[rows, j])
            got = t.ball_count(qq, r)
            assert np.array_equal(got, ref), (what, r, np.flatnonzero(got != ref)[:5])
            for srt in (True, False):
                off, idx = t.ball_csr(qq, r, sorted=srt)
                assert np.array_equal(np.diff(off.astype(np.int64)), ref), (what, r)
                want = np.concatenate(fe.ball_rows(pts, qq, r, box) + [np.empty(0, np.uint32)])
                rowid = np.repeat(np.arange(len(qq)), ref.astype(np.int64))
                assert np.array_equal(idx if srt else idx[np.lexsort((idx, rowid))], want), (what, r)
            if what == "all":
                assert np.array_equal(got[ok], t.ball_count(q[ok], r)), r
        c, tot = t.ball_hist(qq, hr)
        assert np.array_equal(c, href[rows]), what
        assert np.array_equal(tot, href[rows].sum(axis=0, dtype=np.uint64)), what
        if what == "all":
            c0, tot0 = t.ball_hist(q[ok], hr)
            assert np.array_equal(c[ok], c0)
            assert np.array_equal(tot - tot0, href[bad].sum(axis=0, dtype=np.uint64))


@case
def test_ball_sum_and_profile_poisoned(gpu, n, leaf, box):
    """Top-hat sums without values and profiles without values or scale are
    integer-valued (exact below 2^24): counts, sums and bins equal the
    reference, the rows of NaN and d2 = inf queries are zero."""
    pts, q, qp, bad, ok = inputs(n)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    pr = np.array([fe.R_SMALL, fe.R_ALL, fe.R_FIRST_OVERFLOW], np.float32)
    cum = fe.hist_counts(pts, qp, pr, box).astype(np.int64)
    bins = np.diff(cum, axis=1, prepend=0).astype(np.float32)
    assert not bins[bad[:7]].any() and np.array_equal(bins[bad[7]], (0, 0, n))
    for what, qq, rows in query_sets(n):
        for r in (fe.R_SMALL, fe.R_ALL, fe.FLT_MAX):
            ref = counts_of(n, box, r, "qp")[rows]
            s, c = t.ball_sum(qq, np.full(len(qq), r, np.float32), kernel=gpu.KERNEL_TOPHAT,
                              count=True)
            assert np.array_equal(c, ref), (what, r)
            assert s.dtype == np.float32 and np.array_equal(s, ref.astype(np.float32)), (what, r)
            if what == "all":
                s0, c0 = t.ball_sum(q[ok], np.full(len(ok), r, np.float32),
                                    kernel=gpu.KERNEL_TOPHAT, count=True)
                assert np.array_equal(c[ok], c0) and np.array_equal(s[ok], s0), r
                assert not c[bad[:7]].any() and not s[bad[:7]].any(), r
        p = t.ball_profile(qq, pr)
        assert p.dtype == np.float32 and np.array_equal(p, bins[rows]), what
        if what == "all":
            assert np.array_equal(p[ok], t.ball_profile(q[ok], pr))
            assert not p[bad[:7]].any()


@pytest.mark.parametrize("mode", [aniso_ref.RPPI, aniso_ref.SMU])
@case
def test_ball_hist2_poisoned(gpu, n, leaf, box, mode):
    """The pair counts with the poisoned queries present are those of the
    finite queries alone, and both are the brute force's."""
    pts, q, qp, bad, ok = inputs(n)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    e1 = np.array([0.05, 0.2, 2.0], np.float32)
    e2 = np.array([0.02, 0.1, 2.0] if mode == aniso_ref.RPPI else [0.25, 0.5, 1.0], np.float32)
    for los in (1, 2):
        with np.errstate(all="ignore"):
            ref = aniso_ref.hist2_ref(pts, q[ok], e1, e2, mode, los, box)
            assert np.array_equal(aniso_ref.hist2_ref(pts, qp, e1, e2, mode, los, box), ref)
        assert ref.sum() == n * len(ok)  # the last edges hold every finite pair
        assert np.array_equal(t.ball_hist2(q[ok], e1, e2, mode, los), ref), los
        assert np.array_equal(t.ball_hist2(qp, e1, e2, mode, los), ref), los
        assert not t.ball_hist2(qp[bad], e1, e2, mode, los).any(), los
        assert not t.ball_hist2(qp[bad[:1]], e1, e2, mode, los).any(), los
