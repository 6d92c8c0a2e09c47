"""Radius histogram (nbkd_query_ball_hist, ball_hist.hip): the radius count for
many ascending radii in one tree walk.  By definition column j of the result
is nbkd_query_ball_count(q, r[j]) -- the number of points with d2 <= r[j]^2 in
the tree's f32 metric -- so every comparison here is exact equality, against
the oracle's brute force (oracle.ball_count_brute) and against the existing
single-radius path.  New (no reference counterpart: the reference has no
radius search)."""
import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import d2_ref

pytestmark = pytest.mark.gpu

RADII = np.array([0.0, 0.01, 0.02, 0.05, 0.05, 0.11], np.float32)


def _brute(oracle, pts, q, radii, box):
    return np.stack([oracle.ball_count_brute(pts, q, float(r), box) for r in radii], axis=1)


@pytest.mark.parametrize("box", [None, 1.0])
def test_parity_both_metrics(gpu, oracle, box):
    """A zero radius, a repeated radius and a last radius far larger than a
    leaf; counts and totals together, totals alone and counts alone."""
    pts = uniform(20_000, 301)
    q = uniform(700, 302)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    ref = _brute(oracle, pts, q, RADII, box)
    c, tot = t.ball_hist(q, RADII)
    assert c.dtype == np.uint32 and c.shape == (700, len(RADII))
    assert tot.dtype == np.uint64 and tot.shape == (len(RADII),)
    for j in range(len(RADII)):
        assert np.array_equal(c[:, j], ref[:, j]), f"column {j} (r = {RADII[j]})"
    assert np.array_equal(tot, ref.sum(axis=0, dtype=np.uint64))
    c1, tot1 = t.ball_hist(q, RADII, counts=False)
    assert c1 is None and np.array_equal(tot1, tot)
    c2, tot2 = t.ball_hist(q, RADII, total=False)
    assert tot2 is None and np.array_equal(c2, c)


@pytest.mark.parametrize("box", [None, 1.0])
def test_threshold_ties(gpu, oracle, box):
    """The dyadic lattice i/16: thousands of pairs sit exactly on a threshold
    (d2 == t[j]), leaf boxes have ub == t[j] and lb == t[j]: `<=`, the
    whole-leaf rule and the no-threshold-splits shortcut must all agree with
    the brute force."""
    g = np.arange(16, dtype=np.float32) / np.float32(16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = np.concatenate([pts[::7], uniform(100, 303)])
    radii = np.array([1 / 16, np.sqrt(2) / 16, 2 / 16, 3 / 16], np.float32)
    thr = radii * radii
    # the case is what it claims to be: exact ties at radii 0, 2 and 3; the
    # f32 square of sqrt(2)/16 falls one step under 2/256, so radius 1 adds
    # nothing to radius 0
    d2 = d2_ref(q[:586, None, :], pts[None, :, :], box)
    ties = [int((d2 == tj).sum()) for tj in thr]
    assert ties == ([3516, 0, 3516, 17580] if box else [3294, 0, 3072, 12936])
    assert thr[1] < np.float32(2 / 256)
    ref = _brute(oracle, pts, q, radii, box)
    assert np.array_equal(ref[:586, 0], ref[:586, 1])
    for leaf in (16, 64):
        t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
        c, tot = t.ball_hist(q, radii)
        for j in range(len(radii)):
            assert np.array_equal(c[:, j], ref[:, j]), f"leafsize {leaf}, column {j}"
        assert np.array_equal(tot, ref.sum(axis=0, dtype=np.uint64))


@pytest.mark.parametrize("n", [1, 9, 63, 1003])
def test_padding_points_are_never_counted(gpu, oracle, n):
    """Tiny trees, padded to a multiple of 8 with FLT_MAX points; the last
    radius holds the whole box, so its column is n for every query."""
    pts = uniform(n, 304)
    q = uniform(130, 305)
    radii = np.array([0.05, 0.3, 2.0], np.float32)
    t = gpu.Tree(pts, leafsize=16)
    c, tot = t.ball_hist(q, radii)
    assert np.all(c[:, -1] == n)
    assert np.array_equal(c, _brute(oracle, pts, q, radii, None))
    assert np.array_equal(tot, c.sum(axis=0, dtype=np.uint64))


def test_two_staged_chunks_per_leaf(gpu, oracle):
    """leafsize 128: leaves of 65..128 points are staged as two chunks."""
    pts = uniform(5000, 306)
    q = uniform(300, 307)
    radii = np.array([0.02, 0.08, 0.2, 2.0], np.float32)
    for box in (None, 1.0):
        t = gpu.Tree(pts, leafsize=128, boxsize=box)
        c, tot = t.ball_hist(q, radii)
        assert np.array_equal(c, _brute(oracle, pts, q, radii, box))
        assert np.all(c[:, -1] == 5000)
        assert np.array_equal(tot, c.sum(axis=0, dtype=np.uint64))


def test_periodic_queries_outside_the_box(gpu, oracle):
    """Queries outside [0, L]^3 of a periodic tree take the brute-force kernel."""
    pts = uniform(20_000, 308)
    q = uniform(300, 309)
    q[[3, 50, 120, 200, 299]] += np.float32(1.5)
    q[[10, 77]] -= np.float32(0.3)
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    c, tot = t.ball_hist(q, RADII)
    ref = _brute(oracle, pts, q, RADII, 1.0)
    for j, r in enumerate(RADII):
        assert np.array_equal(c[:, j], ref[:, j]), f"column {j}"
        assert np.array_equal(c[:, j], t.ball_count(q, float(r))), f"column {j} vs ball_count"
    assert np.array_equal(tot, ref.sum(axis=0, dtype=np.uint64))
    _, tot1 = t.ball_hist(q, RADII, counts=False)
    assert np.array_equal(tot1, tot)


def test_streaming_accumulates_totals_over_batches(gpu):
    """host_batch = 256: 1000 host queries run as four batches; rows and the
    totals (accumulated on the device across the batches) equal the
    single-batch result."""
    pts = uniform(20_000, 310)
    q = uniform(1000, 311)
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    c0, tot0 = t.ball_hist(q, RADII)
    old = gpu.get_tuning("host_batch")
    try:
        gpu.set_tuning("host_batch", 256)
        c1, tot1 = t.ball_hist(q, RADII)
        _, tot2 = t.ball_hist(q, RADII, counts=False)
        c3, _ = t.ball_hist(q, RADII, total=False)
    finally:
        gpu.set_tuning("host_batch", old)
    assert np.array_equal(c1, c0) and np.array_equal(c3, c0)
    assert np.array_equal(tot1, tot0) and np.array_equal(tot2, tot0)
    assert np.array_equal(tot0, c0.sum(axis=0, dtype=np.uint64))


@pytest.mark.parametrize("box", [None, 1.0])
def test_device_in_and_out_and_the_trees_own_points(gpu, box):
    """A tree built from a device array, queried with that array (the self
    order), device rows: the host-array result for the same points."""
    from nbodyhpc_amd import hip
    pts = uniform(30_000, 312)
    dp = hip.DeviceArray.from_numpy(pts)
    t = gpu.Tree(n=len(pts), dev_ptr=dp.ptr, leafsize=64, boxsize=box)
    c_host, tot_host = t.ball_hist(pts, RADII)
    out = hip.DeviceArray((len(pts), len(RADII)), np.uint32)
    s = hip.Stream()
    gpu.timing_enable(True)
    try:
        gpu.timing_reset()
        tot = t.ball_hist_device(dp.ptr, len(pts), RADII, out.ptr, stream=s.handle)
        assert gpu.timing_read("self_order")[1] == 1
        assert gpu.timing_read("ball_hist")[1] == 1
    finally:
        gpu.timing_enable(False)
    assert np.array_equal(out.numpy(), c_host)
    assert np.array_equal(tot, tot_host)
    # totals only (no rows), and rows only (returns once enqueued)
    tot2 = t.ball_hist_device(dp.ptr, len(pts), RADII, None, stream=s.handle)
    assert np.array_equal(tot2, tot_host)
    out.zero()
    assert t.ball_hist_device(dp.ptr, len(pts), RADII, out.ptr, total=False,
                              stream=s.handle) is None
    s.synchronize()
    assert np.array_equal(out.numpy(), c_host)
    # a prefix of the build array
    m = 10_001
    tot3 = t.ball_hist_device(dp.ptr, m, RADII, out.ptr, stream=s.handle)
    assert np.array_equal(out.numpy()[:m], c_host[:m])
    assert np.array_equal(tot3, c_host[:m].sum(axis=0, dtype=np.uint64))


def test_number_of_radii_and_arguments(gpu):
    pts = uniform(2000, 313)
    q = uniform(200, 314)
    t = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    c, tot = t.ball_hist(q, [0.07])
    assert c.shape == (200, 1) and np.array_equal(c[:, 0], t.ball_count(q, 0.07))
    r32 = np.linspace(0.0, 0.6, 32).astype(np.float32)
    c, tot = t.ball_hist(q, r32)
    for j, r in enumerate(r32):
        assert np.array_equal(c[:, j], t.ball_count(q, float(r))), f"column {j}"
    assert np.array_equal(tot, c.sum(axis=0, dtype=np.uint64))
    bad = [
        (np.linspace(0.0, 0.6, 33), {}, "number of radii"),
        ([0.1, 0.2, 0.15], {}, "ascending"),
        ([0.1, float("nan")], {}, "NaN"),
        ([-0.1, 0.2], {}, "negative"),
        ([0.1, float("inf")], {}, "infinite"),
        ([0.1, 0.2], dict(counts=False, total=False), "both NULL"),
    ]
    for radii, kw, msg in bad:
        with pytest.raises(gpu.NbkdError, match=msg) as e:
            t.ball_hist(q, radii, **kw)
        assert e.value.status == gpu.NBKD_EINVAL
    # no queries: fine, totals zeroed
    c, tot = t.ball_hist(np.zeros((0, 3), np.float32), [0.1, 0.2])
    assert c.shape == (0, 2) and np.array_equal(tot, [0, 0])


def test_python_surface(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    pts = uniform(3000, 315)
    q = uniform(240, 316)
    r = np.array([0.02, 0.05, 0.1, 0.1, 0.2], np.float32)
    cap = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    c_ref, tot_ref = cap.ball_hist(q, r)
    t = KDTree(pts, leafsize=32, boxsize=1.0)
    tot = t.count_neighbors(q, r)
    assert tot.dtype == np.uint64 and np.array_equal(tot, tot_ref)
    assert t.count_neighbors(q, 0.05) == int(tot_ref[1])
    assert np.array_equal(t.count_neighbors(q, r, cumulative=False),
                          np.diff(tot_ref.astype(np.int64), prepend=0).astype(np.uint64))
    pp = t.count_neighbors(q, r, per_point=True)
    assert pp.dtype == np.uint32 and np.array_equal(pp, c_ref)
    assert np.array_equal(t.count_neighbors(q, r, cumulative=False, per_point=True),
                          np.diff(c_ref.astype(np.int64), axis=1, prepend=0).astype(np.uint32))
    nd = t.count_neighbors(q[:12].reshape(3, 4, 3), r, per_point=True)
    assert nd.shape == (3, 4, len(r)) and np.array_equal(nd.reshape(12, -1), c_ref[:12])
    one = t.count_neighbors(q[:12].reshape(3, 4, 3), 0.05, per_point=True)
    assert one.shape == (3, 4) and np.array_equal(one.reshape(-1), c_ref[:12, 1])
    assert np.array_equal(one, t.query_ball(q[:12].reshape(3, 4, 3), 0.05, return_length=True))
    for bad, msg in (([0.2, 0.1], "ascending"), ([], "empty"), (np.zeros(33), "at most 32"),
                     ([0.1, float("nan")], "finite")):
        with pytest.raises(ValueError, match=msg):
            t.count_neighbors(q, bad)
    # auto pair counts: unordered pairs i < j with d2 <= r^2 (periodic metric)
    thr = r * r
    want = np.zeros(len(r), np.uint64)
    for a in range(0, len(pts), 500):
        d2 = d2_ref(pts[a:a + 500, None, :], pts[None, :, :], 1.0)
        j = np.arange(len(pts))[None, :]
        i = np.arange(a, min(a + 500, len(pts)))[:, None]
        for k, tk in enumerate(thr):
            want[k] += np.uint64(((d2 <= tk) & (j > i)).sum())
    got = t.pair_counts(r)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert t.pair_counts(0.1) == int(want[2])
