"""Anisotropic pair counts (nbkd_query_ball_hist2, ball_hist2.hip): (rp, pi) and
(s, mu) bins about a line of sight, one tree walk.  The reference is the numpy
brute force of tests/aniso_ref.py, which applies the header's definitions with
float32 scalars; counts are integers, so every comparison is exact equality.
New (no reference counterpart: the reference has no radius search)."""
import functools
import math

import numpy as np
import pytest

from tests import aniso_ref as ar
from tests.golden.inputs import uniform

pytestmark = pytest.mark.gpu

E1 = np.array([0.0, 0.01, 0.02, 0.05, 0.05, 0.11], np.float32)
PI = np.array([0.005, 0.02, 0.02, 0.3], np.float32)
MU = np.array([0.0, 0.25, 0.5, 0.5, 1.0], np.float32)
MODES = [(ar.RPPI, PI), (ar.SMU, MU)]
MODE_IDS = ["rppi", "smu"]


@functools.lru_cache(maxsize=None)
def parity_inputs():
    pts, q = uniform(6000, 401), uniform(1500, 402)
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


@pytest.mark.parametrize("los", [0, 1, 2])
@pytest.mark.parametrize("mode, e2", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("box", [None, 1.0])
def test_parity(gpu, box, mode, e2, los):
    """A zero edge, a repeated edge on both axes, a pi range three times the rp
    range (the elongated cylinder), both metrics, every line of sight."""
    pts, q = parity_inputs()
    ref = ar.hist2_ref(pts, q, E1, e2, mode, los, box)
    assert ref.sum() > 10_000 and np.all(ref[4] == 0)
    for leaf in (16, 64):
        t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
        got = t.ball_hist2(q, E1, e2, mode, los)
        assert got.dtype == np.uint64 and got.shape == (len(E1), len(e2))
        assert np.array_equal(got, ref), f"leafsize {leaf}"


@pytest.mark.parametrize("box", [None, 1.0])
def test_smu_rows_sum_to_the_radius_histogram(gpu, box):
    """pi2 <= s2 always, so with a last mu edge of exactly 1 every pair inside
    s[-1] is counted: the sum over mu of row b1 is the first difference of
    nbkd_query_ball_hist's totals at the same edges, for nmu = 1 and nmu = 5."""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    _, tot = t.ball_hist(q, E1, counts=False)
    want = np.diff(tot.astype(np.int64), prepend=0).astype(np.uint64)
    for los in (0, 1, 2):
        one = t.ball_hist2(q, E1, [1.0], ar.SMU, los)
        assert one.shape == (len(E1), 1) and np.array_equal(one[:, 0], want)
        five = t.ball_hist2(q, E1, MU, ar.SMU, los)
        assert np.array_equal(five.sum(axis=1), want)
    # the last mu edge below 1 loses pairs
    assert t.ball_hist2(q, E1, [0.9], ar.SMU, 2).sum() < want.sum()


@pytest.mark.parametrize("box", [None, 1.0])
def test_one_pi_edge_of_two_box_lengths_is_a_cylinder_count(gpu, box):
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    for los in (0, 1, 2):
        got = t.ball_hist2(q, E1, [2.0], ar.RPPI, los)
        u, v = [x for x in range(3) if x != los]
        want = np.zeros(len(E1) + 1, np.int64)
        for i in range(0, len(q), 500):
            a = ar.axes_ref(q[i:i + 500, None, :], pts[None, :, :], box)
            rp2 = a[..., u] + a[..., v]
            want += np.bincount(np.searchsorted(ar.thresholds(E1), rp2.reshape(-1), "left"),
                                minlength=len(E1) + 1)
        assert np.array_equal(got[:, 0], want[:-1].astype(np.uint64)), f"los {los}"


# the dyadic lattice i/16 of test_gpu_ball_hist.py::test_threshold_ties
TIE_E1 = np.array([1 / 16, 2 / 16, 3 / 16], np.float32)
TIE_PI = np.array([1 / 16, 2 / 16], np.float32)
# mu = 0.5 (M = 1/4) ties only at s2 == 0 on this lattice: pi2 == M * s2 exactly
# needs a^2 (i^2 + j^2) == (4^b - a^2) k^2 for mu = a / 2^b, and 4^b - a^2 = 3
# (mod 4) times squares is never a sum of two squares.  The edges fl(sqrt(1/6))
# and fl(sqrt(2/3)) tie through the rounded product instead: M = fl(1/6) and
# fl(M * 6 k^2/256) == k^2/256 (offsets (1, 2, 1)/16 and their like), M = fl(2/3)
# with offsets (1, 1, 2)/16.
TIE_MU = np.array([0.0, 0.4082483, 0.5, 0.8164966, 1.0], np.float32)
# pairs of the 586 lattice queries exactly on each threshold, from the brute
# force on the CPU (the same for every line of sight: the query set i = 0 mod 7
# is invariant under cyclic permutations of the axes)
TIES = {
    (None, ar.RPPI): ([35136, 32768, 30464], [27040, 25232]),
    (None, ar.SMU): ([3294, 3072, 12936], [14424, 7786, 586, 4186, 3660]),
    (1.0, ar.RPPI): ([37504, 37504, 37504], [33988, 33988]),
    (1.0, ar.SMU): ([3516, 3516, 17580], [16994, 9962, 586, 5274, 4102]),
}


@pytest.mark.parametrize("mode, e2", [(ar.RPPI, TIE_PI), (ar.SMU, TIE_MU)], ids=MODE_IDS)
@pytest.mark.parametrize("box", [None, 1.0])
def test_threshold_ties(gpu, box, mode, e2):
    """Thousands of pairs with rp2 == T1[k], pi2 == T2[l] and pi2 ==
    fl(M[l] * s2); leaf boxes whose bounds sit on thresholds: `<=`, the leaf
    pruning and the whole-leaf shortcut must agree with the brute force, for
    every line of sight (los 0 and 1 walk with the widened bound)."""
    g = np.arange(16, dtype=np.float32) / np.float32(16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = np.concatenate([pts[::7], uniform(100, 403)])
    assert TIE_MU[1] * TIE_MU[1] == np.float32(1 / 6) and TIE_MU[3] * TIE_MU[3] == np.float32(2 / 3)
    refs = {}
    for los in (0, 1, 2):
        first, second = ar.tie_counts(pts, q[:586], TIE_E1, e2, mode, los, box)
        assert (first, second) == TIES[(box, mode)], f"los {los}"
        assert min(first) > 0 and min(second) > 0
        if mode == ar.SMU:  # beyond the 586 coincident pairs that tie at every mu
            assert second[1] > 586 and second[3] > 586 and second[2] == 586
        refs[los] = ar.hist2_ref(pts, q, TIE_E1, e2, mode, los, box)
    for leaf in (16, 64):
        t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
        for los in (0, 1, 2):
            got = t.ball_hist2(q, TIE_E1, e2, mode, los)
            assert np.array_equal(got, refs[los]), f"leafsize {leaf}, los {los}"


@pytest.mark.parametrize("n", [1, 9, 63, 1003])
def test_padding_points_are_in_no_bin(gpu, n):
    """Tiny trees, padded to a multiple of 8 with FLT_MAX points; the edges hold
    the whole box, so the grand total is m * n in (s, mu) mode."""
    pts = uniform(n, 404)
    q = uniform(130, 405)
    t = gpu.Tree(pts, leafsize=16)
    s = np.array([0.05, 0.3, 2.0], np.float32)
    for los in (0, 2):
        got = t.ball_hist2(q, s, [0.3, 1.0], ar.SMU, los)
        assert int(got.sum()) == 130 * n
        assert np.array_equal(got, ar.hist2_ref(pts, q, s, [0.3, 1.0], ar.SMU, los))
        got = t.ball_hist2(q, s, [0.1, 2.0], ar.RPPI, los)
        assert int(got.sum()) == 130 * n
        assert np.array_equal(got, ar.hist2_ref(pts, q, s, [0.1, 2.0], ar.RPPI, los))


def test_two_staged_chunks_per_leaf(gpu):
    """leafsize 128: leaves of 65..128 points are staged as two chunks."""
    pts = uniform(5000, 406)
    q = uniform(300, 407)
    s = np.array([0.02, 0.08, 0.2, 2.0], np.float32)
    for box in (None, 1.0):
        t = gpu.Tree(pts, leafsize=128, boxsize=box)
        for mode, e2 in ((ar.RPPI, [0.01, 0.1, 2.0]), (ar.SMU, [0.2, 0.7, 1.0])):
            got = t.ball_hist2(q, s, e2, mode, 1)
            assert np.array_equal(got, ar.hist2_ref(pts, q, s, e2, mode, 1, box))
            assert int(got.sum()) == 300 * 5000


@pytest.mark.parametrize("box", [None, 1.0])
def test_all_points_coincident(gpu, box):
    """s2 == 0 for every pair of a query on the points: bin (0, 0) in both
    modes; a query elsewhere sees all of them in one bin."""
    pts = np.full((700, 3), 0.375, np.float32)
    q = np.array([[0.375, 0.375, 0.375], [0.375, 0.375, 0.5], [0.9, 0.1, 0.2]], np.float32)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for mode, e2 in ((ar.RPPI, [0.0, 0.125, 0.3]), (ar.SMU, [0.0, 0.5, 1.0])):
        for los in (0, 1, 2):
            e1 = [0.0, 0.125, 1.0]
            got = t.ball_hist2(q, e1, e2, mode, los)
            assert np.array_equal(got, ar.hist2_ref(pts, q, e1, e2, mode, los, box))
            assert got[0, 0] >= 700


def test_periodic_queries_outside_the_box(gpu):
    """Queries outside [0, L]^3 of a periodic tree take the brute-force kernel
    and count into the same totals."""
    pts = uniform(6000, 408)
    q = uniform(300, 409)
    q[[3, 50, 120, 200, 299]] += np.float32(1.5)
    q[[10, 77]] -= np.float32(0.3)
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    for mode, e2 in MODES:
        for los in (0, 2):
            got = t.ball_hist2(q, E1, e2, mode, los)
            assert np.array_equal(got, ar.hist2_ref(pts, q, E1, e2, mode, los, 1.0))
    # only outside queries
    got = t.ball_hist2(q[[3, 10]], E1, MU, ar.SMU, 1)
    assert np.array_equal(got, ar.hist2_ref(pts, q[[3, 10]], E1, MU, ar.SMU, 1, 1.0))


@pytest.mark.parametrize("m", [1, 63, 65])
def test_packet_edges(gpu, m):
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    for mode, e2 in MODES:
        got = t.ball_hist2(q[:m], E1, e2, mode, 0)
        assert np.array_equal(got, ar.hist2_ref(pts, q[:m], E1, e2, mode, 0, 1.0))


def test_streaming_accumulates_over_batches(gpu):
    """host_batch = 256: 1500 host queries run as six batches; the totals
    accumulate on the device across them."""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    ref = [t.ball_hist2(q, E1, e2, mode, 2) for mode, e2 in MODES]
    old = gpu.get_tuning("host_batch")
    try:
        gpu.set_tuning("host_batch", 256)
        got = [t.ball_hist2(q, E1, e2, mode, 2) for mode, e2 in MODES]
    finally:
        gpu.set_tuning("host_batch", old)
    for a, b, (mode, e2) in zip(got, ref, MODES):
        assert np.array_equal(a, b)
        assert np.array_equal(a, ar.hist2_ref(pts, q, E1, e2, mode, 2, 1.0))


@pytest.mark.parametrize("box", [None, 1.0])
def test_self_order_path_equals_the_bucketed_path(gpu, box):
    """A tree built from a device array, queried with that array on a
    non-default stream (the self order): the host-array result."""
    from nbodyhpc_amd import hip
    pts = uniform(30_000, 410)
    dp = hip.DeviceArray.from_numpy(pts)
    t = gpu.Tree(n=len(pts), dev_ptr=dp.ptr, leafsize=64, boxsize=box)
    s = hip.Stream()
    for mode, e2 in MODES:
        host = t.ball_hist2(pts, E1, e2, mode, 1)
        gpu.timing_enable(True)
        try:
            gpu.timing_reset()
            dev = t.ball_hist2_device(dp.ptr, len(pts), E1, e2, mode, 1, stream=s.handle)
            assert gpu.timing_read("self_order")[1] == 1
            assert gpu.timing_read("ball_hist2")[1] == 1
        finally:
            gpu.timing_enable(False)
        assert np.array_equal(dev, host)
        # a prefix of the build array
        m = 10_001
        assert np.array_equal(t.ball_hist2_device(dp.ptr, m, E1, e2, mode, 1, stream=s.handle),
                              t.ball_hist2(pts[:m], E1, e2, mode, 1))


def test_flush_interval_and_copies_do_not_change_the_result(gpu):
    """hist2_flush_visits = 1 flushes the wave's histogram after every leaf
    visit, 3 after every third; hist2_copies picks the interleaved copies."""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    ref = [t.ball_hist2(q, E1, e2, mode, 0) for mode, e2 in MODES]
    assert np.array_equal(ref[0], ar.hist2_ref(pts, q, E1, PI, ar.RPPI, 0, 1.0))
    for knob, values in (("hist2_flush_visits", (1, 3)), ("hist2_copies", (1, 2, 64))):
        old = gpu.get_tuning(knob)
        assert old == 0
        try:
            for v in values:
                gpu.set_tuning(knob, v)
                for want, (mode, e2) in zip(ref, MODES):
                    assert np.array_equal(t.ball_hist2(q, E1, e2, mode, 0), want), (knob, v)
        finally:
            gpu.set_tuning(knob, old)
        assert gpu.get_tuning(knob) == 0


def test_bin_count_extremes(gpu):
    """32 x 64 bins (one copy of the histogram fills the wave's 8 KiB) and 1 x 1."""
    pts = uniform(2000, 411)
    q = uniform(200, 412)
    t = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    e32 = np.linspace(0.0, 0.45, 32).astype(np.float32)
    pi64 = np.linspace(0.0, 0.5, 64).astype(np.float32)
    mu64 = np.linspace(0.0, 1.0, 64).astype(np.float32)
    for mode, e2 in ((ar.RPPI, pi64), (ar.SMU, mu64)):
        got = t.ball_hist2(q, e32, e2, mode, 2)
        assert got.shape == (32, 64)
        assert np.array_equal(got, ar.hist2_ref(pts, q, e32, e2, mode, 2, 1.0))
        one = t.ball_hist2(q, [0.2], e2[-1:], mode, 2)
        assert one.shape == (1, 1)
        assert np.array_equal(one, ar.hist2_ref(pts, q, [0.2], e2[-1:], mode, 2, 1.0))
    with pytest.raises(gpu.NbkdError, match="got 65") as e:
        t.ball_hist2(q, e32, np.linspace(0, 1, 65), ar.SMU, 2)
    assert e.value.status == gpu.NBKD_EINVAL
    assert np.array_equal(t.ball_hist2(np.zeros((0, 3), np.float32), [0.1], [0.5, 1.0], ar.SMU),
                          [[0, 0]])


def test_auto_counts(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    pts = uniform(3000, 413)
    t = KDTree(pts, leafsize=32, boxsize=1.0)
    s = np.array([0.02, 0.05, 0.1, 0.1, 0.2], np.float32)
    mu = np.array([0.2, 0.5, 0.5, 0.8, 1.0], np.float32)
    pi = np.array([0.01, 0.05, 0.3], np.float32)
    for los in (0, 2):
        for ordered, e2, mode in ((t.count_pairs_smu(pts, s, mu, los), mu, ar.SMU),
                                  (t.count_pairs_rppi(pts, s, pi, los), pi, ar.RPPI)):
            assert ordered.dtype == np.uint64 and ordered.shape == (5, len(e2))
            assert np.array_equal(ordered, ar.hist2_ref(pts, pts, s, e2, mode, los, 1.0))
            # the metric is symmetric: every ordered bin without the self pairs is even
            ordered[0, 0] -= np.uint64(3000)
            assert np.all(ordered % np.uint64(2) == 0)
        auto = t.pair_counts_smu(s, mu, los)
        assert auto.dtype == np.uint64
        # (pair_counts is cumulative and has the self pairs removed once)
        assert np.array_equal(auto.sum(axis=1),
                              np.diff(t.pair_counts(s).astype(np.int64), prepend=0))
        assert np.array_equal(t.pair_counts_rppi(s, pi, los) * np.uint64(2), ordered)
    # N-D queries are flattened
    nd = t.count_pairs_smu(pts[:12].reshape(3, 4, 3), s, mu)
    assert np.array_equal(nd, t.count_pairs_smu(pts[:12], s, mu))
    with pytest.raises(ValueError, match="ascending"):
        t.count_pairs_rppi(pts, [0.2, 0.1], pi)


def test_xi_of_uniform_points_is_noise(gpu):
    """xi_rppi on 20 000 uniform periodic points: |xi| sqrt(RR_unordered) <= 5
    in every bin with RR_unordered >= 100 (Poisson noise; the brute force on the
    CPU gives at most 2.16 for this seed, with RR_unordered >= 3769)."""
    from nbodyhpc_amd.kdtree import KDTree
    n = 20_000
    t = KDTree(uniform(n, 331), leafsize=64, boxsize=1.0)
    rp = np.array([0.01, 0.02, 0.03, 0.04, 0.05], np.float32)
    xi, wp = t.xi_rppi(rp, 0.05, 5)
    assert xi.shape == (4, 5) and wp.shape == (4,)
    r = rp.astype(np.float64)
    pe = np.concatenate([[0.0], (0.05 * (np.arange(5) + 1.0) / 5).astype(np.float32)])
    rr = n * n * math.pi * (r[1:] ** 2 - r[:-1] ** 2)[:, None] * 2 * np.diff(pe)[None, :] / 2
    assert np.all(rr >= 100)
    z = np.abs(xi) * np.sqrt(rr)
    print("max |xi| sqrt(RR):", z.max())
    assert np.all(z <= 5)
    assert np.allclose(wp, 2 * (xi * np.diff(pe)[None, :]).sum(axis=1), rtol=1e-12, atol=0)
    xs, poles = t.xi_smu(rp, 4)
    rr_s = n * n * (4 * math.pi / 3) * (r[1:] ** 3 - r[:-1] ** 3)[:, None] * 0.25 / 2
    print("max |xi(s, mu)| sqrt(RR):", (np.abs(xs) * np.sqrt(rr_s)).max())
    assert np.all(np.abs(xs) * np.sqrt(rr_s) <= 5)
    assert sorted(poles) == [0, 2, 4] and np.allclose(poles[0], xs.mean(axis=1), rtol=1e-12)
