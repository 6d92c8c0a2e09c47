"""Observer-frame pair counts (nbkd_query_ball_hist2_obs, the LOS == observer
instances of ball_hist2.hip): (rp, pi) and (s, mu) bins about the line from an
observer through each pair's midpoint.  The reference is the numpy float32 brute
force of tests/aniso_obs_ref.py, which applies the header's definitions
operation by operation; counts are integers, so every comparison is exact
equality.  New (no reference counterpart: the reference has no radius search)."""
import functools

import numpy as np
import pytest

from tests import aniso_obs_ref as ob
from tests import units
from tests.aniso_ref import RPPI, SMU
from tests.golden.inputs import uniform

pytestmark = pytest.mark.gpu

E1 = np.array([0.0, 0.01, 0.02, 0.05, 0.05, 0.11], np.float32)
PI = np.array([0.005, 0.02, 0.02, 0.3], np.float32)
MU = np.array([0.0, 0.25, 0.5, 0.5, 1.0], np.float32)
MODES = [(RPPI, PI), (SMU, MU)]
MODE_IDS = ["rppi", "smu"]
OUTSIDE = (0.5, 0.5, -2.0)
INSIDE = (0.5, 0.5, 0.5)


@functools.lru_cache(maxsize=None)
def parity_inputs():
    pts, q = uniform(6000, 401), uniform(1500, 402)
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


def observer(name):
    if name == "outside":
        return OUTSIDE
    if name == "inside":
        return INSIDE
    return tuple(float(x) for x in parity_inputs()[0][17])  # a tree point


@functools.lru_cache(maxsize=None)
def parity_ref(name, mode):
    pts, q = parity_inputs()
    ref = ob.hist2_obs_ref(pts, q, E1, MODES[mode][1], mode, observer(name))
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("mode, e2", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["outside", "inside", "on_a_point"])
def test_parity(gpu, name, mode, e2):
    """A zero edge, a repeated edge on both axes, a pi range three times the rp
    range; an observer outside the cube, inside it, and on a tree point."""
    pts, q = parity_inputs()
    ref = parity_ref(name, mode)
    assert ref.sum() > 10_000 and np.all(ref[4] == 0)
    for leaf in (16, 64):
        t = gpu.Tree(pts, leafsize=leaf)
        got = t.ball_hist2_obs(q, E1, e2, mode, observer(name))
        assert got.dtype == np.uint64 and got.shape == (len(E1), len(e2))
        assert np.array_equal(got, ref), f"leafsize {leaf}"


def test_the_line_of_sight_matters(gpu):
    """the observer-frame counts are not the fixed-axis ones (inside the cube
    the lines of sight point everywhere), and far away along z they approach
    them"""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32)
    fixed = t.ball_hist2(q, E1, PI, RPPI, 2)
    assert not np.array_equal(t.ball_hist2_obs(q, E1, PI, RPPI, INSIDE), fixed)
    far = t.ball_hist2_obs(q, E1, PI, RPPI, (0.5, 0.5, -1.0e4))
    assert far.sum() > 10_000
    assert np.abs(far.astype(np.int64) - fixed.astype(np.int64)).sum() < 0.01 * fixed.sum()


def test_smu_rows_sum_to_the_radius_histogram(gpu):
    """pi2 <= s2 by the clamp, so with a last mu edge of exactly 1 every pair
    inside s[-1] is counted: the sum over mu of row b1 is the first difference
    of nbkd_query_ball_hist's totals at the same edges."""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32)
    _, tot = t.ball_hist(q, E1, counts=False)
    want = np.diff(tot.astype(np.int64), prepend=0).astype(np.uint64)
    for o in (OUTSIDE, INSIDE, observer("on_a_point")):
        one = t.ball_hist2_obs(q, E1, [1.0], SMU, o)
        assert one.shape == (len(E1), 1) and np.array_equal(one[:, 0], want)
        assert np.array_equal(t.ball_hist2_obs(q, E1, MU, SMU, o).sum(axis=1), want)
    assert t.ball_hist2_obs(q, E1, [0.9], SMU, OUTSIDE).sum() < want.sum()


# the dyadic lattice arange(13) / 16 per axis about its centre: every
# coordinate, square and product below is exact, ties by the thousand
TIE_E1 = np.array([1 / 16, 2 / 16, 3 / 16, 1 / 4], np.float32)
TIE_PI = np.array([0.0, 1 / 16, 2 / 16, 3 / 16], np.float32)
TIE_MU = np.array([0.0, 0.5, np.sqrt(np.float32(0.5)), 1.0], np.float32)
TIE_O = (6 / 16, 6 / 16, 6 / 16)
# pairs exactly on each threshold (first axis, second axis) and the total count,
# from the brute force on the CPU
TIES = {
    RPPI: ([0, 10134, 0, 10806], [13629, 2616, 1404, 1644], 451989),
    SMU: ([12168, 11154, 44988, 9126], [13629, 2773, 2197, 3789], 394325),
}


@pytest.mark.parametrize("mode, e2", [(RPPI, TIE_PI), (SMU, TIE_MU)], ids=MODE_IDS)
def test_threshold_ties_and_mirror_pairs(gpu, mode, e2):
    """Self counts of the lattice with the observer at its centre: 2196 ordered
    pairs with s2 > 0 are mirror images about the observer (l2 == 0, pi2 = 0),
    thousands of pairs sit on rp2 == T1[k], s2 == T1[k], pi2 == T2[l] and pi2 ==
    fl(M[l] * s2), and leaf boxes have their bounds on thresholds."""
    g = np.arange(13, dtype=np.float32) / np.float32(16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    assert len(pts) == 2197
    first, second, mirror = ob.tie_counts_obs(pts, pts, TIE_E1, e2, mode, TIE_O)
    ref = ob.hist2_obs_ref(pts, pts, TIE_E1, e2, mode, TIE_O)
    assert mirror == 2196
    assert (first, second, int(ref.sum())) == TIES[mode]
    for leaf in (16, 64):
        got = gpu.Tree(pts, leafsize=leaf).ball_hist2_obs(pts, TIE_E1, e2, mode, TIE_O)
        assert np.array_equal(got, ref), f"leafsize {leaf}"
    auto = ref.copy()
    auto[0, 0] -= np.uint64(len(pts))
    assert np.all(auto % np.uint64(2) == 0)


def test_collinear_ray_fires_the_clamp(gpu):
    """Points on one ray from the observer: s is parallel to l for every pair,
    pi2 = s2 in exact arithmetic, and fl(x / l2) comes out above s2 for about a
    third of the pairs.  The clamp keeps pi2 <= s2 and rp2 >= 0 there."""
    tt = np.linspace(1.0, 4.0, 2000).astype(np.float32)
    pts = (tt[:, None] * np.array([0.3, 0.5, 0.7], np.float32)[None, :]).astype(np.float32)
    o = (0.0, 0.0, 0.0)
    fired = ob.clamp_count(pts, pts, o)
    print("pairs with fl(x / l2) > s2:", fired, "of", len(pts) ** 2)
    assert fired > 1_000_000
    t = gpu.Tree(pts, leafsize=32)
    s = np.array([0.0, 0.01, 0.1, 0.5, 1.0, 4.0], np.float32)
    for mode, e2 in ((RPPI, [0.0, 0.01, 0.1, 1.0, 4.0]), (SMU, [0.5, 0.999, 0.99999, 1.0])):
        ref = ob.hist2_obs_ref(pts, pts, s, e2, mode, o)
        assert ref.sum() > 1_000_000
        assert np.array_equal(t.ball_hist2_obs(pts, s, e2, mode, o), ref)


@pytest.mark.parametrize("n", [1, 9, 63, 1003])
def test_padding_points_are_in_no_bin(gpu, n):
    """Tiny trees, padded to a multiple of 8 with FLT_MAX points; the edges hold
    the whole box, so the grand total is m * n."""
    pts = uniform(n, 404)
    q = uniform(130, 405)
    t = gpu.Tree(pts, leafsize=16)
    s = np.array([0.05, 0.3, 2.0], np.float32)
    for o in (OUTSIDE, INSIDE):
        for mode, e2 in ((SMU, [0.3, 1.0]), (RPPI, [0.1, 2.0])):
            got = t.ball_hist2_obs(q, s, e2, mode, o)
            assert int(got.sum()) == 130 * n
            assert np.array_equal(got, ob.hist2_obs_ref(pts, q, s, e2, mode, o))


def test_two_staged_chunks_per_leaf(gpu):
    """leafsize 128: leaves of 65..128 points are staged as two chunks."""
    pts = uniform(5000, 406)
    q = uniform(300, 407)
    s = np.array([0.02, 0.08, 0.2, 2.0], np.float32)
    t = gpu.Tree(pts, leafsize=128)
    for mode, e2 in ((RPPI, [0.01, 0.1, 2.0]), (SMU, [0.2, 0.7, 1.0])):
        got = t.ball_hist2_obs(q, s, e2, mode, OUTSIDE)
        assert np.array_equal(got, ob.hist2_obs_ref(pts, q, s, e2, mode, OUTSIDE))
        assert int(got.sum()) == 300 * 5000


def test_all_points_coincident(gpu):
    """s2 == 0 for every pair of a query on the points: bin (0, 0) in both
    modes, also with the observer on the points (l2 == 0 as well)."""
    pts = np.full((700, 3), 0.375, np.float32)
    q = np.array([[0.375, 0.375, 0.375], [0.375, 0.375, 0.5], [0.9, 0.1, 0.2]], np.float32)
    t = gpu.Tree(pts, leafsize=16)
    e1 = [0.0, 0.125, 1.0]
    for o in (OUTSIDE, (0.375, 0.375, 0.375), (0.375, 0.375, 0.4375)):
        for mode, e2 in ((RPPI, [0.0, 0.125, 0.3]), (SMU, [0.0, 0.5, 1.0])):
            got = t.ball_hist2_obs(q, e1, e2, mode, o)
            assert np.array_equal(got, ob.hist2_obs_ref(pts, q, e1, e2, mode, o))
            assert got[0, 0] >= 700


def test_a_nan_or_far_query_is_in_no_bin(gpu):
    """a query with a NaN coordinate, and one so far away that every s2
    overflows, add nothing and leave the other queries' counts alone"""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32)
    bad = q[:200].copy()
    bad[5, 1] = np.nan
    bad[64] = np.nan
    bad[130] = np.float32(3e19)
    good = np.delete(q[:200], [5, 64, 130], axis=0)
    for mode, e2 in MODES:
        ref = ob.hist2_obs_ref(pts, good, E1, e2, mode, OUTSIDE)
        assert np.array_equal(t.ball_hist2_obs(bad, E1, e2, mode, OUTSIDE), ref)
        assert np.array_equal(t.ball_hist2_obs(good, E1, e2, mode, OUTSIDE), ref)


@pytest.mark.parametrize("m", [1, 63, 65])
def test_packet_edges(gpu, m):
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32)
    for mode, e2 in MODES:
        got = t.ball_hist2_obs(q[:m], E1, e2, mode, INSIDE)
        assert np.array_equal(got, ob.hist2_obs_ref(pts, q[:m], E1, e2, mode, INSIDE))


def test_streaming_accumulates_over_batches(gpu):
    """host_batch = 256: 1500 host queries run as six batches; the totals
    accumulate on the device across them."""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32)
    old = gpu.get_tuning("host_batch")
    try:
        gpu.set_tuning("host_batch", 256)
        got = [t.ball_hist2_obs(q, E1, e2, mode, OUTSIDE) for mode, e2 in MODES]
    finally:
        gpu.set_tuning("host_batch", old)
    for a, (mode, _) in zip(got, MODES):
        assert np.array_equal(a, parity_ref("outside", mode))


def test_self_order_path_equals_the_bucketed_path(gpu):
    """A tree built from a device array, queried with that array on a
    non-default stream (the self order): the host-array result."""
    from nbodyhpc_amd import hip
    pts = uniform(30_000, 410)
    dp = hip.DeviceArray.from_numpy(pts)
    t = gpu.Tree(n=len(pts), dev_ptr=dp.ptr, leafsize=64)
    s = hip.Stream()
    for mode, e2 in MODES:
        host = t.ball_hist2_obs(pts, E1, e2, mode, OUTSIDE)
        gpu.timing_enable(True)
        try:
            gpu.timing_reset()
            dev = t.ball_hist2_obs_device(dp.ptr, len(pts), E1, e2, mode, OUTSIDE,
                                          stream=s.handle)
            assert gpu.timing_read("self_order")[1] == 1
            assert gpu.timing_read("ball_hist2_obs")[1] == 1
            assert gpu.timing_read("ball_hist2")[1] == 0
        finally:
            gpu.timing_enable(False)
        assert np.array_equal(dev, host)
        # every bin of an auto count is even once the self pairs leave (0, 0)
        auto = dev.copy()
        auto[0, 0] -= np.uint64(len(pts))
        assert np.all(auto % np.uint64(2) == 0)
        # a prefix of the build array
        m = 10_001
        assert np.array_equal(
            t.ball_hist2_obs_device(dp.ptr, m, E1, e2, mode, OUTSIDE, stream=s.handle),
            t.ball_hist2_obs(pts[:m], E1, e2, mode, OUTSIDE))


def test_flush_interval_and_copies_do_not_change_the_result(gpu):
    """hist2_flush_visits = 1 flushes the wave's histogram after every leaf
    visit, 3 after every third; hist2_copies picks the interleaved copies."""
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=16)
    for knob, values in (("hist2_flush_visits", (1, 3)), ("hist2_copies", (1, 4))):
        old = gpu.get_tuning(knob)
        assert old == 0
        try:
            for v in values:
                gpu.set_tuning(knob, v)
                for mode, e2 in MODES:
                    assert np.array_equal(t.ball_hist2_obs(q, E1, e2, mode, OUTSIDE),
                                          parity_ref("outside", mode)), (knob, v)
        finally:
            gpu.set_tuning(knob, old)
        assert gpu.get_tuning(knob) == 0


def test_bin_count_extremes(gpu):
    """32 x 64 bins (one copy of the histogram fills the wave's 8 KiB) and 1 x 1."""
    pts = uniform(2000, 411)
    q = uniform(200, 412)
    t = gpu.Tree(pts, leafsize=16)
    e32 = np.linspace(0.0, 0.45, 32).astype(np.float32)
    pi64 = np.linspace(0.0, 0.5, 64).astype(np.float32)
    mu64 = np.linspace(0.0, 1.0, 64).astype(np.float32)
    for mode, e2 in ((RPPI, pi64), (SMU, mu64)):
        got = t.ball_hist2_obs(q, e32, e2, mode, OUTSIDE)
        assert got.shape == (32, 64)
        assert np.array_equal(got, ob.hist2_obs_ref(pts, q, e32, e2, mode, OUTSIDE))
        one = t.ball_hist2_obs(q, [0.2], e2[-1:], mode, OUTSIDE)
        assert one.shape == (1, 1)
        assert np.array_equal(one, ob.hist2_obs_ref(pts, q, [0.2], e2[-1:], mode, OUTSIDE))
    with pytest.raises(gpu.NbkdError, match="got 65") as e:
        t.ball_hist2_obs(q, e32, np.linspace(0, 1, 65), SMU, OUTSIDE)
    assert e.value.status == gpu.NBKD_EINVAL
    assert np.array_equal(t.ball_hist2_obs(np.zeros((0, 3), np.float32), [0.1], [0.5, 1.0], SMU,
                                           OUTSIDE), [[0, 0]])


def test_a_periodic_tree_is_rejected(gpu):
    pts, q = parity_inputs()
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    out_before = t.ball_hist2(q[:10], E1, MU, SMU, 2)
    with pytest.raises(gpu.NbkdError, match="non-periodic trees only") as e:
        t.ball_hist2_obs(q, E1, MU, SMU, OUTSIDE)
    assert e.value.status == gpu.NBKD_EINVAL
    assert str(e.value).startswith("nbkd_query_ball_hist2_obs:")
    assert "nbkd_query_ball_hist2 " in str(e.value)
    # no queries: NBKD_OK before the handle is read, as the header says
    assert np.array_equal(t.ball_hist2_obs(np.zeros((0, 3), np.float32), [0.1], [1.0], SMU,
                                           OUTSIDE), [[0]])
    assert np.array_equal(t.ball_hist2(q[:10], E1, MU, SMU, 2), out_before)


def test_auto_counts_and_the_wrapper(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    pts = uniform(3000, 413)
    t = KDTree(pts, leafsize=32)
    s = np.array([0.02, 0.05, 0.1, 0.1, 0.2], np.float32)
    mu = np.array([0.2, 0.5, 0.5, 0.8, 1.0], np.float32)
    pi = np.array([0.01, 0.05, 0.3], np.float32)
    for o in (OUTSIDE, INSIDE):
        for ordered, e2, mode in ((t.count_pairs_smu(pts, s, mu, observer=o), mu, SMU),
                                  (t.count_pairs_rppi(pts, s, pi, observer=o), pi, RPPI)):
            assert ordered.dtype == np.uint64 and ordered.shape == (5, len(e2))
            assert np.array_equal(ordered, ob.hist2_obs_ref(pts, pts, s, e2, mode, o))
            # (i, j) and (j, i) share a bin: every bin without the self pairs is even
            ordered[0, 0] -= np.uint64(3000)
            assert np.all(ordered % np.uint64(2) == 0)
        auto = t.pair_counts_smu(s, mu, observer=o)
        assert auto.dtype == np.uint64
        assert np.array_equal(auto.sum(axis=1),
                              np.diff(t.pair_counts(s).astype(np.int64), prepend=0))
        assert np.array_equal(t.pair_counts_rppi(s, pi, observer=o) * np.uint64(2), ordered)
    # observer=None is the fixed axis, as before
    assert np.array_equal(t.count_pairs_rppi(pts, s, pi, 1, observer=None),
                          t.count_pairs_rppi(pts, s, pi, 1))
    # N-D queries are flattened; array-likes of any float type are observers
    nd = t.count_pairs_smu(pts[:12].reshape(3, 4, 3), s, mu, observer=np.array(OUTSIDE))
    assert np.array_equal(nd, t.count_pairs_smu(pts[:12], s, mu, observer=list(OUTSIDE)))
    with pytest.raises(ValueError, match="not both"):
        t.count_pairs_rppi(pts, s, pi, 0, observer=OUTSIDE)
    p = KDTree(pts, leafsize=32, boxsize=1.0)
    with pytest.raises(ValueError, match="non-periodic"):
        p.count_pairs_smu(pts, s, mu, observer=OUTSIDE)


FRAMES = ("L205000", "L67.77", "s+40", "s-20", "off1000", "centred17")
E1_FRACTIONS = (0.0, 0.01, 0.03, 0.07, 0.07, 0.15)
PI_FRACTIONS = (0.004, 0.05, 0.05, 0.35)
FRAME_MU = np.array([0.0, 0.3, 0.6, 0.6, 1.0], np.float32)


@pytest.mark.parametrize("mode", [RPPI, SMU], ids=MODE_IDS)
@pytest.mark.parametrize("name", FRAMES)
def test_parity_in_the_frame(gpu, name, mode):
    """The frames of tests/units.py as non-periodic point sets, the observer
    scaled and shifted with them, edges as fractions of the frame's scale: the
    brute force in that frame.  (At scale 2^40 fl(dot * dot) overflows for most
    pairs, |s| |l| being above 2^64: the quotient is infinite, the clamp gives
    pi2 = s2, and the kernel must do exactly that too.)"""
    pts, q = units.inputs(name, 3000, 600)
    f = units.FRAMES[name]
    e1 = np.array([units.length(name, x) for x in E1_FRACTIONS], np.float32)
    e2 = FRAME_MU if mode == SMU else np.array([units.length(name, x) for x in PI_FRACTIONS],
                                               np.float32)
    t = gpu.Tree(pts, leafsize=32)
    for base in (OUTSIDE, INSIDE):
        o = (f.a * np.array(base, np.float64) + f.c).astype(np.float32)
        ref = ob.hist2_obs_ref(pts, q, e1, e2, mode, o)
        assert ref.sum() > 2000 and ref[0, 0] >= 200  # the self rows sit in bin (0, 0)
        assert np.array_equal(t.ball_hist2_obs(q, e1, e2, mode, o), ref), base


def test_landy_szalay_estimators_are_composed_of_the_counts(gpu):
    """xi_rppi_ls / xi_smu_ls on 3000 data and 6000 random points equal
    landy_szalay of the count methods' tables exactly, with an observer and
    with a fixed axis."""
    from nbodyhpc_amd.kdtree import KDTree, landy_szalay
    data, rand = uniform(3000, 414), uniform(6000, 415)
    t, r = KDTree(data, leafsize=32), KDTree(rand, leafsize=32)
    rp = np.array([0.01, 0.02, 0.04, 0.08], np.float32)
    npi, pi_max, nmu = 5, 0.1, 4
    pe = (pi_max * (np.arange(npi) + 1.0) / npi).astype(np.float32)
    me = ((np.arange(nmu) + 1.0) / nmu).astype(np.float32)
    for kw in (dict(observer=OUTSIDE), dict(los=1), dict()):
        dd = t.count_pairs_rppi(data, rp, pe, **kw)[1:]
        dr = r.count_pairs_rppi(data, rp, pe, **kw)[1:]
        rr = r.count_pairs_rppi(rand, rp, pe, **kw)[1:]
        want = landy_szalay(dd, dr, rr, 3000, 6000)
        xi, wp = t.xi_rppi_ls(r, rp, pi_max, npi, **kw)
        assert xi.shape == (3, npi) and np.array_equal(xi, want, equal_nan=True)
        assert np.all(rr > 0) and np.all(np.abs(xi) < 1.0)  # uniform points: noise
        dp = np.diff(np.concatenate([[0.0], pe.astype(np.float64)]))
        assert np.array_equal(wp, 2.0 * (want * dp[None, :]).sum(axis=1))
        dd = t.count_pairs_smu(data, rp, me, **kw)[1:]
        dr = r.count_pairs_smu(data, rp, me, **kw)[1:]
        rr = r.count_pairs_smu(rand, rp, me, **kw)[1:]
        want = landy_szalay(dd, dr, rr, 3000, 6000)
        xs, poles = t.xi_smu_ls(r, rp, nmu, **kw)
        assert np.array_equal(xs, want, equal_nan=True)
        assert sorted(poles) == [0, 2, 4] and np.allclose(poles[0], want.mean(axis=1), rtol=1e-12)
    # the observer changes the table
    assert not np.array_equal(t.xi_rppi_ls(r, rp, pi_max, npi, observer=INSIDE)[0],
                              t.xi_rppi_ls(r, rp, pi_max, npi)[0])
