"""Kernel-weighted sums over per-query balls (nbkd_query_ball_sum,
ball_sum.hip): out_sum[i, c] = sum_j values[j, c] * K(d_ij / h_i) over the
points with d2(i, j) <= fl(h_i * h_i) in the tree's f32 metric.  The brute
force is plain numpy: membership from tests.parity.d2_ref against the f32
product h_i * h_i, terms and sums in float64 with u = min(sqrt(d2) / h_i, 1) in
float64.  New (no reference counterpart)."""
import functools

import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import d2_ref

pytestmark = pytest.mark.gpu

TOPHAT, CUBIC, WENDLAND = 0, 1, 2
U24 = 2.0 ** -24


def kern64(u, kernel):
    if kernel == TOPHAT:
        return np.ones_like(u)
    if kernel == CUBIC:
        return np.where(u <= 0.5, 1 - 6 * u ** 2 + 6 * u ** 3, 2 * (1 - u) ** 3)
    return (1 - u) ** 4 * (1 + 4 * u)


def kern32(u, kernel):
    """K in float32, in the order nbkd.h states (numpy rounds every step)."""
    one, two, four, six = (np.float32(v) for v in (1, 2, 4, 6))
    u = np.asarray(u, np.float32)
    if kernel == TOPHAT:
        return np.ones_like(u)
    w = one - u
    if kernel == CUBIC:
        uu = u * u
        return np.where(u <= np.float32(0.5), (one - six * uu) + six * (uu * u),
                        two * ((w * w) * w))
    w2 = w * w
    return (w2 * w2) * (one + four * u)


def members(pts, q, h, box):
    """(m, n) membership and the f32 d2; a NaN, infinite or negative h: empty"""
    h = np.asarray(h, np.float32)
    d2 = np.empty((len(q), len(pts)), np.float32)
    for a in range(0, len(q), 500):
        d2[a:a + 500] = d2_ref(q[a:a + 500, None, :], pts[None, :, :], box)
    ok = np.isfinite(h) & (h >= 0)
    with np.errstate(invalid="ignore", over="ignore"):
        thr = np.where(ok, h * h, np.float32(-1))
    return (d2 <= thr[:, None]) & ok[:, None], d2


def brute(pts, q, h, box, values, kernel):
    """count (m,), float64 sums, sums of |term| and sums of |value| (m, nv)"""
    mem, d2 = members(pts, q, h, box)
    h64 = np.asarray(h, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.minimum(np.sqrt(d2.astype(np.float64)) / h64[:, None], 1.0)
    u = np.where(mem, np.nan_to_num(u, nan=0.0), 1.0)  # h = 0: coincident points, u = 0
    k = np.where(mem, kern64(u, kernel), 0.0)
    v = np.ones((len(pts), 1)) if values is None else np.asarray(values, np.float64).reshape(len(pts), -1)
    return (mem.sum(axis=1).astype(np.uint32), k @ v, np.abs(k) @ np.abs(v),
            mem.astype(np.float64) @ np.abs(v))


def assert_within_bound(got, cnt, s64, sabs, vabs, what=""):
    """|got - ref64| <= 2^-24 [(c_i + 1) sum_j |t_j| + 16 sum_j |v_j|].

    The first part is the f32 summation of c_i terms in any order (each of the
    c_i - 1 additions rounds once, relative to a partial sum that is at most
    sum |t_j|), with one unit to spare.  The second part is the error of the
    terms themselves, per unit of |v_j|: u = fl(fl(sqrt(d2)) * fl(1 / h)) carries
    <= 3 roundings, amplified by |K'| <= 2.1 (<= 6.3 units); the polynomial
    takes <= 6 more roundings at magnitudes <= 1.5 (<= 9 units); the product
    v * K rounds once (1 unit): 16.3, taken as 16.  An f32 emulation in numpy
    over random summation orders reached 0.09 of the bound, the GPU 0.23."""
    got = np.asarray(got, np.float64).reshape(s64.shape)
    bound = U24 * ((cnt[:, None].astype(np.float64) + 1) * sabs + 16 * vabs)
    err = np.abs(got - s64)
    ratio = np.max(err / np.where(bound > 0, bound, 1.0))
    print(f"{what}: worst error {ratio:.3f} of the bound")
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"{what}: {len(bad)} sums outside the bound, first {bad[:3]}"


# ---------------------------------------------------------------- shared inputs
N1, M1 = 6000, 1500
S1 = N1 ** (-1.0 / 3.0)
ZERO_ROWS = slice(0, 8)       # h = 0 at queries that coincide with a point
WIDE_ROWS = slice(8, 12)      # h = 0.6 L: wider than half the box
BAD_ROWS = slice(12, 18)      # NaN, -1, inf: empty balls


@functools.lru_cache(maxsize=None)
def inputs1():
    pts = uniform(N1, 401)
    q = uniform(M1, 411).copy()
    rng = np.random.default_rng(412)
    h = (rng.random(M1) * 3 * S1).astype(np.float32)
    q[ZERO_ROWS] = pts[100:108]
    h[ZERO_ROWS] = 0.0
    h[WIDE_ROWS] = 0.6
    h[BAD_ROWS] = [np.nan, -1.0, np.inf, -np.inf, -0.0625, np.nan]
    ints = rng.integers(1, 9, size=(N1, 3)).astype(np.float32)
    vals = (0.5 + 1.5 * rng.random((N1, 4))).astype(np.float32)
    return pts, q, h, ints, vals


@functools.lru_cache(maxsize=None)
def ref1(box, which, kernel):
    """the brute force of case 1's inputs: which = None (weight 1) or "ints"
    (the integer values, nv = 3)"""
    pts, q, h, ints, _ = inputs1()
    return brute(pts, q, h, box, ints if which == "ints" else None, kernel)


# ---------------------------------------------------------------- 1. exact membership
@pytest.mark.parametrize("box", [None, 1.0])
def test_membership_per_query_radii(gpu, box):
    pts, q, h, _, _ = inputs1()
    assert M1 % 64 != 0
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    cnt_ref = ref1(box, None, TOPHAT)[0]
    s, c = t.ball_sum(q, h, kernel=TOPHAT, count=True)
    assert s.dtype == np.float32 and s.shape == (M1,)
    assert c.dtype == np.uint32 and c.shape == (M1,)
    bad = np.flatnonzero(c != cnt_ref)
    assert bad.size == 0, f"{bad.size} counts differ, first rows {bad[:5]}: {c[bad[:5]]} vs {cnt_ref[bad[:5]]}"
    assert np.array_equal(s, c.astype(np.float32))
    assert np.all(c[ZERO_ROWS] == 1) and np.all(c[BAD_ROWS] == 0) and np.all(s[BAD_ROWS] == 0)
    assert np.all(c[WIDE_ROWS] > 1000)
    # the sum alone and the count alone
    assert np.array_equal(t.ball_sum(q, h, kernel=TOPHAT), s)
    # every h_i = r: the radius count, bit for bit
    for r in (0.0, 1.3 * S1, 0.6):
        s, c = t.ball_sum(q, np.full(M1, r, np.float32), kernel=CUBIC, count=True)
        assert np.array_equal(c, t.ball_count(q, r))


# ---------------------------------------------------------------- 2. exact sums in any order
@pytest.mark.parametrize("box", [None, 1.0])
def test_integer_sums_exact(gpu, box):
    """Values 1..8: every sum is an integer below 2^24, exact in any order."""
    pts, q, h, ints, _ = inputs1()
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    cnt_ref, s_ref, _, _ = ref1(box, "ints", TOPHAT)
    assert s_ref.max() < 2 ** 24
    s, c = t.ball_sum(q, h, ints, kernel=TOPHAT, count=True)
    assert s.shape == (M1, 3)
    assert np.array_equal(c, cnt_ref)
    assert np.array_equal(s.astype(np.float64), s_ref)
    # one channel, 1-D values
    s1 = t.ball_sum(q, h, ints[:, 1].copy(), kernel=TOPHAT)
    assert s1.shape == (M1,) and np.array_equal(s1, s[:, 1])


# ---------------------------------------------------------------- 3. kernel formula, bit for bit
@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("kernel", [CUBIC, WENDLAND, TOPHAT])
def test_kernel_formula_bit_for_bit(gpu, box, kernel):
    """A jittered 8^3 lattice and queries with exactly one neighbour each: a
    sum is one term, equal under == to the f32 numpy evaluation."""
    rng = np.random.default_rng(431)
    g = (np.arange(8) + 0.5) / 8
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = (pts + rng.uniform(-0.02, 0.02, pts.shape)).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    n = len(pts)
    h = rng.uniform(0.02, 0.04, n).astype(np.float32)  # below half the spacing less the jitter
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    frac = np.linspace(0.01, 0.99, n)  # u on both sides of 1/2
    q = (pts + d * (frac * h)[:, None]).astype(np.float32)
    vals = (0.5 + 1.5 * rng.random((n, 2))).astype(np.float32)
    mem, d2 = members(pts, q, h, box)
    assert np.all(mem.sum(axis=1) == 1) and np.all(mem[np.arange(n), np.arange(n)])
    d2 = d2[np.arange(n), np.arange(n)]
    inv = np.float32(1) / h
    u = np.minimum(np.sqrt(d2) * inv, np.float32(1))
    assert u.dtype == np.float32 and (u < 0.5).sum() > 100 and (u > 0.5).sum() > 100
    expect = vals * kern32(u, kernel)[:, None]
    assert expect.dtype == np.float32
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    s, c = t.ball_sum(q, h, vals, kernel=kernel, count=True)
    assert np.all(c == 1)
    bad = np.argwhere(s != expect)
    assert bad.size == 0, f"{len(bad)} terms differ, first {bad[:3]}: {s[tuple(bad[0])]!r} vs {expect[tuple(bad[0])]!r}"


# ---------------------------------------------------------------- 4. weighted sums within the bound
@pytest.mark.parametrize("box", [None, 1.0])
def test_weighted_sums_within_bound(gpu, box):
    """h_i = the 33rd-neighbour distance; values in [0.5, 2]; nv = 1 and 4."""
    pts, q, _, _, vals = inputs1()
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    h = t.query_kth(q, 33)
    for kernel in (CUBIC, WENDLAND):
        for v in (vals[:, :1].copy(), vals):
            cnt, s64, sabs, vabs = brute(pts, q, h, box, v, kernel)
            # (fl(h * h) may fall below the 33rd neighbour's d2: h = sqrtf(d2) is rounded)
            assert cnt.min() >= 32
            s, c = t.ball_sum(q, h, v, kernel=kernel, count=True)
            assert np.array_equal(c, cnt)
            assert_within_bound(s, cnt, s64, sabs, vabs, f"box {box} kernel {kernel} nv {v.shape[1]}")


# ---------------------------------------------------------------- 5. shapes
def check_all(t, pts, q, h, box, seed):
    """count exact, integer top-hat sums exact, cubic and Wendland sums within the bound"""
    rng = np.random.default_rng(seed)
    ints = rng.integers(1, 9, size=(len(pts), 3)).astype(np.float32)
    vals = (0.5 + 1.5 * rng.random((len(pts), 2))).astype(np.float32)
    cnt, s64, _, _ = brute(pts, q, h, box, ints, TOPHAT)
    s, c = t.ball_sum(q, h, ints, kernel=TOPHAT, count=True)
    assert np.array_equal(c, cnt), (c, cnt)
    assert np.array_equal(s.astype(np.float64), s64)
    for kernel in (CUBIC, WENDLAND):
        cnt, s64, sabs, vabs = brute(pts, q, h, box, vals, kernel)
        s, c = t.ball_sum(q, h, vals, kernel=kernel, count=True)
        assert np.array_equal(c, cnt)
        assert_within_bound(s, cnt, s64, sabs, vabs, f"kernel {kernel}")
    return cnt


@pytest.mark.parametrize("box", [None, 1.0])
def test_padding(gpu, box):
    """n = 13: padded to 16 with FLT_MAX points; balls that hold every point
    reach the padded leaf and count no padding."""
    pts = uniform(13, 451)
    q = np.concatenate([uniform(40, 452), pts])
    h = np.random.default_rng(453).uniform(0.0, 0.5, len(q)).astype(np.float32)
    h[:6] = 0.49 if box else 4.0
    h[6:9] = 3.0e19 if not box else 0.3  # h * h overflows: still 13, not 16
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    cnt = check_all(t, pts, q, h, box, 454)
    assert cnt.max() == 13 if box is None else cnt.max() > 3


@pytest.mark.parametrize("box", [None, 1.0])
def test_two_staged_chunks_per_leaf(gpu, box):
    pts = uniform(5000, 306)
    q = uniform(700, 455)
    h = (np.random.default_rng(456).random(700) * 3 * 5000 ** (-1.0 / 3.0)).astype(np.float32)
    t = gpu.Tree(pts, leafsize=128, boxsize=box)
    check_all(t, pts, q, h, box, 457)


def test_coincident_points_zero_radius(gpu):
    base = uniform(500, 405)
    pts = np.concatenate([base, base])[np.random.default_rng(406).permutation(1000)]
    for box in (None, 1.0):
        t = gpu.Tree(pts, leafsize=16, boxsize=box)
        cnt = check_all(t, pts, pts, np.zeros(1000, np.float32), box, 458)
        assert np.all(cnt == 2)
        # u = 0: K = 1 for every kernel, so the sums are exactly v_a + v_b
        v = np.arange(1000, dtype=np.float32)
        for kernel in (TOPHAT, CUBIC, WENDLAND):
            s = t.ball_sum(pts, np.zeros(1000, np.float32), v, kernel=kernel)
            same = (d2_ref(pts[:, None, :], pts[None, :, :], box) == 0).astype(np.float32)
            assert np.array_equal(s, same @ v)


@pytest.mark.parametrize("m", [1, 63, 65])
def test_small_query_counts(gpu, m):
    pts = uniform(2000, 459)
    q = uniform(m, 460 + m)
    h = np.full(m, 0.12, np.float32)
    for box in (None, 1.0):
        check_all(gpu.Tree(pts, leafsize=32, boxsize=box), pts, q, h, box, 461)


def test_periodic_queries_outside_the_box(gpu):
    """Queries outside [0, L]^3 take the brute kernel; mixed with inside ones."""
    pts = uniform(3000, 462)
    rng = np.random.default_rng(463)
    q = uniform(200, 464).copy()
    out = rng.choice(200, 37, replace=False)
    q[out] += rng.choice([-1.0, 1.0, 2.0], size=(37, 3)).astype(np.float32) * (rng.random((37, 3)) < 0.5)
    q[out[0]] = [1.5, 0.5, 0.5]
    inside = np.all((q >= 0) & (q <= 1), axis=1)
    assert 20 < (~inside).sum() <= 37
    h = rng.uniform(0.0, 0.2, 200).astype(np.float32)
    h[out[1]] = np.nan
    h[out[2]] = 0.7
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    cnt = check_all(t, pts, q, h, 1.0, 465)
    assert cnt[out[1]] == 0 and cnt[~inside].sum() > 100


# ---------------------------------------------------------------- 6. replaced ids
def test_replaced_ids(gpu):
    """After nbkd_set_ids the values are still indexed by input row."""
    n = 3000
    pts = uniform(n, 407)
    q = uniform(500, 466)
    h = np.full(500, 1.5 * n ** (-1.0 / 3.0), np.float32)
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    t.set_ids((np.random.default_rng(408).permutation(n) + 1_000_000).astype(np.uint32))
    check_all(t, pts, q, h, 1.0, 467)


# ---------------------------------------------------------------- 7. host streaming
def test_host_streaming_batches(gpu):
    """host_batch = 256, m = 1000 with a distinct h per row: every batch's
    slice of h follows its queries."""
    pts, q, h, ints, _ = inputs1()
    q, h = q[:1000], h[:1000]
    assert len(np.unique(h[18:])) == 1000 - 18
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    s1, c1 = t.ball_sum(q, h, ints, kernel=TOPHAT, count=True)
    assert np.array_equal(c1, ref1(1.0, "ints", TOPHAT)[0][:1000])
    old = gpu.get_tuning("host_batch")
    try:
        gpu.set_tuning("host_batch", 256)
        s2, c2 = t.ball_sum(q, h, ints, kernel=TOPHAT, count=True)
        only_c = np.empty(1000, np.uint32)
        gpu._check(gpu.lib().nbkd_query_ball_sum(t.h, q.ctypes.data, 1000, h.ctypes.data, None, 1,
                                                 TOPHAT, None, only_c.ctypes.data, 0, None))
    finally:
        gpu.set_tuning("host_batch", old)
    assert np.array_equal(c2, c1) and np.array_equal(s2, s1) and np.array_equal(only_c, c1)
    assert gpu.get_tuning("host_batch") == old


# ---------------------------------------------------------------- 8. device I/O, self order
@pytest.fixture
def timing(gpu):
    """the library's event timers, on for one test: a scope's call count shows
    which path ran"""
    gpu.timing_enable(True)
    gpu.timing_reset()
    yield gpu
    gpu.timing_enable(False)


@pytest.mark.parametrize("box", [None, 1.0])
def test_device_io_self_order_repeatability(gpu, timing, box):
    """Raw HIP buffers (nbodyhpc_amd.hip, not torch: see tests/test_gpu_fof.py).
    The tree is built from a device array and queried with that same pointer,
    so the self-order path runs, on a stream."""
    from nbodyhpc_amd import hip
    pts, _, _, ints, vals = inputs1()
    n, guard = N1, 64
    rng = np.random.default_rng(481)
    h = (rng.random(n) * 2.5 * S1).astype(np.float32)
    h[5], h[6] = np.nan, 0.6
    dp = hip.DeviceArray.from_numpy(pts)
    dh = hip.DeviceArray.from_numpy(h)
    di, dv = hip.DeviceArray.from_numpy(ints), hip.DeviceArray.from_numpy(vals)
    t = gpu.Tree(n=n, dev_ptr=dp.ptr, leafsize=32, boxsize=box)
    host = gpu.Tree(pts, leafsize=32, boxsize=box)  # the bucketed path, host arrays
    s = hip.Stream()
    cnt_all = members(pts, pts, h, box)[0].sum(axis=1)
    for m in (n, 1000):  # all rows; the first 1000 (their tree positions are listed)
        s_host, c_host = host.ball_sum(pts[:m], h[:m], ints, kernel=TOPHAT, count=True)
        assert np.array_equal(c_host, cnt_all[:m])
        runs = []
        for _ in range(2):
            ds = hip.DeviceArray.from_numpy(np.full(m * 3 + guard, -7.0, np.float32))
            dc = hip.DeviceArray.from_numpy(np.full(m + guard, 0xDEADBEEF, np.uint32))
            dk = hip.DeviceArray.from_numpy(np.full(m * 4 + guard, -7.0, np.float32))
            t.ball_sum_device(dp.ptr, m, dh.ptr, di.ptr, 3, TOPHAT, ds.ptr, dc.ptr, stream=s.handle)
            t.ball_sum_device(dp.ptr, m, dh.ptr, dv.ptr, 4, CUBIC, dk.ptr, None, stream=s.handle)
            s.synchronize()
            hs, hc, hk = ds.numpy(), dc.numpy(), dk.numpy()
            assert np.all(hs[m * 3:] == -7.0) and np.all(hc[m:] == 0xDEADBEEF)
            assert np.all(hk[m * 4:] == -7.0)
            runs.append((hs[:m * 3].reshape(m, 3), hc[:m], hk[:m * 4].reshape(m, 4)))
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b)
        assert np.array_equal(runs[0][1], c_host)
        assert np.array_equal(runs[0][0], s_host)
        if m == 1000:
            cnt, s64, sabs, vabs = brute(pts, pts[:m], h[:m], box, vals, CUBIC)
            assert_within_bound(runs[0][2], cnt, s64, sabs, vabs, f"self order m {m}")
    # weight 1 on the device: values NULL, the count alone
    dc = hip.DeviceArray.from_numpy(np.full(n + guard, 0xDEADBEEF, np.uint32))
    t.ball_sum_device(dp.ptr, n, dh.ptr, None, 1, WENDLAND, None, dc.ptr, stream=s.handle)
    s.synchronize()
    hc = dc.numpy()
    assert np.array_equal(hc[:n], cnt_all) and np.all(hc[n:] == 0xDEADBEEF)
    # every device call took the self-order path (2 x 2 x 2 + 1 calls); the
    # host tree's two calls did not
    assert timing.timing_read("self_order")[1] == 9
    assert timing.timing_read("ball_sum")[1] == 11


# ---------------------------------------------------------------- 9. Python surface
def test_python_surface(gpu):
    import math
    from nbodyhpc_amd.kdtree import KDTree
    pts, q, _, _, vals = inputs1()
    t = KDTree(pts, leafsize=32, boxsize=1.0)
    # sph_density of the tree's own points, unit masses, top-hat: count * 3 / (4 pi h^3)
    k = 32
    hk = t.kth_distance(pts, k)
    rho = t.sph_density(k=k, kernel="tophat")
    cnt = members(pts, pts, hk, 1.0)[0].sum(axis=1)
    assert cnt.min() >= k - 1  # (fl(h * h) may fall below the k-th neighbour's d2)
    assert rho.dtype == np.float64 and rho.shape == (N1,)
    assert np.array_equal(rho, 3.0 / (4.0 * math.pi) * cnt.astype(np.float64) / hk.astype(np.float64) ** 3)
    # kernel_sum: shapes, broadcasting, counts
    q3 = q[:1200].reshape(30, 40, 3)
    s, c = t.kernel_sum(q3, 2 * S1, vals[:, :2], kernel="wendland", return_count=True)
    assert s.dtype == np.float64 and s.shape == (30, 40, 2) and c.shape == (30, 40)
    cb, s64, sabs, vabs = brute(pts, q[:1200], np.full(1200, 2 * S1, np.float32), 1.0,
                                vals[:, :2], WENDLAND)
    assert np.array_equal(c.reshape(-1), cb)
    assert_within_bound(s.reshape(-1, 2), cb, s64, sabs, vabs, "kernel_sum")
    assert t.kernel_sum(q[:7], np.linspace(0.01, 0.1, 7)).shape == (7,)
    # sph_density with masses at arbitrary points: sigma / h^3 * sum
    mass = vals[:, 0].copy()
    h = np.full(1200, 2 * S1, np.float32)
    rho = t.sph_density(q[:1200], mass=mass, kernel="cubic", h=h)
    cb, s64, sabs, vabs = brute(pts, q[:1200], h, 1.0, mass, CUBIC)
    scale = 8.0 / math.pi / h.astype(np.float64) ** 3
    assert_within_bound(rho / scale, cb, s64, sabs, vabs, "sph_density")
    # interpolate: a constant field comes back within 4 ulp (f32) where the
    # ball is not empty, NaN where it is.  Top-hat, any constant: numerator
    # c * n and denominator n are exact in f32 for n < 2^21 (c = 2.5 has three
    # significant bits).  Cubic with masses and a power of two: scaling by 8 is
    # exact at every step, so numerator = 8 * denominator bit for bit.
    hq = (np.random.default_rng(491).random(M1) * 1.5 * S1).astype(np.float32)
    empty = members(pts, q, hq, 1.0)[0].sum(axis=1) == 0
    assert 50 < empty.sum() < M1 - 50
    for const, kernel, m_ in ((2.5, "tophat", None), (8.0, "cubic", vals[:, 1]),
                              (8.0, "wendland", None)):
        out = t.interpolate(q, hq, np.full(N1, const), mass=m_, kernel=kernel)
        assert out.shape == (M1,) and np.all(np.isnan(out[empty]))
        # (a ball whose only members sit at u = 1 has K = 0: 0 / 0)
        ok = ~empty & ~np.isnan(out)
        assert ok.sum() > (~empty).sum() - 5
        assert np.all(np.abs(out[ok] - const) <= 4 * np.spacing(np.float32(const)))
    # several channels
    f3 = np.stack([np.full(N1, 1.0), np.full(N1, -2.0), np.full(N1, 0.5)], 1)
    out = t.interpolate(q, hq, f3, kernel="cubic")
    assert out.shape == (M1, 3)
    ok = ~np.isnan(out[:, 0])
    assert np.array_equal(out[ok], np.broadcast_to([1.0, -2.0, 0.5], (ok.sum(), 3)))
