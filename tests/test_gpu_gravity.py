"""Barnes-Hut potentials and accelerations (nbkd_gravity, gravity.hip) against
two numpy oracles: a float64 brute force (the direct sum), and the walk that
nbkd.h defines run over the exported tree (moments in float64 in the stated
order, the opening test in float32, the accepted monopoles and the remaining
points summed in float64).  New (no reference counterpart).

Rounding bound per output component: (T + 16) * u * sum |t_i|, u = 2^-24, T the
number of terms of that query, t_i the terms of that component evaluated in
float64 from the float32 inputs: each term carries fewer than 16 roundings, and
a sequential float32 sum of T terms adds at most (T - 1) * u * sum |t|."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


# ---------------------------------------------------------------- inputs
def cube(n, seed):
    """n float32 points in [-0.5, 0.5]^3"""
    return (np.random.default_rng(seed).random((n, 3)) - 0.5).astype(np.float32)


def clumps(n, seed):
    """eight Gaussian clumps of sigma = 0.02, kept inside [-0.5, 0.5]^3"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.35, 0.35, (8, 3))
    p = c[rng.integers(0, 8, n)] + rng.normal(0.0, 0.02, (n, 3))
    return np.clip(p, -0.5, 0.5).astype(np.float32)


def masses(n, seed):
    return (0.5 + np.random.default_rng(seed).random(n)).astype(np.float32)


# ---------------------------------------------------------------- oracles
class Sums:
    """float64 sums of one call's terms per query: values (phi, ax, ay, az), the
    sums of |term| per component, and the term count"""

    def __init__(self, m):
        self.val = np.zeros((m, 4))
        self.abs = np.zeros((m, 4))
        self.T = np.zeros(m, np.int64)
        self.accepted = np.zeros(m, np.int64)

    def add(self, rows, q, mu, p, eps):
        """queries `rows` (positions q[rows]) each gain the terms (mu[j], p[j])"""
        d = p[None, :, :].astype(np.float64) - q[rows, None, :].astype(np.float64)
        d2 = (d * d).sum(axis=2)
        on = d2 != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(on, 1.0 / np.sqrt(d2 + float(eps) ** 2), 0.0)
        mu = np.asarray(mu, np.float64)[None, :]
        t = np.concatenate([(-mu * inv)[:, :, None], (mu * inv ** 3)[:, :, None] * d], axis=2)
        self.val[rows] += t.sum(axis=1)
        self.abs[rows] += np.abs(t).sum(axis=1)
        self.T[rows] += on.sum(axis=1)


def brute(pts, mass, q, eps):
    """the direct sum in float64"""
    s = Sums(len(q))
    for a in range(0, len(q), 256):
        s.add(np.arange(a, min(a + 256, len(q))), q, mass, pts, eps)
    return s


def moments(nodes, xyz, mt, real):
    """per node, as nbkd.h defines them: M (f32), c (f32, 3), s2 (f32)"""
    nn = len(nodes)
    M64, S64 = np.zeros(nn), np.zeros((nn, 3))
    lo, hi = np.zeros((nn, 3), np.float32), np.zeros((nn, 3), np.float32)

    def fill(i):
        nd = nodes[i]
        if nd["dim"] < 0:
            sel = np.arange(nd["left"], nd["right"])
            sel = sel[real[sel]]
            assert sel.size > 0  # no node without a real point
            m = mt[sel].astype(np.float64)
            M64[i] = np.cumsum(m)[-1]
            S64[i] = np.cumsum(m[:, None] * xyz[sel].astype(np.float64), axis=0)[-1]
            lo[i], hi[i] = xyz[sel].min(axis=0), xyz[sel].max(axis=0)
        else:
            l, r = int(nd["left"]), int(nd["right"])
            fill(l)
            fill(r)
            M64[i] = M64[l] + M64[r]
            S64[i] = S64[l] + S64[r]
            lo[i], hi[i] = np.minimum(lo[l], lo[r]), np.maximum(hi[l], hi[r])

    fill(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (S64 / M64[:, None]).astype(np.float32)
    none = M64 == 0
    c[none] = (np.float32(0.5) * (lo + hi))[none]
    e = hi - lo
    s2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    assert e.dtype == np.float32 and s2.dtype == np.float32
    return M64.astype(np.float32), c, s2


def tree_walk(exported, n, mass, q, theta, eps):
    """nbkd.h's walk over an exported tree (nodes, x, y, z, perm)"""
    nodes, x, y, z, perm = exported
    xyz = np.stack([x, y, z], 1)
    real = perm < n
    mt = np.zeros(len(perm), np.float32)
    mt[real] = np.asarray(mass, np.float32)[perm[real]]
    M, c, s2 = moments(nodes, xyz, mt, real)
    th2 = np.float32(theta) * np.float32(theta)
    s = Sums(len(q))

    def visit(i, rows):
        d = c[i][None, :] - q[rows]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        ok = (s2[i] <= th2 * d2) if th2 > 0 else np.zeros(len(rows), bool)
        if ok.any():
            s.add(rows[ok], q, M[i:i + 1], c[i:i + 1], eps)
            s.accepted[rows[ok]] += 1
        rows = rows[~ok]
        if rows.size == 0:
            return
        nd = nodes[i]
        if nd["dim"] < 0:
            sel = np.arange(nd["left"], nd["right"])
            sel = sel[real[sel]]
            s.add(rows, q, mt[sel], xyz[sel], eps)
        else:
            visit(int(nd["left"]), rows)
            visit(int(nd["right"]), rows)

    visit(0, np.arange(len(q)))
    return s


WORST = {}


def assert_within(phi, acc, s, what):
    """every component of every query within (T + 16) u sum |t|"""
    got = np.concatenate([np.asarray(phi, np.float64).reshape(-1, 1),
                          np.asarray(acc, np.float64).reshape(-1, 3)], axis=1)
    bound = (s.T[:, None] + 16) * U24 * s.abs
    err = np.abs(got - s.val)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0)))
    WORST[what] = ratio
    print(f"{what}: worst error {ratio:.4f} of the rounding bound")
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, f"{what}: {len(bad)} components outside the bound, first {bad[:3]}"


# ---------------------------------------------------------------- shared case 1
N1, M1 = 2003, 300


@functools.lru_cache(maxsize=None)
def case1():
    pts, mass = cube(N1, 601), masses(N1, 602)
    q = np.concatenate([cube(M1, 603), pts[:M1]])
    return pts, mass, q


@functools.lru_cache(maxsize=None)
def ref1(eps, unit):
    pts, mass, q = case1()
    return brute(pts, np.ones(N1, np.float32) if unit else mass, q, eps)


# ---------------------------------------------------------------- 1. the direct sum
@pytest.mark.parametrize("eps", [0.0, 0.05])
def test_direct_sum(gpu, eps):
    pts, mass, q = case1()
    assert N1 % 8 != 0  # padding points are present
    t = gpu.Tree(pts, leafsize=16)
    phi, acc = t.gravity(q, mass, theta=0.0, eps=eps)
    assert phi.dtype == np.float32 and phi.shape == (2 * M1,)
    assert acc.dtype == np.float32 and acc.shape == (2 * M1, 3)
    s = ref1(eps, False)
    assert np.all(s.T[:M1] == N1) and np.all(s.T[M1:] == N1 - 1)
    assert_within(phi, acc, s, f"direct eps {eps}")
    p1, a1 = t.gravity(q, None, theta=0.0, eps=eps)
    p2, a2 = t.gravity(q, np.ones(N1, np.float32), theta=0.0, eps=eps)
    assert np.array_equal(p1, p2) and np.array_equal(a1, a2)
    assert_within(p1, a1, ref1(eps, True), f"direct unit masses eps {eps}")


# ---------------------------------------------------------------- 2. the tree oracle
N2, FAR2 = 3000, 500


def shell(m, seed, lo=1.75, hi=4.0):
    """m float32 points with lo <= max |coordinate| <= hi: outside the points'
    cube, at least lo - 0.5 from it"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-hi, hi, (m, 3))
    a = rng.integers(0, 3, m)
    q[np.arange(m), a] = rng.uniform(lo, hi, m) * rng.choice([-1.0, 1.0], m)
    return q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case2(dist):
    """rows [0, FAR2): far queries; then 200 queries inside the cube and the
    first 400 own points"""
    pts = cube(N2, 611) if dist == "uniform" else clumps(N2, 612)
    q = np.concatenate([shell(FAR2, 615), cube(200, 613), pts[:400]])
    mass = masses(N2, 614)
    return pts, mass, q, brute(pts, mass, q, 0.0)


@pytest.mark.parametrize("theta", [0.3, 0.6, 0.9])
@pytest.mark.parametrize("leafsize", [16, 64])
@pytest.mark.parametrize("dist", ["uniform", "clumps"])
def test_tree_oracle(gpu, dist, leafsize, theta):
    """Every query is compared.  Every far query must accept a node at every
    theta, otherwise the comparison proves nothing about the monopoles: a leaf
    of 64 of 3000 uniform points has a diagonal near 0.5, so s <= 0.3 d needs
    d >= 1.6, which no query inside the unit cube has; the far rows lie 1.25 to
    3.5 outside it (they open the nearer nodes and accept the farther ones).
    The inside rows and the own points accept what the geometry lets them
    (nothing at theta = 0.3 on uniform points) and are compared all the same;
    over all of them some node must be accepted from theta = 0.6 on."""
    pts, mass, q, direct = case2(dist)
    t = gpu.Tree(pts, leafsize=leafsize)
    exported = t.export()
    for eps in (0.0, 0.01):
        s = tree_walk(exported, N2, mass, q, theta, eps)
        assert s.accepted[:FAR2].min() > 0, "a far query accepted no node"
        if theta == 0.3:
            assert s.T[:FAR2].max() > 1, "no far query opened the root"
        if theta >= 0.6:
            assert s.accepted[FAR2:].sum() > 0
        print(f"accepted nodes per query: far {s.accepted[:FAR2].mean():.1f}, "
              f"near {s.accepted[FAR2:].mean():.1f}; terms {s.T[:FAR2].mean():.0f}, "
              f"{s.T[FAR2:].mean():.0f}")
        phi, acc = t.gravity(q, mass, theta=theta, eps=eps)
        assert_within(phi, acc, s, f"{dist} leaf {leafsize} theta {theta} eps {eps}")
        if eps == 0.0:
            # the monopole remainder M b^2 / (d^2 (d - b)) with b <= theta d
            rem = 1.01 * theta ** 2 * (1 + theta) / (1 - theta) * np.abs(direct.val[:, 0])
            rnd = (s.T + 16) * U24 * s.abs[:, 0]
            err = np.abs(phi.astype(np.float64) - direct.val[:, 0])
            print(f"worst relative potential error {np.max(err / np.abs(direct.val[:, 0])):.2e}")
            assert np.all(err <= rem + rnd)


# ---------------------------------------------------------------- 3. canonical order
def test_canonical_order(gpu):
    """The build array as device queries (the self-order path), the same rows
    as host queries (bucketed and sorted), and host batches of 64: == arrays."""
    from nbodyhpc_amd import hip
    pts, mass, _ = case1()
    dp, dm = hip.DeviceArray.from_numpy(pts), hip.DeviceArray.from_numpy(mass)
    t = gpu.Tree(n=N1, dev_ptr=dp.ptr, leafsize=16)
    s = hip.Stream()
    gpu.timing_enable(True)
    gpu.timing_reset()
    try:
        runs = []
        for _ in range(2):
            dphi = hip.DeviceArray.from_numpy(np.full(N1, -7.0, np.float32))
            dacc = hip.DeviceArray.from_numpy(np.full(3 * N1, -7.0, np.float32))
            t.gravity_device(dp.ptr, N1, dm.ptr, 0.5, 0.01, dphi.ptr, dacc.ptr, stream=s.handle)
            s.synchronize()
            runs.append((dphi.numpy(), dacc.numpy().reshape(N1, 3)))
        assert gpu.timing_read("self_order")[1] == 2
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        hphi, hacc = t.gravity(pts, mass, theta=0.5, eps=0.01)
        assert gpu.timing_read("self_order")[1] == 2 and gpu.timing_read("gravity_walk")[1] == 3
        old = gpu.get_tuning("host_batch")
        try:
            gpu.set_tuning("host_batch", 64)
            bphi, bacc = t.gravity(pts, mass, theta=0.5, eps=0.01)
        finally:
            gpu.set_tuning("host_batch", old)
        assert gpu.timing_read("gravity_walk")[1] == 3 + (N1 + 63) // 64
        assert gpu.timing_read("gravity_moments")[1] == 4  # once per call
    finally:
        gpu.timing_enable(False)
    assert np.all(runs[0][0] < 0)
    assert np.array_equal(hphi, runs[0][0]) and np.array_equal(hacc, runs[0][1])
    assert np.array_equal(bphi, runs[0][0]) and np.array_equal(bacc, runs[0][1])
    assert_within(hphi, hacc, tree_walk(t.export(), N1, mass, pts, 0.5, 0.01), "canonical order")


# ---------------------------------------------------------------- 4. small and degenerate shapes
def check_tree(gpu, pts, mass, q, leafsize=16, thetas=(0.0, 0.5), eps=(0.0, 0.02), what=""):
    t = gpu.Tree(pts, leafsize=leafsize)
    exported = t.export()
    for theta in thetas:
        for e in eps:
            s = tree_walk(exported, len(pts), np.ones(len(pts)) if mass is None else mass, q,
                          theta, e)
            phi, acc = t.gravity(q, mass, theta=theta, eps=e)
            assert_within(phi, acc, s, f"{what} theta {theta} eps {e}")
    return t


@pytest.mark.parametrize("m", [1, 63, 65])
def test_small_query_counts(gpu, m):
    pts = cube(700, 621)
    check_tree(gpu, pts, masses(700, 622), cube(m, 623 + m), what=f"m {m}")


def test_one_point(gpu):
    pts = cube(1, 631)
    t = check_tree(gpu, pts, np.array([1.25], np.float32), cube(5, 632), what="n 1")
    for theta in (0.0, 0.5):
        phi, acc = t.gravity(pts, np.array([1.25], np.float32), theta=theta, eps=0.1)
        assert np.all(phi == 0) and np.all(acc == 0)


def test_seventeen_points(gpu):
    pts = cube(17, 633)
    check_tree(gpu, pts, masses(17, 634), np.concatenate([cube(30, 635), pts]), what="n 17")


def test_all_points_coincident(gpu):
    p = np.array([[0.125, -0.25, 0.375]], np.float32)
    pts = np.repeat(p, 40, axis=0)
    mass = masses(40, 636)
    out = cube(9, 637)
    t = check_tree(gpu, pts, mass, out, what="coincident")
    for theta in (0.0, 0.5):
        for eps in (0.0, 0.05):
            phi, acc = t.gravity(pts, mass, theta=theta, eps=eps)
            assert np.all(phi == 0) and np.all(acc == 0)
    # an outside query sees the single monopole (M, p)
    s = tree_walk(t.export(), 40, mass, out, 0.5, 0.0)
    assert np.all(s.accepted == 1) and np.all(s.T == 1)
    phi, acc = t.gravity(out, mass, theta=0.5, eps=0.0)
    M = np.float32(np.cumsum(mass.astype(np.float64))[-1])
    d = p - out
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.allclose(phi, -M / np.sqrt(d2), rtol=8 * U24, atol=0)


def test_two_coincident_points_softened(gpu):
    """each sees nothing from the other, whatever the softening"""
    pts = np.array([[0.1, 0.2, -0.3], [0.1, 0.2, -0.3]], np.float32)
    t = gpu.Tree(pts, leafsize=16)
    for theta in (0.0, 0.7):
        phi, acc = t.gravity(pts, None, theta=theta, eps=0.05)
        assert np.all(phi == 0) and np.all(acc == 0)


def test_zero_mass_subset(gpu):
    pts = cube(900, 641)
    mass = masses(900, 642)
    mass[np.random.default_rng(643).random(900) < 0.3] = 0.0
    order = np.argsort(pts[:, 0], kind="stable")
    mass[order[:130]] = 0.0  # whole leaves, and nodes above them, without mass
    q = np.concatenate([cube(100, 644), pts[:200]])
    check_tree(gpu, pts, mass, q, thetas=(0.0, 0.4, 0.8), what="zero masses")


def test_two_staged_chunks_per_leaf(gpu):
    pts = cube(1500, 645)
    q = np.concatenate([cube(100, 646), pts[:100]])
    check_tree(gpu, pts, masses(1500, 647), q, leafsize=128, thetas=(0.0, 0.6), what="leaf 128")


# ---------------------------------------------------------------- 5. replaced ids
def test_replaced_ids(gpu):
    """After nbkd_set_ids the masses are still indexed by input row."""
    n = 1500
    pts, mass = cube(n, 651), masses(n, 652)
    q = np.concatenate([cube(200, 653), pts[:200]])
    t = gpu.Tree(pts, leafsize=16)
    exported = t.export()  # the build's permutation
    before = t.gravity(q, mass, theta=0.5, eps=0.01)
    t.set_ids((np.random.default_rng(654).permutation(n) + 1_000_000).astype(np.uint32))
    after = t.gravity(q, mass, theta=0.5, eps=0.01)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert_within(after[0], after[1], tree_walk(exported, n, mass, q, 0.5, 0.01), "replaced ids")
    phi, acc = t.gravity(q, mass, theta=0.0, eps=0.01)
    assert_within(phi, acc, brute(pts, mass, q, 0.01), "replaced ids direct")


# ---------------------------------------------------------------- 6. device buffers, a caller's stream
def test_device_buffers_on_a_stream(gpu):
    from nbodyhpc_amd import hip
    pts, mass, q = case1()
    m, guard = len(q), 64
    t = gpu.Tree(pts, leafsize=16)
    dq, dm = hip.DeviceArray.from_numpy(q), hip.DeviceArray.from_numpy(mass)
    s = hip.Stream()

    def run(want_phi, want_acc):
        dphi = hip.DeviceArray.from_numpy(np.full(guard + m + guard, -7.0, np.float32))
        dacc = hip.DeviceArray.from_numpy(np.full(guard + 3 * m + guard, -7.0, np.float32))
        t.gravity_device(dq.ptr, m, dm.ptr, 0.5, 0.01, dphi.ptr + 4 * guard if want_phi else None,
                         dacc.ptr + 4 * guard if want_acc else None, stream=s.handle)
        s.synchronize()
        hp, ha = dphi.numpy(), dacc.numpy()
        assert np.all(hp[:guard] == -7.0) and np.all(hp[guard + m:] == -7.0)
        assert np.all(ha[:guard] == -7.0) and np.all(ha[guard + 3 * m:] == -7.0)
        return hp[guard:guard + m], ha[guard:guard + 3 * m].reshape(m, 3)

    phi, acc = run(True, True)
    assert_within(phi, acc, tree_walk(t.export(), N1, mass, q, 0.5, 0.01), "device buffers")
    p_only, untouched = run(True, False)
    assert np.array_equal(p_only, phi) and np.all(untouched == -7.0)
    untouched, a_only = run(False, True)
    assert np.array_equal(a_only, acc) and np.all(untouched == -7.0)
    hphi, hacc = t.gravity(q, mass, theta=0.5, eps=0.01)
    assert np.array_equal(hphi, phi) and np.array_equal(hacc, acc)
    assert np.array_equal(t.gravity(q, mass, theta=0.5, eps=0.01, acc=False)[0], phi)
    assert np.array_equal(t.gravity(q, mass, theta=0.5, eps=0.01, phi=False)[1], acc)


# ---------------------------------------------------------------- 7. rejections
def test_rejections_on_a_live_tree(gpu):
    pts = (cube(500, 661) + np.float32(0.5)).astype(np.float32)
    q = np.ascontiguousarray(pts[:8])
    phi, acc = np.full(8, 77.0, np.float32), np.full((8, 3), 77.0, np.float32)

    def call(t, theta, eps):
        st = gpu.lib().nbkd_gravity(t.h, q.ctypes.data, 8, None, ctypes.c_float(theta),
                                    ctypes.c_float(eps), phi.ctypes.data, acc.ctypes.data, 0, None)
        return st, gpu.lib().nbkd_last_error()

    per = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    st, msg = call(per, 0.5, 0.0)
    assert st == gpu.NBKD_EINVAL and b"Ewald" in msg
    with pytest.raises(gpu.NbkdError) as e:
        per.gravity(q)
    assert e.value.status == gpu.NBKD_EINVAL
    t = gpu.Tree(pts, leafsize=16)
    for theta, eps, word in ((1.0, 0.0, b"theta"), (0.5, -1.0, b"eps")):
        st, msg = call(t, theta, eps)
        assert st == gpu.NBKD_EINVAL and word in msg
    assert np.all(phi == 77.0) and np.all(acc == 77.0)
    st, _ = call(t, 0.5, 0.0)
    assert st == gpu.NBKD_OK and np.all(phi < 0)


# ---------------------------------------------------------------- 8. Python surface
def test_python_surface(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    pts, mass, q = case1()
    t = KDTree(pts, leafsize=16)
    s = ref1(0.05, False)
    G = 4.30091e-6
    phi, acc = t.gravity(q, mass, softening=0.05, theta=0.0, G=G)
    assert phi.dtype == np.float64 and phi.shape == (2 * M1,)
    assert acc.dtype == np.float64 and acc.shape == (2 * M1, 3)
    assert_within(phi / G, acc / G, s, "KDTree.gravity")
    p = t.potential(q.reshape(2, M1, 3), mass, softening=0.05, theta=0.0)
    assert p.shape == (2, M1) and np.array_equal(p.reshape(-1) * G, phi)
    only_a = t.gravity(q, mass, softening=0.05, theta=0.0, potential=False)
    assert only_a[0] is None and np.array_equal(only_a[1] * G, acc)
    # points=None: the tree's own points, unit masses; theta > 0 against the walk
    phi0, acc0 = t.gravity(theta=0.5)
    assert phi0.shape == (N1,) and acc0.shape == (N1, 3)
    nodes, x, y, z, idx = t.export()
    nd = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4)
    rec = np.zeros(len(nd), gpu.NODE_DTYPE)
    rec["dim"], rec["split"] = nd[:, 0].view(np.int32), nd[:, 1].view(np.float32)
    rec["left"], rec["right"] = nd[:, 2], nd[:, 3]
    assert_within(phi0, acc0, tree_walk((rec, x, y, z, idx), N1, np.ones(N1), pts, 0.5, 0.0),
                  "KDTree.gravity own points")
    assert np.array_equal(t.potential(), phi0)
    with pytest.raises(ValueError, match="Ewald"):
        KDTree(pts + np.float32(0.5), leafsize=16, boxsize=1.0).gravity()
