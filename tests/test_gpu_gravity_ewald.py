"""Barnes-Hut potentials and accelerations on a periodic tree
(nbkd_gravity_ewald, gravity_ewald.hip) against two numpy oracles:
(A) a float64 direct Ewald sum from nbkd.h's formulas, with no table, and
(B) the walk that nbkd.h defines run over the exported tree, with the exported
table interpolated in the stated float32 steps and the terms summed in float64.
New (no reference counterpart).

Rounding bound per output component, as in test_gpu_gravity.py:
(T + 16) * u * sum t_i, u = 2^-24, T the number of terms of that query,
t_i = |mu| (inv + cmax_i iL) for the potential and |mu| (inv^3 |d_a| + cmax_i iL2)
for an acceleration component, cmax_i the largest magnitude among the eight
table corners the term uses (which covers cancellation inside the
interpolation).  Against oracle A the interpolation error of the table is
allowed on top: 2 E_phi iL sum m and 2 E_a iL2 sum m (doubled: a sample maximum
underestimates the supremum), E_phi and E_a as measured by
test_gravity_ewald_host.py::test_interpolation_error and recorded in DESIGN.md
(section "Periodic gravity", line "Interpolation error").

Worst measured fractions of the bound on an MI355X: 0.28 (n = 1, a sum of one
term), 0.21 against oracle A (the interpolation allowance), 0.07 against oracle
B, 0.05 for the direct sums against the interpolated table."""
import ctypes
import functools

import numpy as np
import pytest

from . import ewald_oracle as eo

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
E_PHI, E_A = 1.245e-4, 5.58e-4  # DESIGN.md, "Interpolation error", box units
F32 = np.float32


# ---------------------------------------------------------------- inputs
def box(n, seed, L=1.0):
    """n float32 points in [0, L)^3"""
    p = (np.random.default_rng(seed).random((n, 3)) * L).astype(F32)
    p[p >= F32(L)] = 0.0
    return p


def clumps(n, seed, L=1.0):
    """eight Gaussian clumps of sigma = 0.02 L, the first centred on the corner
    (0, 0, 0) of the box, so that it lies across all three faces"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.15, 0.85, (8, 3))
    c[0] = 0.0
    p = c[rng.integers(0, 8, n)] + rng.normal(0.0, 0.02, (n, 3))
    p = ((p - np.floor(p)) * L).astype(F32)
    p[p >= F32(L)] = 0.0
    return p


def masses(n, seed):
    return (0.5 + 1.5 * np.random.default_rng(seed).random(n)).astype(F32)


@functools.lru_cache(maxsize=None)
def table():
    from nbodyhpc_amd import capi
    t = capi.ewald_table()
    t.setflags(write=False)
    return t


def wrap32(d, L):
    """nbkd.h's offset rule per axis, in float32"""
    L = F32(L)
    d = np.asarray(d, F32)
    dm, dp = d - L, d + L
    r = np.where(np.abs(dm) < np.abs(d), dm, d)
    r = np.where(np.abs(dp) < np.abs(r), dp, r)
    assert r.dtype == F32
    return r


# ---------------------------------------------------------------- oracles
class Sums:
    """float64 sums of one call's terms per query: values (phi, ax, ay, az), the
    sums of the bound's t_i per component, and the term count"""

    def __init__(self, m, L):
        self.L = L
        self.iL = F32(1.0) / F32(L)
        self.iL2 = self.iL * self.iL
        self.val = np.zeros((m, 4))
        self.abs = np.zeros((m, 4))
        self.T = np.zeros(m, np.int64)
        self.accepted = np.zeros(m, np.int64)
        self.msum = np.zeros(m)

    def offsets(self, rows, q, p):
        d = wrap32(p[None, :, :] - q[rows, None, :], self.L)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == F32
        return d, d2 != 0

    def add(self, rows, q, mu, p, eps, exact=None):
        """queries `rows` (positions q[rows]) each gain the terms (mu[j], p[j]):
        the correction interpolated from the table, or (exact: a key under which
        the values are kept for the next eps) from the float64 sums at the
        float64 offset"""
        d32, on = self.offsets(rows, q, p)
        d = d32.astype(np.float64)
        d2 = (d * d).sum(axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(on, 1.0 / np.sqrt(d2 + float(eps) ** 2), 0.0)
        mu32 = np.asarray(mu, F32)
        mu = mu32.astype(np.float64)[None, :]
        C, cmax = eo.interpolate(table(), d32.reshape(-1, 3), self.L)
        cmax = cmax.reshape(d32.shape[:2] + (4,)).astype(np.float64)
        if exact is not None:
            if exact not in EXACT:
                cphi, ca = eo.corrections(d.reshape(-1, 3) / float(self.L))
                C = np.concatenate([cphi[:, None] / float(self.L), ca / float(self.L) ** 2], 1)
                EXACT[exact] = C.reshape(d32.shape[:2] + (4,))
            C = EXACT[exact]
            kp = ka = mu
        else:
            C = C.reshape(d32.shape[:2] + (4,)).astype(np.float64)
            kp = (mu32 * self.iL).astype(np.float64)[None, :]
            ka = (mu32 * self.iL2).astype(np.float64)[None, :]
        onf = on.astype(np.float64)
        t = np.concatenate([(-mu * inv - onf * kp * C[..., 0])[:, :, None],
                            (mu * inv ** 3)[:, :, None] * d + (onf * ka)[:, :, None] * C[..., 1:]],
                           axis=2)
        a = np.concatenate(
            [(mu * (inv + onf * cmax[..., 0] * float(self.iL)))[:, :, None],
             mu[:, :, None] * ((inv ** 3)[:, :, None] * np.abs(d)
                               + onf[:, :, None] * cmax[..., 1:] * float(self.iL2))], axis=2)
        self.val[rows] += t.sum(axis=1)
        self.abs[rows] += a.sum(axis=1)
        self.T[rows] += on.sum(axis=1)
        self.msum[rows] += (onf * mu).sum(axis=1)


EXACT = {}


def direct(pts, mass, q, eps, L, exact):
    """every point a term: oracle A (exact) or the theta = 0 walk's sums"""
    s = Sums(len(q), L)
    for a in range(0, len(q), 64):
        s.add(np.arange(a, min(a + 64, len(q))), q, mass, pts, eps, (L, a) if exact else None)
    return s


def moments(nodes, xyz, mt, real):
    """per node, as nbkd.h defines them: M (f32), c (f32, 3), s2 (f32)"""
    nn = len(nodes)
    M64, S64 = np.zeros(nn), np.zeros((nn, 3))
    lo, hi = np.zeros((nn, 3), F32), np.zeros((nn, 3), F32)

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
        c = (S64 / M64[:, None]).astype(F32)
    none = M64 == 0
    c[none] = (F32(0.5) * (lo + hi))[none]
    e = hi - lo
    s2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    assert e.dtype == F32 and s2.dtype == F32
    return M64.astype(F32), c, s2


def tree_walk(exported, n, mass, q, theta, eps, L):
    """oracle B: nbkd.h's walk over an exported tree (nodes, x, y, z, perm)"""
    nodes, x, y, z, perm = exported
    xyz = np.stack([x, y, z], 1)
    real = perm < n
    mt = np.zeros(len(perm), F32)
    mt[real] = np.asarray(mass, F32)[perm[real]]
    M, c, s2 = moments(nodes, xyz, mt, real)
    th2 = F32(theta) * F32(theta)
    s = Sums(len(q), L)

    def visit(i, rows):
        d = wrap32(c[i][None, :] - q[rows], L)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == F32
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


def check(phi, acc, s, what, interp=False):
    """every component of every query within (T + 16) u sum t, plus (oracle A)
    the doubled interpolation error of the table"""
    got = np.concatenate([np.asarray(phi, np.float64).reshape(-1, 1),
                          np.asarray(acc, np.float64).reshape(-1, 3)], axis=1)
    bound = (s.T[:, None] + 16) * U24 * s.abs
    err = np.abs(got - s.val)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0)))
    if interp:
        extra = np.concatenate([(2 * E_PHI * float(s.iL) * s.msum)[:, None],
                                np.repeat((2 * E_A * float(s.iL2) * s.msum)[:, None], 3, 1)], 1)
        ratio = float(np.max(err / np.where(bound + extra > 0, bound + extra, 1.0)))
        bound = bound + extra
    WORST[what] = ratio
    print(f"{what}: worst error {ratio:.4f} of the bound")
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, f"{what}: {len(bad)} components outside the bound, first {bad[:3]}"
    return bound


# ---------------------------------------------------------------- 1. the lattice identity
def test_lattice_identity(gpu):
    """8^3 unit masses on the lattice k/8 of a unit box see, each, the lattice
    of spacing 1/8 without themselves and their own images:
    phi = 2.8372975 * 8 - 2.8372975 = 19.861082 and no acceleration.  Every
    offset is a table node (no interpolation error); the offsets of exactly
    +-1/2 exercise the tie of the wrap."""
    k = np.arange(8, dtype=F32) / F32(8)
    pts = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    t = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    phi, acc = t.gravity_ewald(pts, None, theta=0.0, eps=0.0)
    s = direct(pts, np.ones(512, F32), pts, 0.0, 1.0, False)
    assert np.all(s.T == 511)
    bound = (s.T[:, None] + 16) * U24 * s.abs
    print(f"phi in [{phi.min():.6f}, {phi.max():.6f}], max |acc| {np.abs(acc).max():.2e}, "
          f"bounds {bound[:, 0].max():.2e} {bound[:, 1:].max():.2e}")
    assert np.all(np.abs(phi.astype(np.float64) - 2.8372975 * 7) <= bound[:, 0])
    assert np.all(np.abs(acc.astype(np.float64)) <= bound[:, 1:])
    check(phi, acc, s, "lattice")


# ---------------------------------------------------------------- 2. oracle A
N2, M2 = 257, 64


@functools.lru_cache(maxsize=None)
def case2(L):
    pts, mass = box(N2, 711, L), masses(N2, 712)
    q = np.concatenate([box(M2, 713, L), pts[:M2]])
    return pts, mass, q


@pytest.mark.parametrize("eps", [0.0, 0.01])
@pytest.mark.parametrize("L", [1.0, 7.5])
def test_direct_ewald_sum(gpu, L, eps):
    pts, mass, q = case2(L)
    assert N2 % 8 != 0  # padding points are present
    t = gpu.Tree(pts, leafsize=16, boxsize=L)
    phi, acc = t.gravity_ewald(q, mass, theta=0.0, eps=eps)
    assert phi.dtype == F32 and phi.shape == (2 * M2,)
    assert acc.dtype == F32 and acc.shape == (2 * M2, 3)
    s = direct(pts, mass, q, eps, L, True)
    assert np.all(s.T[:M2] == N2) and np.all(s.T[M2:] == N2 - 1)
    check(phi, acc, s, f"oracle A L {L} eps {eps}", interp=True)
    # and, tighter, the same sum with the table interpolated as stated
    check(phi, acc, direct(pts, mass, q, eps, L, False), f"direct L {L} eps {eps}")
    p1, a1 = t.gravity_ewald(q, None, theta=0.0, eps=eps)
    p2, a2 = t.gravity_ewald(q, np.ones(N2, F32), theta=0.0, eps=eps)
    assert np.array_equal(p1, p2) and np.array_equal(a1, a2)


# ---------------------------------------------------------------- 3. oracle B
N3 = 3000


@functools.lru_cache(maxsize=None)
def case3(dist):
    pts = box(N3, 721) if dist == "uniform" else clumps(N3, 722)
    q = np.concatenate([box(128, 723), pts[:128]])
    return pts, masses(N3, 724), q


@pytest.mark.parametrize("theta", [0.3, 0.6, 0.9])
@pytest.mark.parametrize("leafsize", [16, 64])
@pytest.mark.parametrize("dist", ["uniform", "clumps"])
def test_tree_oracle(gpu, dist, leafsize, theta):
    """Rounding bound only.  A query that opened a node the oracle accepts (or
    the reverse) would differ by that node's monopole remainder, far above the
    bound: agreement of every query is agreement of every opening decision.
    The clumps are small against their distances, so nodes are accepted at
    every theta; a leaf of 16 of 3000 uniform points has a diagonal near 0.3,
    accepted from theta = 0.6 on."""
    pts, mass, q = case3(dist)
    if dist == "clumps":
        near = np.minimum(pts, F32(1.0) - pts).max(axis=1) < 0.06
        lo, hi = pts[near] < 0.5, pts[near] >= 0.5
        assert lo.any(axis=0).all() and hi.any(axis=0).all()  # a clump across the corner
    t = gpu.Tree(pts, leafsize=leafsize, boxsize=1.0)
    exported = t.export()
    for eps in (0.0, 0.01):
        s = tree_walk(exported, N3, mass, q, theta, eps, 1.0)
        if dist == "clumps" or theta >= 0.6:
            assert s.accepted.sum() > 0
        assert s.T.min() > 1  # the root was opened
        print(f"accepted nodes per query {s.accepted.mean():.1f}, terms {s.T.mean():.0f}")
        phi, acc = t.gravity_ewald(q, mass, theta=theta, eps=eps)
        check(phi, acc, s, f"{dist} leaf {leafsize} theta {theta} eps {eps}")


# ---------------------------------------------------------------- 4. Newton's third law
def test_newtons_third_law(gpu):
    """At theta = 0 the terms of a pair are exact negatives (the wrap and the
    interpolation are antisymmetric), so sum m_i a_i = 0 up to the roundings of
    each query's own sum."""
    pts, mass, _ = case2(7.5)
    t = gpu.Tree(pts, leafsize=16, boxsize=7.5)
    phi, acc = t.gravity_ewald(pts, mass, theta=0.0, eps=0.0)
    s = direct(pts, mass, pts, 0.0, 7.5, False)
    bound = check(phi, acc, s, "third law rows")
    m64 = mass.astype(np.float64)
    total = (m64[:, None] * acc.astype(np.float64)).sum(axis=0)
    limit = (m64[:, None] * bound[:, 1:]).sum(axis=0)
    print(f"sum m a = {total}, within {limit}")
    assert np.all(np.abs(total) <= limit)


# ---------------------------------------------------------------- 5. == determinism
N5 = 2003


def test_canonical_order(gpu):
    """Two calls, the build array as device queries (the self-order path), the
    same rows as host queries (bucketed and sorted), and host batches of 64:
    == arrays."""
    from nbodyhpc_amd import hip
    pts, mass = box(N5, 731, 2.5), masses(N5, 732)
    dp, dm = hip.DeviceArray.from_numpy(pts), hip.DeviceArray.from_numpy(mass)
    t = gpu.Tree(n=N5, dev_ptr=dp.ptr, leafsize=16, boxsize=2.5)
    s = hip.Stream()
    gpu.timing_enable(True)
    gpu.timing_reset()
    try:
        runs = []
        for _ in range(2):
            dphi = hip.DeviceArray.from_numpy(np.full(N5, -7.0, F32))
            dacc = hip.DeviceArray.from_numpy(np.full(3 * N5, -7.0, F32))
            t.gravity_ewald_device(dp.ptr, N5, dm.ptr, 0.5, 0.01, dphi.ptr, dacc.ptr,
                                   stream=s.handle)
            s.synchronize()
            runs.append((dphi.numpy(), dacc.numpy().reshape(N5, 3)))
        assert gpu.timing_read("self_order")[1] == 2
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        hphi, hacc = t.gravity_ewald(pts, mass, theta=0.5, eps=0.01)
        assert gpu.timing_read("self_order")[1] == 2
        assert gpu.timing_read("gravity_ewald_walk")[1] == 3
        old = gpu.get_tuning("host_batch")
        try:
            gpu.set_tuning("host_batch", 64)
            bphi, bacc = t.gravity_ewald(pts, mass, theta=0.5, eps=0.01)
        finally:
            gpu.set_tuning("host_batch", old)
        assert gpu.timing_read("gravity_ewald_walk")[1] == 3 + (N5 + 63) // 64
        assert gpu.timing_read("gravity_moments")[1] == 4  # once per call
    finally:
        gpu.timing_enable(False)
    assert np.array_equal(hphi, runs[0][0]) and np.array_equal(hacc, runs[0][1])
    assert np.array_equal(bphi, runs[0][0]) and np.array_equal(bacc, runs[0][1])
    check(hphi, hacc, tree_walk(t.export(), N5, mass, pts, 0.5, 0.01, 2.5), "canonical order")


def test_device_buffers_on_a_stream(gpu):
    """a caller's stream, device buffers between guard words, one output
    against both"""
    from nbodyhpc_amd import hip
    pts, mass = box(N5, 731, 2.5), masses(N5, 732)
    q = np.concatenate([box(300, 733, 2.5), pts[:300]])
    m, guard = len(q), 64
    t = gpu.Tree(pts, leafsize=16, boxsize=2.5)
    dq, dm = hip.DeviceArray.from_numpy(q), hip.DeviceArray.from_numpy(mass)
    s = hip.Stream()

    def run(want_phi, want_acc):
        dphi = hip.DeviceArray.from_numpy(np.full(guard + m + guard, -7.0, F32))
        dacc = hip.DeviceArray.from_numpy(np.full(guard + 3 * m + guard, -7.0, F32))
        t.gravity_ewald_device(dq.ptr, m, dm.ptr, 0.5, 0.01,
                               dphi.ptr + 4 * guard if want_phi else None,
                               dacc.ptr + 4 * guard if want_acc else None, stream=s.handle)
        s.synchronize()
        hp, ha = dphi.numpy(), dacc.numpy()
        assert np.all(hp[:guard] == -7.0) and np.all(hp[guard + m:] == -7.0)
        assert np.all(ha[:guard] == -7.0) and np.all(ha[guard + 3 * m:] == -7.0)
        return hp[guard:guard + m], ha[guard:guard + 3 * m].reshape(m, 3)

    phi, acc = run(True, True)
    check(phi, acc, tree_walk(t.export(), N5, mass, q, 0.5, 0.01, 2.5), "device buffers")
    p_only, untouched = run(True, False)
    assert np.array_equal(p_only, phi) and np.all(untouched == -7.0)
    untouched, a_only = run(False, True)
    assert np.array_equal(a_only, acc) and np.all(untouched == -7.0)
    hphi, hacc = t.gravity_ewald(q, mass, theta=0.5, eps=0.01)
    assert np.array_equal(hphi, phi) and np.array_equal(hacc, acc)
    assert np.array_equal(t.gravity_ewald(q, mass, theta=0.5, eps=0.01, acc=False)[0], phi)
    assert np.array_equal(t.gravity_ewald(q, mass, theta=0.5, eps=0.01, phi=False)[1], acc)


# ---------------------------------------------------------------- 6. edges
def check_tree(gpu, pts, mass, q, L=1.0, leafsize=16, thetas=(0.0, 0.5), eps=(0.0, 0.02), what=""):
    t = gpu.Tree(pts, leafsize=leafsize, boxsize=L)
    exported = t.export()
    for theta in thetas:
        for e in eps:
            s = tree_walk(exported, len(pts), np.ones(len(pts)) if mass is None else mass, q,
                          theta, e, L)
            phi, acc = t.gravity_ewald(q, mass, theta=theta, eps=e)
            check(phi, acc, s, f"{what} theta {theta} eps {e}")
    return t


@pytest.mark.parametrize("m", [1, 63, 65])
def test_small_query_counts(gpu, m):
    pts = box(700, 741)
    check_tree(gpu, pts, masses(700, 742), box(m, 743 + m), what=f"m {m}")


def test_one_point(gpu):
    """another query sees the point and all its images; the point itself
    nothing (its own images' constant is left out)"""
    pts = box(1, 751)
    t = check_tree(gpu, pts, np.array([1.25], F32), box(5, 752), what="n 1")
    for theta in (0.0, 0.5):
        phi, acc = t.gravity_ewald(pts, np.array([1.25], F32), theta=theta, eps=0.1)
        assert np.all(phi == 0) and np.all(acc == 0)


def test_seventeen_points(gpu):
    pts = box(17, 753, 3.0)
    check_tree(gpu, pts, masses(17, 754), np.concatenate([box(30, 755, 3.0), pts]), L=3.0,
               what="n 17")


def test_all_points_coincident(gpu):
    p = np.array([[0.125, 0.75, 0.375]], F32)
    pts = np.repeat(p, 40, axis=0)
    mass = masses(40, 756)
    t = check_tree(gpu, pts, mass, box(9, 757), what="coincident")
    for theta in (0.0, 0.5):
        for eps in (0.0, 0.05):
            phi, acc = t.gravity_ewald(pts, mass, theta=theta, eps=eps)
            assert np.all(phi == 0) and np.all(acc == 0)


def test_zero_mass_subset(gpu):
    pts = box(900, 761)
    mass = masses(900, 762)
    mass[np.random.default_rng(763).random(900) < 0.3] = 0.0
    order = np.argsort(pts[:, 0], kind="stable")
    mass[order[:130]] = 0.0  # whole leaves, and nodes above them, without mass
    q = np.concatenate([box(60, 764), pts[:100]])
    check_tree(gpu, pts, mass, q, thetas=(0.0, 0.4, 0.8), eps=(0.0,), what="zero masses")


def test_two_staged_chunks_per_leaf(gpu):
    pts = box(1500, 765)
    q = np.concatenate([box(60, 766), pts[:60]])
    check_tree(gpu, pts, masses(1500, 767), q, leafsize=128, thetas=(0.0, 0.6), eps=(0.01,),
               what="leaf 128")


def test_replaced_ids(gpu):
    """After nbkd_set_ids the masses are still indexed by input row."""
    n = 1500
    pts, mass = box(n, 771), masses(n, 772)
    q = np.concatenate([box(100, 773), pts[:100]])
    t = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    exported = t.export()  # the build's permutation
    before = t.gravity_ewald(q, mass, theta=0.5, eps=0.01)
    t.set_ids((np.random.default_rng(774).permutation(n) + 1_000_000).astype(np.uint32))
    after = t.gravity_ewald(q, mass, theta=0.5, eps=0.01)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    check(after[0], after[1], tree_walk(exported, n, mass, q, 0.5, 0.01, 1.0), "replaced ids")


@pytest.mark.parametrize("L", [1.0, 6.0])
def test_pair_half_a_box_apart(gpu, L):
    """Two points exactly L/2 apart on x: each lies between two images of the
    other, so the acceleration along x vanishes by symmetry (the Newtonian term
    of the image the tie picks is cancelled by the table's value at x = 1/2)."""
    pts = np.array([[0.25 * L, 0.5 * L, 0.125 * L], [0.75 * L, 0.5 * L, 0.125 * L]], F32)
    assert pts[1, 0] - pts[0, 0] == F32(0.5 * L)
    mass = np.array([1.5, 0.75], F32)
    t = gpu.Tree(pts, leafsize=16, boxsize=L)
    phi, acc = t.gravity_ewald(pts, mass, theta=0.0, eps=0.0)
    s = direct(pts, mass, pts, 0.0, L, False)
    bound = check(phi, acc, s, f"half a box L {L}")
    assert np.all(np.isfinite(phi)) and np.all(np.isfinite(acc))
    assert np.all(np.abs(acc.astype(np.float64)[:, 0]) <= bound[:, 1])


# ---------------------------------------------------------------- 7. outside queries
def test_outside_queries(gpu):
    """a query outside [0, L]^3 or NaN gets NaN rows; its neighbours in the
    packet are unchanged"""
    L = 2.0
    pts, mass = box(700, 781, L), masses(700, 782)
    q = np.concatenate([box(40, 783, L), pts[:30]])
    t = gpu.Tree(pts, leafsize=16, boxsize=L)
    phi0, acc0 = t.gravity_ewald(q, mass, theta=0.5, eps=0.01)
    bad = {5: (-0.1, 1.0, 1.0), 17: (1.0, L * 1.5, 1.0), 33: (1.0, 1.0, float("nan")),
           69: (float("nan"),) * 3}
    q2 = q.copy()
    for row, v in bad.items():
        q2[row] = v
    phi, acc = t.gravity_ewald(q2, mass, theta=0.5, eps=0.01)
    rows = np.array(sorted(bad))
    good = np.setdiff1d(np.arange(len(q)), rows)
    assert np.all(np.isnan(phi[rows])) and np.all(np.isnan(acc[rows]))
    assert np.array_equal(phi[good], phi0[good]) and np.array_equal(acc[good], acc0[good])
    only = t.gravity_ewald(q2, mass, theta=0.5, eps=0.01, acc=False)[0]
    assert np.array_equal(only, phi, equal_nan=True)
    # a query on the face x = L is inside
    edge = np.array([[L, 0.0, 1.0]], F32)
    pe, ae = t.gravity_ewald(edge, mass, theta=0.5, eps=0.01)
    assert np.all(np.isfinite(pe)) and np.all(np.isfinite(ae))
    check(pe, ae, tree_walk(t.export(), 700, mass, edge, 0.5, 0.01, L), "query on a face")


# ---------------------------------------------------------------- 8. rejections
def test_rejections_on_live_trees(gpu):
    pts = box(500, 791)
    q = np.ascontiguousarray(pts[:8])
    phi, acc = np.full(8, 77.0, F32), np.full((8, 3), 77.0, F32)

    def call(fn, t, theta, eps):
        st = fn(t.h, q.ctypes.data, 8, None, ctypes.c_float(theta), ctypes.c_float(eps),
                phi.ctypes.data, acc.ctypes.data, 0, None)
        return st, gpu.lib().nbkd_last_error()

    ewald, plain = gpu.lib().nbkd_gravity_ewald, gpu.lib().nbkd_gravity
    flat = gpu.Tree(pts, leafsize=16)
    st, msg = call(ewald, flat, 0.5, 0.0)
    assert st == gpu.NBKD_EINVAL and b"periodic" in msg and b"nbkd_gravity " in msg
    with pytest.raises(gpu.NbkdError) as e:
        flat.gravity_ewald(q)
    assert e.value.status == gpu.NBKD_EINVAL
    per = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    for theta, eps, word in ((1.0, 0.0, b"theta"), (0.5, -1.0, b"eps")):
        st, msg = call(ewald, per, theta, eps)
        assert st == gpu.NBKD_EINVAL and word in msg
    # the old call still refuses the periodic tree
    st, msg = call(plain, per, 0.5, 0.0)
    assert st == gpu.NBKD_EINVAL and b"Ewald" in msg
    assert np.all(phi == 77.0) and np.all(acc == 77.0)
    st, _ = call(ewald, per, 0.5, 0.0)
    assert st == gpu.NBKD_OK and np.all(phi != 77.0) and np.all(np.isfinite(acc))


# ---------------------------------------------------------------- 9. Python surface
def test_python_surface(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    L = 7.5
    pts, mass, q = case2(L)
    t = KDTree(pts, leafsize=16, boxsize=L)
    s = direct(pts, mass, q, 0.01, L, False)
    G = 4.30091e-6
    phi, acc = t.gravity_ewald(q, mass, softening=0.01, theta=0.0, G=G)
    assert phi.dtype == np.float64 and phi.shape == (2 * M2,)
    assert acc.dtype == np.float64 and acc.shape == (2 * M2, 3)
    check(phi / G, acc / G, s, "KDTree.gravity_ewald")
    p = t.potential_ewald(q.reshape(2, M2, 3), mass, softening=0.01, theta=0.0)
    assert p.shape == (2, M2) and np.array_equal(p.reshape(-1) * G, phi)
    only_a = t.gravity_ewald(q, mass, softening=0.01, theta=0.0, potential=False)
    assert only_a[0] is None and np.array_equal(only_a[1] * G, acc)
    # points outside the box are their wrapped copies (exact shifts in float64)
    shift = np.random.default_rng(795).integers(-2, 3, q.shape) * L
    moved = q.astype(np.float64) + shift
    assert (moved < 0).any() and (moved >= L).any()
    p2, a2 = t.gravity_ewald(moved, mass, softening=0.01, theta=0.0, G=G)
    assert np.array_equal(p2, phi) and np.array_equal(a2, acc)
    # points=None: the tree's own points, unit masses
    phi0, acc0 = t.gravity_ewald(theta=0.5)
    assert phi0.shape == (N2,) and acc0.shape == (N2, 3)
    nodes, x, y, z, idx = t.export()
    nd = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4)
    rec = np.zeros(len(nd), gpu.NODE_DTYPE)
    rec["dim"], rec["split"] = nd[:, 0].view(np.int32), nd[:, 1].view(np.float32)
    rec["left"], rec["right"] = nd[:, 2], nd[:, 3]
    check(phi0, acc0, tree_walk((rec, x, y, z, idx), N2, np.ones(N2), pts, 0.5, 0.0, L),
          "KDTree.gravity_ewald own points")
    assert np.array_equal(t.potential_ewald(), phi0)
    with pytest.raises(ValueError, match="periodic"):
        KDTree(pts, leafsize=16).gravity_ewald()
    with pytest.raises(ValueError, match="periodic"):
        KDTree(pts, leafsize=16).potential_ewald()
