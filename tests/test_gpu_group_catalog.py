"""Group catalogue (nbkd_group_catalog, group.hip): heads, sizes, member lists
and float64 moments of the kept groups of a canonical labelling.

Oracle: plain numpy.  The rows are grouped with a stable argsort of the labels
(groups by ascending head, rows ascending inside each); the terms are the
header's expressions: float32 offsets from the head's position (on a periodic
tree the first of d, fl(d - L), fl(d + L) with the smallest magnitude), every
product in float64.  Each group's terms are summed with np.add.reduceat
(np.sum per segment).

Tolerance (derived, not measured): any order of summing m float64 terms t_i
errs by at most (m - 1) * 2^-53 * sum |t_i|; the device and the oracle each stay
within that, so they differ by less than size * 2^-52 * sum |t_i| per group and
component, which is what the tests allow.  head, size, offsets, members and
dmax are compared with ==.  New (no reference counterpart)."""
import ctypes
import functools

import numpy as np
import pytest

from tests.golden.inputs import uniform

pytestmark = pytest.mark.gpu

SIZES = (1, 1, 2, 63, 64, 65, 255, 256, 257, 513)


def crafted_labels(n, sizes, seed):
    """Rows in a shuffled order dealt to groups of the given sizes, singletons
    for the rest; each label is the smallest row of its group."""
    order = np.random.default_rng(seed).permutation(n)
    lab = np.arange(n, dtype=np.uint32)
    at = 0
    for s in sizes:
        rows = order[at:at + s]
        lab[rows] = rows.min()
        at += s
    assert at <= n
    return lab


def oracle(pts, box, lab, mm=1, weight=None, values=None):
    """(head, size, offsets, members, moments, dmax, abs) with abs[g, c] =
    sum |t_i| of group g's component c."""
    pts = np.asarray(pts, np.float32)
    lab = np.asarray(lab, np.uint32)
    n = len(pts)
    order = np.argsort(lab, kind="stable")
    heads, start, cnt = np.unique(lab[order], return_index=True, return_counts=True)
    keep = cnt >= max(int(mm), 1)
    nv = 0 if values is None else np.asarray(values).reshape(n, -1).shape[1]
    nt = 5 + 2 * nv
    head, size = heads[keep].astype(np.uint32), cnt[keep].astype(np.uint32)
    G = len(head)
    off = np.zeros(G + 1, np.uint64)
    np.cumsum(size, out=off[1:])
    if G == 0:
        return (head, size, off, np.empty(0, np.uint32), np.empty((0, nt)),
                np.empty(0, np.float32), np.empty((0, nt)))
    rows = np.concatenate([order[s:s + c] for s, c in zip(start[keep], cnt[keep])])
    d = pts[rows] - pts[lab[rows]]  # float32
    assert d.dtype == np.float32
    if box is not None:
        L = np.float32(box)
        dm, dp = d - L, d + L
        r = d.copy()
        r = np.where(np.abs(dm) < np.abs(r), dm, r)
        r = np.where(np.abs(dp) < np.abs(r), dp, r)
        d = r.astype(np.float32)
    w = np.ones(len(rows)) if weight is None else np.asarray(weight, np.float32)[rows].astype(np.float64)
    x, y, z = (d[:, a].astype(np.float64) for a in range(3))
    terms = [w, w * x, w * y, w * z, w * ((x * x + y * y) + z * z)]
    if nv:
        v = np.asarray(values, np.float32).reshape(n, -1)[rows].astype(np.float64)
        terms += [w * v[:, c] for c in range(nv)]
        terms += [w * (v[:, c] * v[:, c]) for c in range(nv)]
    t = np.stack(terms, axis=1)
    seg = off[:-1].astype(np.int64)
    mom = np.add.reduceat(t, seg, axis=0)
    ab = np.add.reduceat(np.abs(t), seg, axis=0)
    dmax = np.maximum.reduceat(np.abs(d).max(axis=1), seg).astype(np.float32)
    return head, size, off, rows.astype(np.uint32), mom, dmax, ab


def compare(got, ref, exact=False):
    head, size, off, mem, mom, dmax = got
    rhead, rsize, roff, rmem, rmom, rdmax, rabs = ref
    assert head.dtype == np.uint32 and size.dtype == np.uint32 and mem.dtype == np.uint32
    assert off.dtype == np.uint64 and mom.dtype == np.float64 and dmax.dtype == np.float32
    assert np.array_equal(head, rhead)
    assert np.array_equal(size, rsize)
    assert np.array_equal(off, roff)
    assert np.array_equal(mem, rmem)
    assert np.array_equal(dmax, rdmax)
    assert mom.shape == rmom.shape
    if exact:
        assert np.array_equal(mom, rmom)
        return
    bound = rsize.astype(np.float64)[:, None] * 2.0 ** -52 * rabs
    err = np.abs(mom - rmom)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"G = {len(head)}, K = {len(mem)}, largest {rsize.max() if len(rsize) else 0}, "
          f"worst error / bound = {worst:.3g}")
    bad = np.argwhere(err > bound)
    assert bad.size == 0, f"{len(bad)} sums beyond the bound, first {bad[:3]}: " \
                          f"{mom[tuple(bad[0])]} vs {rmom[tuple(bad[0])]}"


# ---------------------------------------------------------------- 1. crafted labels on boundaries
N1 = 2000


@functools.lru_cache(maxsize=None)
def case1():
    rng = np.random.default_rng(502)
    pts = uniform(N1, 501)
    lab = crafted_labels(N1, SIZES, 503)
    w = (0.5 + rng.random(N1)).astype(np.float32)
    v = rng.normal(size=(N1, 3)).astype(np.float32)
    return pts, lab, w, v


@pytest.mark.parametrize("mm", [1, 2, 64, 65, 514])
def test_crafted_labels_on_boundaries(gpu, mm):
    """Groups of 1, 2, 63..65, 255..257 and 513 rows: segments that end on,
    one before and one after the 64-lane and 256-thread boundaries, and one
    that crosses eight waves."""
    pts, lab, w, v = case1()
    t = gpu.Tree(pts, leafsize=32)
    got = t.group_catalog(lab, mm, weight=w, values=v)
    ref = oracle(pts, None, lab, mm, w, v)
    if mm == 514:
        assert len(ref[0]) == 0 and len(ref[3]) == 0
        assert len(got[0]) == 0 and len(got[3]) == 0 and got[4].shape == (0, 11)
    if mm == 1:
        assert len(got[0]) == len(np.unique(lab)) and len(got[3]) == N1
    compare(got, ref)


# ---------------------------------------------------------------- 2. exact case
@pytest.mark.parametrize("box", [None, 1.0])
def test_exact_sums_on_the_dyadic_lattice(gpu, box):
    """The 16^3 lattice i/16, rows shuffled, unit weights, small-integer
    values: every term and every partial sum is exactly representable, so the
    moments equal the oracle's under == whatever the summation order."""
    g = np.arange(16, dtype=np.float32) / np.float32(16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = pts[np.random.default_rng(402).permutation(len(pts))]
    n = len(pts)
    lab = crafted_labels(n, SIZES + (1024, 1025), 504)
    v = np.random.default_rng(505).integers(-7, 8, size=(n, 2)).astype(np.float32)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for mm in (1, 64):
        got = t.group_catalog(lab, mm, weight=None, values=v)
        compare(got, oracle(pts, box, lab, mm, None, v), exact=True)
        assert np.array_equal(got[4][:, 0], got[1].astype(np.float64))


# ---------------------------------------------------------------- 3. real groups
N3 = 6000
S3 = N3 ** (-1.0 / 3.0)


@functools.lru_cache(maxsize=None)
def case3():
    rng = np.random.default_rng(506)
    return (uniform(N3, 401), (0.5 + rng.random(N3)).astype(np.float32),
            rng.normal(size=(N3, 3)).astype(np.float32))


@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("f", [0.5, 0.87])
def test_real_groups(gpu, f, box):
    """Friends-of-friends labels: many small groups (f = 0.5) and the
    percolation threshold (f = 0.87: the largest group has 385 / 741 members
    and crosses several 64- and 256-member boundaries).  Raw sums and dmax
    only: at f = 0.87 periodic groups may span the box."""
    pts, w, v = case3()
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    lab, siz, ng = t.fof(f * S3)
    if f == 0.87:
        assert int(siz.max()) == (741 if box else 385)
    for mm in (1, 5):
        got = t.group_catalog(lab, mm, weight=w, values=v)
        ref = oracle(pts, box, lab, mm, w, v)
        compare(got, ref)
        if mm == 1:
            assert len(got[0]) == ng
            assert np.array_equal(got[1], siz[siz > 0])


# ---------------------------------------------------------------- 4. one group and none
def test_one_group_and_none(gpu):
    """n = 20001 (padded to 20008).  One group of every row: 313 waves'
    partials go through the combine kernel.  Then n singletons, and
    min_members = 2 of them: nothing is kept."""
    n = 20001
    rng = np.random.default_rng(507)
    pts = uniform(n, 508)
    w = (0.5 + rng.random(n)).astype(np.float32)
    v = rng.normal(size=(n, 4)).astype(np.float32)
    t = gpu.Tree(pts, leafsize=32)
    lab = np.zeros(n, np.uint32)
    got = t.group_catalog(lab, 1, weight=w, values=v)
    assert len(got[0]) == 1 and np.array_equal(got[3], np.arange(n))
    compare(got, oracle(pts, None, lab, 1, w, v))
    lab = np.arange(n, dtype=np.uint32)
    got = t.group_catalog(lab, 1, weight=w, values=v)
    assert len(got[0]) == n and np.all(got[5] == 0)
    compare(got, oracle(pts, None, lab, 1, w, v))
    got = t.group_catalog(lab, 2, weight=w, values=v)
    assert all(len(got[j]) == 0 for j in (0, 1, 3, 4, 5)) and np.array_equal(got[2], [0])


# ---------------------------------------------------------------- 5. periodic unwrapping
def test_periodic_unwrapping_by_construction(gpu):
    """Five points across the x = 0 face are one compact group about x = 0;
    a chain along the whole box spans it."""
    from nbodyhpc_amd.kdtree import KDTree
    a = np.array([[x, 0.5, 0.5] for x in (0.98, 0.99, 0.0, 0.01, 0.02)], np.float32)
    chain = np.stack([np.arange(100) / 100.0, np.full(100, 0.25), np.full(100, 0.75)], -1)
    pts = np.concatenate([a, chain.astype(np.float32), uniform(200, 509)])
    n = len(pts)
    lab = np.arange(n, dtype=np.uint32)
    lab[:5] = 0
    lab[5:105] = 5
    t = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    got = t.group_catalog(lab, 5)
    compare(got, oracle(pts, 1.0, lab, 5))
    assert np.array_equal(got[0], [0, 5]) and np.array_equal(got[1], [5, 100])
    assert got[5][0] < 0.5 and got[5][1] >= 0.5
    kt = KDTree(pts, leafsize=16, boxsize=1.0)
    cat = kt.fof_catalog(None, labels=lab, min_members=5)
    assert np.array_equal(cat["head"], [5, 0]) and np.array_equal(cat["size"], [100, 5])
    c = cat["center"][1]
    assert min(c[0], 1.0 - c[0]) < 1e-6 and 0.0 <= c[0] < 1.0
    assert abs(c[1] - 0.5) < 1e-6 and abs(c[2] - 0.5) < 1e-6
    assert np.array_equal(cat["spans_box"], [True, False])
    assert np.array_equal(cat["mass"], [100.0, 5.0])
    # the same labels on a non-periodic tree: nothing spans a box
    cat = KDTree(pts, leafsize=16).fof_catalog(None, labels=lab, min_members=5)
    assert not cat["spans_box"].any()
    assert abs(cat["center"][1][0] - 0.4) < 1e-6


# ---------------------------------------------------------------- 6 / 7. invalid labels, capacity
class Outputs:
    """Sentinel-filled host outputs of a raw call."""

    def __init__(self, G, K, nt):
        self.ng, self.nm = ctypes.c_uint64(77), ctypes.c_uint64(77)
        self.head = np.full(G, 77, np.uint32)
        self.size = np.full(G, 77, np.uint32)
        self.off = np.full(G + 1, 77, np.uint64)
        self.mem = np.full(K, 77, np.uint32)
        self.mom = np.full((G, nt), 77.0)
        self.dmax = np.full(G, 77.0, np.float32)

    def call(self, gpu, t, lab, mm, gcap, mcap):
        lab = np.ascontiguousarray(lab, np.uint32)
        return gpu.lib().nbkd_group_catalog(
            t.h, lab.ctypes.data, None, None, 0, mm, gcap, mcap, ctypes.byref(self.ng),
            ctypes.byref(self.nm), self.head.ctypes.data, self.size.ctypes.data,
            self.off.ctypes.data, self.mem.ctypes.data, self.mom.ctypes.data,
            self.dmax.ctypes.data, 0, None)

    def untouched(self):
        return all(bool(np.all(x == 77)) for x in (self.head, self.size, self.off, self.mem,
                                                   self.mom, self.dmax))


def test_invalid_labels(gpu):
    n = 1000
    t = gpu.Tree(uniform(n, 510), leafsize=16)
    good = crafted_labels(n, (3, 70, 200), 511)
    one = good.copy()
    one[17] = n  # out of range
    chain = np.arange(n, dtype=np.uint32)
    chain[900], chain[800] = 800, 700  # label[900] = 800 but label[800] = 700
    for lab in (one, chain):
        o = Outputs(n, n, 5)
        st = o.call(gpu, t, lab, 1, n, n)
        assert st == gpu.NBKD_EINVAL
        assert b"canonical" in gpu.lib().nbkd_last_error()
        assert o.ng.value == 0 and o.nm.value == 0 and o.untouched()
        with pytest.raises(gpu.NbkdError) as e:
            t.group_catalog(lab)
        assert e.value.status == gpu.NBKD_EINVAL
    # the tree still answers
    o = Outputs(n, n, 5)
    assert o.call(gpu, t, good, 1, n, n) == gpu.NBKD_OK
    assert o.ng.value == n - 270 and o.nm.value == n


def test_capacity(gpu):
    pts, lab, _, _ = case1()
    t = gpu.Tree(pts, leafsize=32)
    ref = oracle(pts, None, lab, 2)
    G, K = len(ref[0]), len(ref[3])
    assert G == 8 and K == sum(SIZES) - 2
    for gcap, mcap in ((G - 1, K), (G, K - 1), (0, 0)):
        o = Outputs(G, K, 5)
        assert o.call(gpu, t, lab, 2, gcap, mcap) == gpu.NBKD_OK
        assert o.ng.value == G and o.nm.value == K and o.untouched()
    o = Outputs(G, K, 5)
    assert o.call(gpu, t, lab, 2, G, K) == gpu.NBKD_OK
    assert o.ng.value == G and o.nm.value == K
    compare((o.head, o.size, o.off, o.mem, o.mom, o.dmax), ref)
    # min_members = 0 is 1
    a, b = t.group_catalog(lab, 0), t.group_catalog(lab, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 8. determinism, independence
def test_determinism_and_independence(gpu):
    """Equal under ==: a second call, trees with other leaf sizes, the
    device-in / device-out call, a tree with replaced ids.  Device buffers
    are raw HIP allocations (nbodyhpc_amd.hip): a process that drives libnbkd
    cannot also initialise torch.cuda (see nbodyhpc_amd/hip.py)."""
    from nbodyhpc_amd import hip
    pts, w, v = case3()
    box = 1.0
    lab = gpu.Tree(pts, leafsize=32, boxsize=box).fof(0.87 * S3)[0]
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    first = t.group_catalog(lab, 2, weight=w, values=v)
    G, K = len(first[0]), len(first[3])
    assert int(first[1].max()) == 741

    def same(other):
        return all(np.array_equal(x, y) for x, y in zip(first, other))

    assert same(t.group_catalog(lab, 2, weight=w, values=v))
    for leaf in (16, 128):
        assert same(gpu.Tree(pts, leafsize=leaf, boxsize=box).group_catalog(lab, 2, weight=w,
                                                                         values=v))
    # device in, device out
    dl, dw, dv = (hip.DeviceArray.from_numpy(x) for x in (lab, w, v))
    nt = 5 + 2 * v.shape[1]
    guard = 16
    dh = hip.DeviceArray.from_numpy(np.full(G + guard, 0xDEADBEEF, np.uint32))
    ds = hip.DeviceArray.from_numpy(np.full(G + guard, 0xDEADBEEF, np.uint32))
    do = hip.DeviceArray.from_numpy(np.full(G + 1 + guard, 77, np.uint64))
    dm = hip.DeviceArray.from_numpy(np.full(K + guard, 0xDEADBEEF, np.uint32))
    dq = hip.DeviceArray.from_numpy(np.full((G + guard, nt), 77.0))
    dx = hip.DeviceArray.from_numpy(np.full(G + guard, 77.0, np.float32))
    assert t.group_catalog_device(dl.ptr, dw.ptr, dv.ptr, v.shape[1], 2, 0, 0) == (G, K)
    assert t.group_catalog_device(dl.ptr, dw.ptr, dv.ptr, v.shape[1], 2, G, K, dh.ptr, ds.ptr,
                                  do.ptr, dm.ptr, dq.ptr, dx.ptr) == (G, K)
    hip.synchronize()
    outs = [a.numpy() for a in (dh, ds, do, dm, dq, dx)]
    lens = (G, G, G + 1, K, G, G)
    assert same([o[:m] for o, m in zip(outs, lens)])
    for o, m, fill in zip(outs, lens, (0xDEADBEEF, 0xDEADBEEF, 77, 0xDEADBEEF, 77.0, 77.0)):
        assert np.all(o[m:] == fill)  # nothing past the ends
    # moments alone on a stream of the caller's
    s = hip.Stream()
    dq2 = hip.DeviceArray.from_numpy(np.full((G, nt), 77.0))
    t.group_catalog_device(dl.ptr, dw.ptr, dv.ptr, v.shape[1], 2, G, K, moments_ptr=dq2.ptr,
                           stream=s.handle)
    assert np.array_equal(dq2.numpy(), first[4])
    # replaced ids: labels and members are still input rows
    ids = (np.random.default_rng(512).permutation(N3) + 1_000_000).astype(np.uint32)
    t.set_ids(ids)
    assert same(t.group_catalog(lab, 2, weight=w, values=v))


# ---------------------------------------------------------------- 9. Python surface
def test_python_surface(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    pts, m, v = case3()
    b = 0.5 * S3
    t = KDTree(pts, leafsize=32, boxsize=1.0)
    cat = t.fof_catalog(b, min_members=5, mass=m, values=v, members=True)
    group, sizes = t.fof(b, 5, return_sizes=True)
    G = len(sizes)
    assert G > 10
    assert np.array_equal(cat["size"], sizes)
    off = cat["offsets"]
    assert off.dtype == np.uint64 and off.shape == (G + 1,) and off[-1] == sizes.sum()
    m64, v64 = m.astype(np.float64), v.astype(np.float64)
    for g in range(G):
        rows = np.flatnonzero(group == g)
        assert np.array_equal(cat["members"][int(off[g]):int(off[g + 1])], rows)
        assert cat["head"][g] == rows[0]
        mass = m64[rows].sum()
        mean = (m64[rows, None] * v64[rows]).sum(axis=0) / mass
        var = (m64[rows, None] * v64[rows] ** 2).sum(axis=0) / mass - mean ** 2
        assert abs(cat["mass"][g] - mass) <= 1e-9 * mass
        assert np.all(np.abs(cat["mean"][g] - mean) <= 1e-9 * np.abs(mean))
        # (away from the cancellation region of sum w v^2 / sum w - mean^2)
        ok = var > 1e-6 * mean ** 2
        assert np.all(np.abs(cat["dispersion"][g][ok] - np.sqrt(var[ok])) <= 1e-9 * np.sqrt(var[ok]))
    assert cat["center"].shape == (G, 3) and cat["center"].dtype == np.float64
    assert np.all((cat["center"] >= 0) & (cat["center"] < 1.0))
    assert cat["rms_radius"].shape == (G,) and np.all(cat["rms_radius"] > 0)
    assert cat["spans_box"].dtype == bool and not cat["spans_box"].any()
    # without members, and with the labels passed in: the same catalogue
    lab, _ = t.fof_labels(b)
    cat2 = t.fof_catalog(None, min_members=5, mass=m, values=v, labels=lab)
    assert "members" not in cat2 and "offsets" not in cat2
    for k in cat2:
        assert np.array_equal(cat2[k], cat[k]), k
