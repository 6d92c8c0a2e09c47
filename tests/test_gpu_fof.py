"""Friends-of-friends groups (nbkd_fof, fof.hip): points i and j are friends
iff d2(i, j) <= b*b in the tree's f32 metric, groups are the connected
components, a point's label is the smallest input row of its group.  The
labelling is canonical, so every comparison here is exact equality, against a
brute force in plain numpy: the f32 distances of tests.parity.d2_ref in row
blocks, then min-label propagation with pointer jumping to a fixed point.  New
(no reference counterpart: the reference has no group finder)."""
import functools

import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import d2_ref

pytestmark = pytest.mark.gpu


def brute_labels(pts, b, box):
    """labels[i] = the smallest row of i's friends-of-friends group."""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    thr = np.float32(b) * np.float32(b)
    adj = np.empty((n, n), bool)
    for a in range(0, n, 500):
        adj[a:a + 500] = d2_ref(pts[a:a + 500, None, :], pts[None, :, :], box) <= thr
    assert np.array_equal(adj, adj.T)  # the metric is symmetric bit for bit
    lab = np.arange(n, dtype=np.int64)
    sparse = int(adj.sum()) <= 4_000_000
    if sparse:
        ei, ej = np.nonzero(adj)
    while True:
        if sparse:
            m = lab.copy()
            np.minimum.at(m, ei, lab[ej])
        else:
            m = np.where(adj, lab[None, :], n).min(axis=1)
        m = m[m]  # pointer jumping (m[x] <= x is a member of x's group)
        if np.array_equal(m, lab):
            return lab.astype(np.uint32)
        lab = m


def check(gpu, t, pts, b, box, ref=None):
    """labels, sizes and ngroups of the host-output call against the brute force"""
    n = len(pts)
    ref = brute_labels(pts, b, box) if ref is None else ref
    lab, siz, ng = t.fof(b)
    assert lab.dtype == np.uint32 and lab.shape == (n,)
    assert siz.dtype == np.uint32 and siz.shape == (n,)
    bad = np.flatnonzero(lab != ref)
    assert bad.size == 0, f"{bad.size} labels differ, first rows {bad[:5]}: {lab[bad[:5]]} vs {ref[bad[:5]]}"
    assert np.array_equal(siz, np.bincount(ref, minlength=n).astype(np.uint32))
    assert int(siz.sum(dtype=np.uint64)) == n
    assert ng == np.count_nonzero(siz) == len(np.unique(ref))
    lab2, siz2, ng2 = t.fof(b, sizes=False)
    assert siz2 is None and ng2 == ng and np.array_equal(lab2, lab)
    return lab, siz, ng


# ---------------------------------------------------------------- 1. both metrics, three regimes
N1 = 6000
S1 = N1 ** (-1.0 / 3.0)
CASE1 = {  # b / s -> ((groups, largest) non-periodic, (groups, largest) periodic)
    0.2: ((5904, 3), (5902, 3)),
    0.5: ((4587, 8), (4552, 8)),
    0.87: ((921, 385), (712, 741)),
    1.2: ((21, 5972), (5, 5993)),
}


@functools.lru_cache(maxsize=None)
def ref1(f, box):
    return brute_labels(uniform(N1, 401), f * S1, box)


@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("f", sorted(CASE1))
def test_both_metrics_three_regimes(gpu, f, box):
    """Isolated pairs, small groups, the percolation threshold (heavy CAS
    contention) and one giant group; the table is what the brute force gives."""
    pts = uniform(N1, 401)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    lab, siz, ng = check(gpu, t, pts, f * S1, box, ref1(f, box))
    groups, largest = CASE1[f][1 if box else 0]
    print(f"b = {f} s, box {box}: {ng} groups, largest {siz.max()}")
    assert ng == groups
    assert int(siz.max()) == largest
    # links through the faces are exercised: the two partitions differ
    assert not np.array_equal(ref1(f, None), ref1(f, 1.0))


# ---------------------------------------------------------------- 2. exact threshold ties
@pytest.mark.parametrize("leaf", [16, 64])
@pytest.mark.parametrize("box", [None, 1.0])
def test_threshold_ties(gpu, box, leaf):
    """The 16^3 dyadic lattice i/16, rows shuffled: every nearest-neighbour
    pair sits exactly on d2 == b*b at b = 1/16, and one step below nothing
    links."""
    g = np.arange(16, dtype=np.float32) / np.float32(16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = pts[np.random.default_rng(402).permutation(len(pts))]
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    b = np.float32(1 / 16)
    lab, siz, ng = t.fof(b)
    assert ng == 1 and np.all(lab == 0) and siz[0] == 4096 and not siz[1:].any()
    lab, siz, ng = t.fof(np.nextafter(b, np.float32(0)))
    assert ng == 4096 and np.array_equal(lab, np.arange(4096)) and np.all(siz == 1)


# ---------------------------------------------------------------- 3. long chain
def test_long_chain(gpu):
    """1000 points on a line, spacing exactly b, shuffled: the chain crosses
    about 60 leaves and falls apart if a single hook is lost."""
    i = np.arange(1000, dtype=np.float32)
    pts = np.stack([i / np.float32(64), np.full(1000, 0.5, np.float32),
                    np.full(1000, 0.25, np.float32)], -1)
    pts = pts[np.random.default_rng(403).permutation(1000)]
    t = gpu.Tree(pts, leafsize=16)
    b = np.float32(1 / 64)
    lab, siz, ng = t.fof(b)
    assert ng == 1 and np.all(lab == 0) and siz[0] == 1000
    lab, siz, ng = t.fof(np.nextafter(b, np.float32(0)))
    assert ng == 1000 and np.array_equal(lab, np.arange(1000))


# ---------------------------------------------------------------- 4. whole-leaf path and the face
def two_balls():
    rng = np.random.default_rng(7)

    def ball(c):
        v = rng.normal(size=(3000, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return np.asarray(c) + v * (0.01 * rng.random(3000) ** (1 / 3))[:, None]

    first = ball((0.0, 0.5, 0.5)) % 1.0
    second = ball((0.4, 0.5, 0.5))
    return np.clip(np.concatenate([first, second]).astype(np.float32), 0.0, 1.0)


@pytest.mark.parametrize("box", [None, 1.0])
def test_whole_leaf_path_and_the_face(gpu, box):
    """Two balls of radius 0.01, b = 0.05: leaf boxes are far smaller than b,
    so nearly every pair takes the whole-leaf branch; one ball straddles the
    x = 0 face and is one group only on the periodic tree."""
    pts = two_balls()
    t = gpu.Tree(pts, leafsize=64, boxsize=box)
    lab, siz, ng = check(gpu, t, pts, 0.05, box)
    members = sorted(siz[siz > 0].tolist(), reverse=True)
    print(f"box {box}: groups {members}")
    if box:
        assert ng == 2 and members == [3000, 3000]
    else:
        assert ng == 3 and members == [3000, 1543, 1457]


# ---------------------------------------------------------------- 5. padding
@pytest.mark.parametrize("n", [1, 9, 63, 1003])
def test_padding(gpu, n):
    """Tiny trees padded to a multiple of 8 with FLT_MAX points: they are in
    no group, and nothing at an index >= n is written (guard words after the
    device outputs stay intact)."""
    from nbodyhpc_amd import hip
    pts = uniform(n, 304)
    t = gpu.Tree(pts, leafsize=16)
    lab, siz, ng = t.fof(2.0)
    assert ng == 1 and np.all(lab == 0) and siz[0] == n and not siz[1:].any()
    lab, siz, ng = t.fof(0.0)
    assert ng == n and np.array_equal(lab, np.arange(n)) and np.all(siz == 1)
    guard = 64
    for b in (2.0, 0.0, 0.05):
        dl = hip.DeviceArray.from_numpy(np.full(n + guard, 0xDEADBEEF, np.uint32))
        dz = hip.DeviceArray.from_numpy(np.full(n + guard, 0xDEADBEEF, np.uint32))
        t.fof_device(b, dl.ptr, dz.ptr)
        hip.synchronize()
        hl, hz = dl.numpy(), dz.numpy()
        assert np.all(hl[n:] == 0xDEADBEEF) and np.all(hz[n:] == 0xDEADBEEF)
        ref_l, ref_z, _ = t.fof(b)
        assert np.array_equal(hl[:n], ref_l) and np.array_equal(hz[:n], ref_z)
        assert np.array_equal(ref_l, brute_labels(pts, b, None))


# ---------------------------------------------------------------- 6. coincident points
def test_coincident_points(gpu):
    """b = 0 links exactly the coincident pairs: 500 groups of 2."""
    base = uniform(500, 405)
    pts = np.concatenate([base, base])[np.random.default_rng(406).permutation(1000)]
    for box in (None, 1.0):
        t = gpu.Tree(pts, leafsize=16, boxsize=box)
        lab, siz, ng = check(gpu, t, pts, 0.0, box)
        assert ng == 500 and np.all(siz[siz > 0] == 2)


# ---------------------------------------------------------------- 7. leafsize 128
@pytest.mark.parametrize("box", [None, 1.0])
def test_two_staged_chunks_per_leaf(gpu, box):
    """leafsize 128: leaves of 65..128 points are staged as two chunks."""
    pts = uniform(5000, 306)
    t = gpu.Tree(pts, leafsize=128, boxsize=box)
    check(gpu, t, pts, 0.87 * 5000 ** (-1.0 / 3.0), box)


# ---------------------------------------------------------------- 8. replaced ids
def test_replaced_ids(gpu):
    """After nbkd_set_ids the labels are still input rows."""
    n = 3000
    pts = uniform(n, 407)
    b = 0.87 * n ** (-1.0 / 3.0)
    t = gpu.Tree(pts, leafsize=32, boxsize=1.0)
    before = t.fof(b)
    ids = (np.random.default_rng(408).permutation(n) + 1_000_000).astype(np.uint32)
    t.set_ids(ids)
    after = t.fof(b)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert after[2] == before[2]
    assert np.array_equal(after[0], brute_labels(pts, b, 1.0))


# ---------------------------------------------------------------- 9. device outputs, repeatability
@pytest.mark.parametrize("box", [None, 1.0])
def test_device_outputs_and_repeatability(gpu, box):
    """Device buffers are raw HIP allocations (nbodyhpc_amd.hip): a process
    that drives libnbkd cannot also initialise torch.cuda, whose wheel bundles
    another HIP runtime (see nbodyhpc_amd/hip.py)."""
    from nbodyhpc_amd import hip
    f = 0.87
    pts = uniform(N1, 401)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    lab, siz, ng = t.fof(f * S1)
    assert np.array_equal(lab, ref1(f, box))
    lab2, siz2, ng2 = t.fof(f * S1)
    assert np.array_equal(lab2, lab) and np.array_equal(siz2, siz) and ng2 == ng
    fill = np.full(N1, 0xFFFFFFFF, np.uint32)
    dl, dz = hip.DeviceArray.from_numpy(fill), hip.DeviceArray.from_numpy(fill)
    t.fof_device(f * S1, dl.ptr, dz.ptr)
    hip.synchronize()
    assert np.array_equal(dl.numpy(), lab) and np.array_equal(dz.numpy(), siz)
    # labels alone, on a non-default stream
    s = hip.Stream()
    hip.memcpy(dl.ptr, fill.ctypes.data, fill.nbytes, hip.H2D)
    t.fof_device(f * S1, dl.ptr, None, stream=s.handle)
    s.synchronize()
    assert np.array_equal(dl.numpy(), lab)
    # both, on that stream, twice: identical arrays
    for _ in range(2):
        hip.memcpy(dl.ptr, fill.ctypes.data, fill.nbytes, hip.H2D)
        hip.memcpy(dz.ptr, fill.ctypes.data, fill.nbytes, hip.H2D)
        t.fof_device(f * S1, dl.ptr, dz.ptr, stream=s.handle)
        s.synchronize()
        assert np.array_equal(dl.numpy(), lab) and np.array_equal(dz.numpy(), siz)


# ---------------------------------------------------------------- 10. argument errors
def test_argument_errors(gpu):
    t = gpu.Tree(uniform(100, 409), leafsize=16)
    for b in (-1.0, float("nan"), float("inf")):
        with pytest.raises(gpu.NbkdError) as e:
            t.fof(b)
        assert e.value.status == gpu.NBKD_EINVAL
    import ctypes
    ng = ctypes.c_uint64()
    st = gpu.lib().nbkd_fof(t.h, 0.1, None, None, ctypes.byref(ng), 0, None)
    assert st == gpu.NBKD_EINVAL and b"NULL" in gpu.lib().nbkd_last_error()


# ---------------------------------------------------------------- 11. Python surface
def test_python_surface(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    pts = uniform(N1, 401)
    b = 0.5 * S1
    ref = ref1(0.5, 1.0).astype(np.int64)
    t = KDTree(pts, leafsize=32, boxsize=1.0)
    labels, sizes = t.fof_labels(b)
    assert labels.dtype == np.uint32 and labels.shape == (N1,)
    assert sizes.dtype == np.uint32 and sizes.shape == (N1,)
    assert np.array_equal(labels, ref)
    assert np.array_equal(sizes, np.bincount(ref, minlength=N1))
    # numbering by descending size, ties by the smaller label
    heads = np.unique(ref)
    cnt = np.bincount(ref, minlength=N1)[heads]
    order = np.lexsort((heads, -cnt))
    number = np.full(N1, -1, np.int64)
    number[heads[order]] = np.arange(len(heads))
    group, gs = t.fof(b, return_sizes=True)
    assert group.dtype == np.int64 and group.shape == (N1,)
    assert gs.dtype == np.int64 and gs.shape == (4552,)
    assert np.array_equal(group, number[ref])
    assert np.array_equal(gs, cnt[order])
    assert np.all(np.diff(gs) <= 0) and gs.sum() == N1
    assert np.array_equal(t.fof(b), group)
    # min_members = 3: smaller groups map to -1, the numbering of the rest stays
    g3, s3 = t.fof(b, min_members=3, return_sizes=True)
    keep = cnt[order] >= 3
    assert s3.min() >= 3 and np.array_equal(s3, cnt[order][keep])
    small = cnt[order][group] < 3
    assert np.all(g3[small] == -1) and np.array_equal(g3[~small], group[~small])
    assert s3.sum() == np.count_nonzero(g3 >= 0)
