"""The packet walk (packet.hpp) under the radius kernels that share it: the CSR
fill (ball.hip), the radius histogram (ball_hist.hip), the kernel-weighted sums
(ball_sum.hip) and the friends-of-friends hook (fof.hip) on walk_begin /
walk_next_leaf, the radial profiles (ball_profile.hip) on the macro form of the
same traversal, on the walk shapes their own tests do not reach: split planes
tied with the queries, a deep stack, plain and periodic packets in one launch,
and an open tree with queries far outside the data.  The test_prologue_* cases
run what the five radius kernels do before the walk (packet_query, packet_plain)
with a wave and lanes without a query, periodic queries outside the box, a plain
and a non-plain packet and a padded leaf; the two gravity walks, which have no
vote, meet those conditions in their own tests
(test_small_query_counts with m = 1, 63, 65 on 700 points, test_seventeen_points,
and test_gpu_gravity_ewald.py's test_outside_queries).

Every output is compared with a brute force in plain numpy on the host: the
f32 distances of tests.parity.d2_ref between the queries and the points, in
blocks.  The blocks are slabs in x at least 1.02 r wide, and a slab of queries
is only compared with the points of the same and the two adjacent slabs: d2 is
a sum of non-negative f32 terms, so a pair whose x coordinates lie more than
1.02 r apart (minimum image on a periodic tree) has d2 > fl(r * r) and is in
no ball.  Counts, integer-weighted sums and labels are exact, so these checks
need no tolerance.

The last test pins the order of the walk: the f32 sums of ball_sum (cubic
kernel, per-query radii) and ball_profile with one real-valued channel are
added per lane in the order the walk reaches the leaves, so their bits must
equal those recorded in tests/golden/packet_walk_order.npz.  That file was
written by this module's recorder,
    NBKD_LIB=<libnbkd.so of commit 5d70d44> python -m tests.test_gpu_packet_walk out.npz
with the library of the last commit in which all five kernels ran the macro
walk; the recorder ran every call twice and found equal bits.  Per
case it holds the SHA-256 of each output array (all rows are pinned) and every
16th row (for the failure message)."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import d2_ref
from tests.test_gpu_collect_walk import filament_points, grid_points

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "packet_walk_order.npz")
NR = 8
ROW_STRIDE = 16


# ---------------------------------------------------------------- shapes
@functools.lru_cache(maxsize=None)
def shape(name):
    """name -> (points, queries, leafsize, boxsize, r, b): r the radius of the
    query checks (mean count roughly 30 to 200), b the linking length."""
    if name.startswith("grid"):
        # 4097 points on the 1/16 lattice, self queries: q - split == 0 takes
        # the "not right" side.  r * 16 = 2.4 lies between the lattice
        # distances sqrt(5) and sqrt(6); b = 1/16 ties with the nearest
        # neighbours' distance
        g = grid_points()
        return g, g, 64, (1.0 if name == "grid_periodic" else None), 0.15, 1.0 / 16.0
    if name.startswith("filament"):
        # both children are wanted many levels in a row along the filament
        f = filament_points()
        return f, f[::25], 16, (1.0 if name == "filament_periodic" else None), 0.006, 0.002
    if name == "plain_and_periodic":
        # the lattice in the middle half of a box of L = 4 (its packets walk
        # with the plain formulas) and queries over the whole box, faces included
        g = grid_points() * np.float32(2.0) + np.float32(1.0)
        q = np.concatenate([g, uniform(1000, 103, L=4.0)])
        assert q.min() >= 0.0 and q.max() <= 4.0
        return g, q, 64, 4.0, 0.3, 2.0 / 16.0
    if name == "open_far":
        # 1000 queries 100 to 150 units outside the data, 1000 inside, shuffled:
        # 64 consecutive queries share little of their walks
        pts = uniform(20_000, 106)
        rng = np.random.Generator(np.random.PCG64(107))
        far = (rng.uniform(-1, 1, size=(1000, 3)) * 25.0
               + np.where(rng.uniform(size=(1000, 3)) < 0.5, -125.0, 125.0)).astype(np.float32)
        q = np.concatenate([far, uniform(1000, 108)])
        return pts, q[rng.permutation(len(q))], 64, None, 0.11, 0.03
    raise KeyError(name)


SHAPES = ["grid_periodic", "grid_open", "filament_periodic", "filament_open",
          "plain_and_periodic", "open_far"]
PINNED = SHAPES[:4]


def radii_of(r):
    return np.geomspace(r / 4.0, r, NR).astype(np.float32)


# ---------------------------------------------------------------- the brute force
def near_pairs(q, pts, r, box):
    """(qi, pj, d2) of every pair with d2_ref(q[qi], pts[pj]) <= fl(r * r),
    ordered by (qi, pj)."""
    q, pts = np.asarray(q, np.float32), np.asarray(pts, np.float32)
    thr = np.float32(r) * np.float32(r)
    lo = 0.0 if box is not None else float(pts[:, 0].min())
    ext = float(box) if box is not None else float(pts[:, 0].max()) - lo
    ns = max(1, min(512, int(ext / (1.02 * float(r)))))
    w = max(ext / ns, 1.02 * float(r))
    sq = np.floor((q[:, 0].astype(np.float64) - lo) / w).astype(np.int64)
    sp = np.floor((pts[:, 0].astype(np.float64) - lo) / w).astype(np.int64)
    if box is not None:
        sq, sp = np.clip(sq, 0, ns - 1), np.clip(sp, 0, ns - 1)
    out = []
    for s in np.unique(sq):
        ds = np.abs(sp - s)
        if box is not None:
            ds = np.minimum(ds, ns - ds)
        qs, ps = np.flatnonzero(sq == s), np.flatnonzero(ds <= 1)
        if ps.size == 0:
            continue
        step = max(1, 4_000_000 // ps.size)
        for a in range(0, qs.size, step):
            d2 = d2_ref(q[qs[a:a + step], None, :], pts[None, ps, :], box)
            i, j = np.nonzero(d2 <= thr)
            out.append((qs[a:a + step][i], ps[j], d2[i, j]))
    qi = np.concatenate([o[0] for o in out])
    pj = np.concatenate([o[1] for o in out])
    d2 = np.concatenate([o[2] for o in out])
    order = np.lexsort((pj, qi))
    return qi[order], pj[order], d2[order]


@functools.lru_cache(maxsize=None)
def query_pairs(name):
    pts, q, _, box, r, _ = shape(name)
    qi, pj, d2 = near_pairs(q, pts, r, box)
    mean = len(qi) / len(q)
    print(f"{name}: {len(qi)} pairs within r = {r}, mean count {mean:.1f}")
    assert 30.0 <= mean <= 200.0
    return qi, pj, d2


@functools.lru_cache(maxsize=None)
def int_weights(name):
    n = len(shape(name)[0])
    return np.random.default_rng(900).integers(1, 9, size=n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def brute_labels(name):
    """labels[i] = the smallest row of i's group: a union-find (min-label
    propagation with pointer jumping, to a fixed point) over the pairs at b"""
    pts, _, _, box, _, b = shape(name)
    n = len(pts)
    qi, pj, _ = near_pairs(pts, pts, b, box)
    starts = np.flatnonzero(np.r_[True, qi[1:] != qi[:-1]])
    assert len(starts) == n  # every point is its own friend
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum.reduceat(lab[pj], starts)
        m = m[m]
        if np.array_equal(m, lab):
            return lab.astype(np.uint32)
        lab = m


def tree_of(gpu, name):
    pts, _, leaf, box, _, _ = shape(name)
    return gpu.Tree(pts, leafsize=leaf, boxsize=box)


# ---------------------------------------------------------------- checks
@pytest.mark.parametrize("name", SHAPES)
def test_csr_rows(gpu, name):
    _, q, _, _, r, _ = shape(name)
    qi, pj, _ = query_pairs(name)
    t = tree_of(gpu, name)
    off, idx = t.ball_csr(q, r, sorted=True)
    t.close()
    want = np.concatenate([[0], np.cumsum(np.bincount(qi, minlength=len(q)))]).astype(np.uint64)
    assert np.array_equal(off, want)
    assert np.array_equal(idx, pj.astype(np.uint32))


@pytest.mark.parametrize("name", SHAPES)
def test_histogram(gpu, name):
    _, q, _, _, r, _ = shape(name)
    qi, _, d2 = query_pairs(name)
    radii = radii_of(r)
    assert radii[-1] == np.float32(r)
    t = tree_of(gpu, name)
    got, _ = t.ball_hist(q, radii, total=False)
    t.close()
    want = np.stack([np.bincount(qi[d2 <= rk * rk], minlength=len(q)) for rk in radii], axis=1)
    assert np.array_equal(got, want.astype(np.uint32))


@pytest.mark.parametrize("name", SHAPES)
def test_tophat_sum_integer_weights(gpu, name):
    """Weights 1..8: every sum is an integer below 2^24, exact in any order."""
    _, q, _, _, r, _ = shape(name)
    qi, pj, _ = query_pairs(name)
    w = int_weights(name)
    t = tree_of(gpu, name)
    got, cnt = t.ball_sum(q, np.full(len(q), r, np.float32), w, kernel=gpu.KERNEL_TOPHAT,
                          count=True)
    t.close()
    want = np.bincount(qi, weights=w[pj].astype(np.float64), minlength=len(q))
    assert want.max() < 2 ** 24
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(cnt, np.bincount(qi, minlength=len(q)).astype(np.uint32))


@pytest.mark.parametrize("name", SHAPES)
def test_profile_integer_weights(gpu, name):
    _, q, _, _, r, _ = shape(name)
    qi, pj, d2 = query_pairs(name)
    w = int_weights(name)
    radii = radii_of(r)
    t = tree_of(gpu, name)
    got = t.ball_profile(q, radii, w)
    t.close()
    # bin = the number of thresholds with !(d2 <= t_k); every pair here is
    # within the last one
    b = np.zeros(len(qi), np.int64)
    for rk in radii:
        b += ~(d2 <= rk * rk)
    assert b.max() < NR
    want = np.bincount(qi * NR + b, weights=w[pj].astype(np.float64),
                       minlength=len(q) * NR).reshape(len(q), NR)
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("name", SHAPES)
def test_fof_partition(gpu, name):
    want = brute_labels(name)
    t = tree_of(gpu, name)
    lab, siz, ng = t.fof(shape(name)[5])
    t.close()
    assert 1 < ng < len(want)  # neither one group nor none
    assert np.array_equal(lab, want)
    assert np.array_equal(siz, np.bincount(want, minlength=len(want)).astype(np.uint32))


# ---------------------------------------------------------------- the packet prologue
# What the kernels do before the walk (packet.hpp packet_query, packet_plain):
# lanes and a whole wave without a query, periodic queries outside the box,
# which go to the brute kernels, one packet that votes for the plain formulas
# and packets that do not, on a tree with a padded leaf.
PRO_N, PRO_M, PRO_R = 3001, 131, 0.05


@functools.lru_cache(maxsize=None)
def prologue_case(box):
    """(points, [first call's queries, second call's], [their d2 matrices]):
    131 queries, 5 outside [0, 1]^3, 63 within 0.02 of a face, 63 interior, in
    mixed order; then 64 inside [0.4, 0.6]^3, a single packet that votes plain
    on the periodic tree."""
    pts = uniform(PRO_N, 950)
    rng = np.random.default_rng(951)
    face = uniform(63, 952)
    ax, side = rng.integers(0, 3, 63), rng.integers(0, 2, 63)
    off = rng.uniform(0.0, 0.02, 63).astype(np.float32)
    face[np.arange(63), ax] = np.where(side == 0, off, np.float32(1.0) - off)
    inner = (0.2 + 0.6 * uniform(63, 953)).astype(np.float32)
    out = uniform(5, 954)
    out[[0, 1, 2], [0, 1, 2]] += np.float32(1.5)
    out[[3, 4], [2, 0]] = np.float32(-0.3), np.float32(-0.01)
    q1 = np.concatenate([face, inner, out])[rng.permutation(PRO_M)]
    q2 = (0.4 + 0.2 * uniform(64, 955)).astype(np.float32)
    assert len(q1) == PRO_M and PRO_N % 8 != 0
    assert ((q1 < 0.0) | (q1 > 1.0)).any(axis=1).sum() == 5
    assert q2.min() >= 0.4 and q2.max() <= 0.6
    qs = [q1, q2]
    d2 = [d2_ref(q[:, None, :], pts[None, :, :], box) for q in qs]
    for a in [pts] + qs + d2:
        a.setflags(write=False)
    return pts, qs, d2


@pytest.mark.parametrize("box", [None, 1.0], ids=["open", "periodic"])
def test_prologue_csr_rows(gpu, box):
    pts, qs, d2s = prologue_case(box)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for q, d2 in zip(qs, d2s):
        inside = d2 <= np.float32(PRO_R) * np.float32(PRO_R)
        off, idx = t.ball_csr(q, PRO_R, sorted=True)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(inside.sum(axis=1))])
                              .astype(np.uint64))
        assert np.array_equal(idx, np.nonzero(inside)[1].astype(np.uint32))
    t.close()


@pytest.mark.parametrize("box", [None, 1.0], ids=["open", "periodic"])
def test_prologue_histogram(gpu, box):
    pts, qs, d2s = prologue_case(box)
    radii = radii_of(PRO_R)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for q, d2 in zip(qs, d2s):
        got, _ = t.ball_hist(q, radii, total=False)
        want = np.stack([(d2 <= rk * rk).sum(axis=1) for rk in radii], axis=1)
        assert want[:, -1].max() > 0
        assert np.array_equal(got, want.astype(np.uint32))
    t.close()


@pytest.mark.parametrize("box", [None, 1.0], ids=["open", "periodic"])
def test_prologue_pair_counts(gpu, box):
    from tests import aniso_ref as ar
    pts, qs, _ = prologue_case(box)
    e1 = np.array([0.01, 0.02, PRO_R], np.float32)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for q in qs:
        for mode, e2, los in ((ar.RPPI, np.array([0.01, PRO_R], np.float32), 2),
                              (ar.SMU, np.array([0.5, 1.0], np.float32), 0)):
            want = ar.hist2_ref(pts, q, e1, e2, mode, los, box)
            assert want.sum() > 0
            assert np.array_equal(t.ball_hist2(q, e1, e2, mode, los), want)
    t.close()


@pytest.mark.parametrize("box", [None, 1.0], ids=["open", "periodic"])
def test_prologue_tophat_sum(gpu, box):
    """Weights 1..8: every sum is an integer below 2^24, exact in any order."""
    pts, qs, d2s = prologue_case(box)
    w = np.random.default_rng(956).integers(1, 9, size=PRO_N).astype(np.float32)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for q, d2 in zip(qs, d2s):
        inside = d2 <= np.float32(PRO_R) * np.float32(PRO_R)
        got, cnt = t.ball_sum(q, np.full(len(q), PRO_R, np.float32), w,
                              kernel=gpu.KERNEL_TOPHAT, count=True)
        assert np.array_equal(got.astype(np.float64), inside.astype(np.float64) @ w)
        assert np.array_equal(cnt, inside.sum(axis=1).astype(np.uint32))
    t.close()


@pytest.mark.parametrize("box", [None, 1.0], ids=["open", "periodic"])
def test_prologue_profile(gpu, box):
    pts, qs, d2s = prologue_case(box)
    w = np.random.default_rng(956).integers(1, 9, size=PRO_N).astype(np.float32)
    radii = radii_of(PRO_R)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for q, d2 in zip(qs, d2s):
        # bin = the number of thresholds with !(d2 <= t_k); bin NR is outside
        b = np.zeros(d2.shape, np.int64)
        for rk in radii:
            b += ~(d2 <= rk * rk)
        want = np.stack([(b == k).astype(np.float64) @ w for k in range(NR)], axis=1)
        assert want.sum() > 0
        assert np.array_equal(t.ball_profile(q, radii, w).astype(np.float64), want)
    t.close()


# ---------------------------------------------------------------- the order pin
def order_outputs(gpu, name):
    """name -> {"sum": (m,) f32, "profile": (m, NR) f32}: real-valued weights,
    per-query radii from r / 2 to r for the sums"""
    pts, q, _, _, r, _ = shape(name)
    rng = np.random.default_rng(901)
    vals = (0.5 + 1.5 * rng.random(len(pts))).astype(np.float32)
    h = (r * (0.5 + 0.5 * rng.random(len(q)))).astype(np.float32)
    t = tree_of(gpu, name)
    out = {"sum": t.ball_sum(q, h, vals, kernel=gpu.KERNEL_CUBIC),
           "profile": t.ball_profile(q, radii_of(r), vals)}
    t.close()
    assert out["sum"].dtype == np.float32 and out["sum"].shape == (len(q),)
    assert out["profile"].dtype == np.float32 and out["profile"].shape == (len(q), NR)
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


@pytest.mark.parametrize("name", PINNED)
def test_same_order_of_leaves(gpu, name):
    want = np.load(GOLDEN, allow_pickle=False)
    for key, got in order_outputs(gpu, name).items():
        rows = want[f"{name}/{key}/rows"]
        bad = np.flatnonzero((got[::ROW_STRIDE].view(np.uint32) != rows.view(np.uint32))
                             .reshape(len(rows), -1).any(axis=1))
        assert bad.size == 0, (f"{name} {key}: {bad.size} of the {len(rows)} recorded rows differ,"
                               f" first row {bad[0] * ROW_STRIDE}: {got[bad[0] * ROW_STRIDE]!r} vs"
                               f" {rows[bad[0]]!r}")
        assert np.array_equal(digest(got), want[f"{name}/{key}/sha256"]), f"{name} {key}"


def record(path):
    from nbodyhpc_amd import capi
    out = {}
    for name in PINNED:
        first, second = order_outputs(capi, name), order_outputs(capi, name)
        for key, a in first.items():
            if not np.array_equal(a.view(np.uint32), second[key].view(np.uint32)):
                raise SystemExit(f"{name} {key}: two runs give different bits")
            out[f"{name}/{key}/rows"] = a[::ROW_STRIDE].copy()
            out[f"{name}/{key}/sha256"] = digest(a)
        print(f"{name}: two runs equal", flush=True)
    np.savez(path, **out)
    print(f"wrote {path} with the library {capi.LIB_PATH}", flush=True)


if __name__ == "__main__":
    record(sys.argv[1])
