"""Every query kernel on coordinates away from the unit box (tests/units.py):
scales 2^-45 .. 2^55, kpc/h and Mpc/h periodic boxes, sets centred on 0 (half
the coordinates negative, -0.0 and +0.0 mixed) and sets at a large offset.

The exact-output kernels (build, kNN, radius count / histogram / CSR, FoF) run
in every frame against the C oracle and the brute forces the suite already
has; tests/test_units_inputs.py shows on the CPU that those references are
sound there.  The float-sum kernels (ball_sum, ball_profile, gravity) run in
the frames whose h^2 and 1/d^3 stay inside float32, with their own relative
bounds unchanged.  On the power-of-two frames the GPU's outputs must also be
the base frame's scaled: 2^e commutes with every IEEE add, multiply, divide
and square root, and the tree (hence every summation order) is the same.  The
kNN work counters must not depend on the unit either where the density seed is
defined; where it is not ("Coordinate range") the results stay
exact and the counters are printed and reported."""
import functools
import json
import os

import numpy as np
import pytest

from tests import units
from tests.parity import assert_knn_equal, check_tree_structure, d2_ref, leaf_sets
from tests.test_gpu_ball_profile import check_all as profile_check_all
from tests.test_gpu_ball_sum import CUBIC, TOPHAT, WENDLAND
from tests.test_gpu_ball_sum import check_all as sum_check_all
from tests.test_gpu_fof import brute_labels
from tests.test_gpu_fof import check as fof_check
from tests.test_gpu_gravity import check_tree, masses

pytestmark = pytest.mark.gpu

N, M = 20_003, 3000        # exact kernels: n % 8 != 0, a third of the queries are self rows
NSELF = 60_000             # self-order path: several anchors, both anchor halves
NF, MF = 6000, 1500        # FoF and the float sums (their brute forces are O(n m))
NG, MG = 6003, 600         # gravity (its oracle walks the tree in Python)
SF = NF ** (-1.0 / 3.0)
KS = (1, 8, 32, 33, 64, 100, 200)
HIST_FRACTIONS = (0.01, 0.03, 0.074, 0.12, 0.2, 0.3)

case_param = pytest.mark.parametrize("case", units.CASES, ids=units.case_id)


def cases_of(names):
    return [c for c in units.CASES if c[0] in names]


def base_case(case):
    """the (frame, box) a dyadic case is an exact multiple of, and the factor"""
    name, box = case
    f = units.FRAMES[name]
    return (f.base, None if box is None else box / f.a), np.float32(2.0 ** f.exp)


@functools.lru_cache(maxsize=None)
def orc():
    from oracle.oracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=8)
def oracle_tree(name, box, n, m, leaf):
    return orc().tree(units.inputs(name, n, m)[0], leaf, box)


@pytest.fixture
def tuning(gpu):
    """nbkd_set_tuning knobs, restored after the test."""
    saved = {n: gpu.get_tuning(n) for n in ("knn_seed_margin", "self_order")}
    yield gpu.set_tuning
    for n, v in saved.items():
        gpu.set_tuning(n, v)


# ---------------------------------------------------------------- build
def splits_where_sets_agree(gn, gi, on, oi):
    """Every internal node that holds the same points in both trees must have
    the same split value, the order statistic of that set (== on floats: a
    split at -0.0 equals one at +0.0).  Returns (such nodes, internal nodes);
    the root is always one."""
    same = internal = 0
    stack = [(0, 0, len(gi))]
    while stack:
        nid, lo, hi = stack.pop()
        if gn["dim"][nid] < 0:
            continue
        internal += 1
        if np.array_equal(np.sort(gi[lo:hi]), np.sort(oi[lo:hi])):
            same += 1
            assert gn["split"][nid] == on["split"][nid], f"node {nid}: the same points, another split"
        m = ((hi - lo) // 2) // 8 * 8
        stack.append((int(gn["right"][nid]), lo + m, hi))
        stack.append((nid + 1, lo, lo + m))
    return same, internal


@pytest.mark.parametrize("leaf", [16, 64])
@case_param
def test_build_node_table(gpu, case, leaf):
    """The node table (dim, left, right, split) against the oracle's: the radix
    select's float keys must order negative coordinates as the reference's
    comparison does, and the key-space bounding box must hold.

    Where no two points share a coordinate the whole table is pinned and is
    compared bit for bit, with the leaves' members.  In the frames whose
    float32 coordinates collide (off1000: steps of 2^-14; off-3e5: steps of
    1/32; zeros: 100 rows tied at the root's split, of both signs) which of the
    points tied at a split go left is the partition's choice (DESIGN.md
    section 4), and the descendants' splits follow from it.  There the shape is
    compared exactly, every node that holds the oracle's points must have the
    oracle's split, and check_tree_structure holds the rest to the median-split
    rule."""
    name, box = case
    pts, _ = units.inputs(name, N, M)
    assert N % 8 != 0
    tie_free = all(len(np.unique(pts[:, a])) == N for a in range(3))
    assert tie_free == (name not in units.TIED)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    o = orc().tree(pts, leaf, box)
    gn, gx, gy, gz, gi = t.export()
    on, _, _, _, oi = o.export()
    assert t.n == o.n and t.size == o.size
    for key in ("dim", "left", "right"):
        assert np.array_equal(gn[key], on[key]), key
    check_tree_structure(gn, gx, gy, gz, gi, N, leaf)
    same, internal = splits_where_sets_agree(gn, gi, on, oi)
    if tie_free:
        assert np.array_equal(gn.view(np.uint32), on.view(np.uint32))
        assert leaf_sets(gn, gi) == leaf_sets(on, oi)
        assert same == internal
    else:
        print(f"{units.case_id(case)} leafsize {leaf}: {same} of {internal} internal nodes hold "
              "the oracle's points")
        if name == "zeros":
            assert gn["dim"][0] == 0 and gn["split"][0] == 0  # the root splits among the zeros
    real = gi < N
    assert np.array_equal(np.stack([gx, gy, gz], 1)[real].view(np.uint32),
                          pts[gi[real]].view(np.uint32))  # signs of zero travel too
    t.close()


# ---------------------------------------------------------------- kNN
@case_param
def test_knn_vs_oracle_tree(gpu, tuning, case):
    """k = 1 and 8 (lane select), 32 (its power-of-two copy), 33 and 64 (the
    (32, 64] path), 100 (paired wave select), 200 (k > 128): rows, the k-th
    distance and the squared output against the oracle tree; k = 32 again with
    a seed margin that sends most queries through the retry rounds and the
    exact kernel."""
    name, box = case
    pts, q = units.inputs(name, N, M)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    o = oracle_tree(name, box, N, M, 32)
    for k in KS:
        dr, ir = o.query(q, k, workers=4)
        d, i = t.query(q, k)
        assert_knn_equal(d, i, dr, ir, pts, q, box)
        assert np.array_equal(t.query_kth(q, k).view(np.uint32), dr[:, k - 1].view(np.uint32)), k
        if k in (8, 32, 100, 200):
            d2r, _ = o.query(q, k, workers=4, sqrt=False)
            d2, i2 = t.query(q, k, squared=True)
            assert np.all(np.isfinite(d2))
            assert_knn_equal(d2, i2, d2r, ir, pts, q, box, sqrt=False)
            assert np.array_equal(np.sqrt(d2), d)
    tuning("knn_seed_margin", 0.05)
    dr, ir = o.query(q, 32, workers=4)
    d, i = t.query(q, 32)
    assert_knn_equal(d, i, dr, ir, pts, q, box)
    t.close()


# ---------------------------------------------------------------- kNN work counters
COUNTERS = ("node_visits", "pair_evals", "leaves_reached", "sparse_iters", "points_staged",
            "packets", "candidates", "leaves_scanned", "fallback_queries", "retry_queries",
            "chunk_lanes")
SELF_FRAMES = ("unit", "s-45", "s-20", "s+17", "s+55", "L205000", "centred17")
HOMOGENEOUS = ("s-20", "s+17")
REPORTED = ("s-45", "s+40", "s+55", "L205000", "L67.77")


@functools.lru_cache(maxsize=None)
def knn32_counted(case, path):
    """(d, i, counters) of the k = 32 query with the work counters on.
    "bucketed": host queries (N points, M queries, leafsize 32).  "self": the
    tree built from a device array and queried with its own rows (NSELF)."""
    from nbodyhpc_amd import capi, hip
    name, box = case
    capi.stats_enable(True)
    try:
        if path == "bucketed":
            pts, q = units.inputs(name, N, M)
            t = capi.Tree(pts, leafsize=32, boxsize=box)
            d, i = t.query(q, 32)
        else:
            pts, _ = units.inputs(name, NSELF, 3)
            dp = hip.DeviceArray.from_numpy(pts)
            t = capi.Tree(n=NSELF, dev_ptr=dp.ptr, leafsize=32, boxsize=box)
            od = hip.DeviceArray((NSELF, 32), np.float32)
            oi = hip.DeviceArray((NSELF, 32), np.uint32)
            s = hip.Stream()
            capi.timing_enable(True)
            capi.timing_reset()
            t.query_device(dp.ptr, NSELF, 32, od.ptr, oi.ptr, s.handle)
            s.synchronize()
            took = capi.timing_read("self_order")[1]
            capi.timing_enable(False)
            assert took > 0, "the self-order path did not run"
            d, i = od.numpy(), oi.numpy()
        st = capi.stats_read_all()
    finally:
        capi.stats_enable(False)
        capi.timing_enable(False)
    t.close()
    return d, i, {key: st[key] for key in COUNTERS}


def check_knn32_counted(case, path):
    name, box = case
    d, i, st = knn32_counted(case, path)
    if path == "bucketed":
        pts, q = units.inputs(name, N, M)
        dr, ir = oracle_tree(name, box, N, M, 32).query(q, 32, workers=4)
    else:
        pts, _ = units.inputs(name, NSELF, 3)
        q = pts
        dr, ir = orc().tree(pts, 32, box).query(q, 32, workers=8)
        assert np.all(d[:, 0] == 0)
    assert_knn_equal(d, i, dr, ir, pts, q, box)
    return st


@case_param
def test_knn_bucketed_with_counters_exact(gpu, case):
    """the STATS instance of the collect kernel gives the oracle's rows too"""
    st = check_knn32_counted(case, "bucketed")
    print(units.case_id(case), st)
    assert st["packets"] > 0


@pytest.mark.parametrize("case", cases_of(SELF_FRAMES), ids=units.case_id)
def test_self_order_vs_oracle_tree(gpu, case):
    """A tree built from a device array, queried with its own rows at k = 32:
    seeds come from each row's anchor (anchor_chunk_kernel), 60 000 points
    give several anchors and both anchor halves."""
    st = check_knn32_counted(case, "self")
    print(units.case_id(case), st)
    assert st["packets"] > 0


@pytest.mark.parametrize("path", ["bucketed", "self"])
@pytest.mark.parametrize("case", cases_of(HOMOGENEOUS), ids=units.case_id)
def test_work_counters_do_not_depend_on_the_unit(gpu, case, path):
    """The seeds are homogeneous in the scale, so the walk is the unit frame's
    walk: every counter equal.  A counter that differs means a constant with
    units in it.

    At 2^17 every counter is equal.  At 2^-20 only `packets` and
    `fallback_queries` are asserted: guess_r2 (query.hip) forms `r3 * r3`, the
    sixth power of the seed radius, and with a radius of 6e-8 to 8e-8 (0.06 to
    0.085 of 2^-20) that product is 2^-144 to 2^-141, a subnormal with 5 to 8
    significant bits left.  cbrtf of it gives a seed that differs from the
    unit frame's scaled in its low bits, so a few queries' seed balls hold
    other points: measured, 8 524 984 pair evaluations against 8 523 912 and
    3324 retried queries against 3307 (self order, 60 000 points), 417 512
    against 417 472 and 272 against 272 (bucketed).  The rows stay exact.  The
    other counters are printed ("Coordinate range")."""
    base, _ = base_case(case)
    st = knn32_counted(case, path)[2]
    ref = knn32_counted(base, path)[2]
    print(units.case_id(case), path, st, "unit frame", ref)
    # the seed works in the unit frame: most queries pass at the first attempt
    assert ref["fallback_queries"] == 0
    assert ref["retry_queries"] < 0.5 * (M if path == "bucketed" else NSELF)
    keys = COUNTERS if case[0] == "s+17" else ("packets", "fallback_queries")
    assert {key: st[key] for key in keys} == {key: ref[key] for key in keys}


def test_work_counters_report(gpu):
    """Outside the seed's range (and in the non-dyadic boxes) only exactness is
    asserted; the counters are printed next to the unit frame's and written to
    $NBKD_TEST_REPORT_DIR/units_stats.json."""
    report = {}
    for case in cases_of(("unit",) + HOMOGENEOUS + REPORTED):
        entry = {"bucketed": check_knn32_counted(case, "bucketed")}
        if case[0] in SELF_FRAMES:
            entry["self"] = check_knn32_counted(case, "self")
        report[units.case_id(case)] = entry
        print(units.case_id(case), entry)
    out = os.environ.get("NBKD_TEST_REPORT_DIR")
    if out:
        with open(os.path.join(out, "units_stats.json"), "w") as f:
            json.dump({"bucketed": {"n": N, "m": M}, "self": {"n": NSELF, "m": NSELF}, "k": 32,
                       "leafsize": 32, "counters": report}, f, indent=1)


# ---------------------------------------------------------------- radius queries
def radius_set(name, box, o, q):
    """about two mean spacings, several leaves wide (leafsize 16), a realised
    pair distance, and on periodic frames 0.499 L; then the 8 ascending
    radii of the histogram (those and four more)"""
    d2 = o.query(q, 8, workers=4, sqrt=False)[0]
    tie = units.tie_radius(d2[:, 7])
    assert tie is not None
    t2 = np.float32(tie) * np.float32(tie)
    assert (d2 == t2).any()  # d2 == r2 occurs
    radii = [units.length(name, 0.074), units.length(name, 0.2), tie]
    if box is not None:
        radii.append(units.length(name, 0.499))
    hist = [units.length(name, f) for f in HIST_FRACTIONS] + [tie]
    hist.append(units.length(name, 0.499 if box is not None else 0.4))
    hist = np.sort(np.array(hist, np.float32))
    assert len(hist) == 8 and np.all(np.diff(hist) > 0)
    return radii, hist


def csr_rows(off, idx, rows):
    return [np.sort(idx[off[j]:off[j + 1]]) for j in rows]


@case_param
def test_radius_queries(gpu, case):
    """ball_count, ball_csr (rows as sorted sets) and ball_hist against the
    oracle's brute-force count and tests.parity.d2_ref."""
    name, box = case
    pts, q = units.inputs(name, N, M)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    radii, hist = radius_set(name, box, oracle_tree(name, box, N, M, 32), q)
    for n_r, r in enumerate(radii):
        cb = orc().ball_count_brute(pts, q, r, box)
        c = t.ball_count(q, r)
        bad = np.flatnonzero(c != cb)
        assert bad.size == 0, f"r = {r!r}: {bad.size} counts differ, rows {bad[:5]}: {c[bad[:5]]} vs {cb[bad[:5]]}"
        # the widest periodic ball holds half the points: CSR rows of a subset
        sub = np.arange(M) if n_r < 3 else np.concatenate([np.arange(150), np.arange(M - 150, M)])
        off, idx = t.ball_csr(q[sub], r)
        assert np.array_equal(np.diff(off.astype(np.int64)), cb[sub].astype(np.int64))
        r2 = np.float32(r) * np.float32(r)
        rows = range(0, len(sub), 41)
        for j, row in zip(rows, csr_rows(off, idx, rows)):
            expect = np.flatnonzero(d2_ref(q[sub[j]], pts, box) <= r2)
            assert np.array_equal(row, expect.astype(np.uint32)), (r, j)
    if box is not None:
        assert cb.min() > 0.4 * N
    ref = np.stack([orc().ball_count_brute(pts, q, float(r), box) for r in hist], axis=1)
    c, tot = t.ball_hist(q, hist)
    for j in range(len(hist)):
        assert np.array_equal(c[:, j], ref[:, j]), f"column {j} (r = {hist[j]!r})"
    assert np.array_equal(tot, ref.sum(axis=0, dtype=np.uint64))
    t.close()


# ---------------------------------------------------------------- FoF
FOF_FRAMES = ("s-45", "s+17", "s+55", "L205000", "L67.77", "centred17", "off-3e5")
FOF_CASES = [(c, f) for c in cases_of(FOF_FRAMES) for f in (0.5, 0.87)]
# at -3e5 the coordinates are multiples of 1/32: b = 1/16 puts every pair two
# steps apart along an axis exactly on the threshold
FOF_CASES.append((("off-3e5", None), 1.0 / (16 * SF)))


def fof_length(name, f):
    return units.length(name, f * SF)


@pytest.mark.parametrize("case,f", FOF_CASES, ids=[f"{units.case_id(c)}-{f:.3g}" for c, f in FOF_CASES])
def test_fof(gpu, case, f):
    name, box = case
    pts, _ = units.inputs(name, NF, MF)
    b = fof_length(name, f)
    if name == "off-3e5":
        thr = np.float32(b) * np.float32(b)
        ties = int((d2_ref(pts[:500, None, :], pts[None, :, :]) == thr).sum())
        print(f"b = {b!r}: {ties} pairs of the first 500 rows on the threshold")
        assert (ties > 100) == (f > 0.9)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    lab, siz, ng = fof_check(gpu, t, pts, b, box)
    print(f"{units.case_id(case)} b = {f:.3g} s: {ng} groups, largest {siz.max()}")
    assert 1 < ng < NF
    t.close()


# ---------------------------------------------------------------- equivariance, exact kernels
def no_tie_rows(d):
    """rows of an (m, k + 1) result whose k + 1 distances are all different"""
    return np.all(np.diff(np.sort(d, axis=1), axis=1) != 0, axis=1)


@pytest.mark.parametrize("case", cases_of(units.DYADIC), ids=units.case_id)
def test_equivariance_exact_kernels(gpu, case):
    """The GPU's own outputs in a power-of-two frame are the base frame's
    scaled: distances and split values x 2^e under ==, indices equal where the
    row has no tie, node ranges, counts, histograms and CSR rows identical.
    No reference is involved, so an absolute constant that the oracle
    comparison happens to survive would still show here."""
    name, box = case
    (bname, bbox), s = base_case(case)
    pts, q = units.inputs(name, N, M)
    bpts, bq = units.inputs(bname, N, M)
    assert np.array_equal(pts, bpts * s) and np.array_equal(q, bq * s)
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    tb = gpu.Tree(bpts, leafsize=16, boxsize=bbox)
    gn, gx, _, _, gi = t.export()
    bn, bx, _, _, bi = tb.export()
    for key in ("dim", "left", "right"):
        assert np.array_equal(gn[key], bn[key]), key
    assert np.array_equal(gn["split"], bn["split"] * s)
    assert np.array_equal(gi, bi)
    assert np.array_equal(gx[gi < N], bx[bi < N] * s)
    for k in (1, 8, 32, 64, 100, 200):
        d, i = t.query(q, k + 1)
        db, ib = tb.query(bq, k + 1)
        assert np.array_equal(d, db * s), k
        clean = no_tie_rows(db)
        assert clean.sum() > M // 2
        assert np.array_equal(i[clean], ib[clean]), k
        d, i = t.query(q, k)
        db, ib = tb.query(bq, k)
        assert np.array_equal(d, db * s), k
        assert np.array_equal(i[clean], ib[clean]), k
        assert np.array_equal(t.query_kth(q, k), tb.query_kth(bq, k) * s)
        d2 = t.query(q, k, squared=True)[0]
        assert np.array_equal(d2, tb.query(bq, k, squared=True)[0] * s * s)
    radii, hist = radius_set(name, box, oracle_tree(name, box, N, M, 32), q)
    bradii, bhist = radius_set(bname, bbox, oracle_tree(bname, bbox, N, M, 32), bq)
    assert np.array_equal(np.array(radii, np.float32), np.array(bradii, np.float32) * s)
    assert np.array_equal(hist, bhist * s)
    for r, rb in zip(radii, bradii):
        assert np.array_equal(t.ball_count(q, r), tb.ball_count(bq, rb))
    for r, rb in zip(radii[:3], bradii[:3]):
        off, idx = t.ball_csr(q, r)
        boff, bidx = tb.ball_csr(bq, rb)
        assert np.array_equal(off, boff)
        rows = range(0, M, 7)
        assert all(np.array_equal(a, b) for a, b in zip(csr_rows(off, idx, rows),
                                                        csr_rows(boff, bidx, rows)))
    c, tot = t.ball_hist(q, hist)
    cb, totb = tb.ball_hist(bq, bhist)
    assert np.array_equal(c, cb) and np.array_equal(tot, totb)
    t.close()
    tb.close()


@pytest.mark.parametrize("case", cases_of(units.DYADIC), ids=units.case_id)
def test_equivariance_fof(gpu, case):
    """FoF labels, sizes and group counts of a power-of-two frame equal the
    base frame's."""
    name, box = case
    (bname, bbox), s = base_case(case)
    pts, _ = units.inputs(name, NF, MF)
    bpts, _ = units.inputs(bname, NF, MF)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    tb = gpu.Tree(bpts, leafsize=32, boxsize=bbox)
    for f in (0.5, 0.87):
        lab, siz, ng = t.fof(fof_length(name, f))
        blab, bsiz, bng = tb.fof(fof_length(bname, f))
        assert np.array_equal(lab, blab) and np.array_equal(siz, bsiz) and ng == bng
        assert 1 < ng < NF
    if name == "s+17" and box is None:  # the base frame's labels are right too
        assert np.array_equal(blab, brute_labels(bpts, fof_length(bname, 0.87), bbox))
    t.close()
    tb.close()


# ---------------------------------------------------------------- float sums
SUM_FRAMES = ("unit", "s-20", "s+17", "L205000", "centred17")
SUM_DYADIC = ("s-20", "s+17", "centred17")
GRAVITY_FRAMES = ("unit", "s-20", "s+17", "centred17")


def unit_draws(seed, lo, hi, m):
    """float32 factors in [lo, hi) to be multiplied by a frame's scale"""
    return np.random.default_rng(seed).uniform(lo, hi, m).astype(np.float32)


def scaled(name, v):
    """float32 values times the frame's scale (exact on the dyadic frames)"""
    return (np.asarray(v, np.float64) * units.FRAMES[name].a).astype(np.float32)


def sum_inputs(name):
    pts, q = units.inputs(name, NF, MF)
    h = scaled(name, unit_draws(701, 0.0, 3 * SF, MF))
    rng = np.random.default_rng(702)
    ints = rng.integers(1, 9, size=(NF, 3)).astype(np.float32)
    vals = (0.5 + 1.5 * rng.random((NF, 2))).astype(np.float32)
    return pts, q, h, ints, vals


@functools.lru_cache(maxsize=None)
def ball_sum_outputs(case):
    from nbodyhpc_amd import capi
    name, box = case
    pts, q, h, ints, vals = sum_inputs(name)
    t = capi.Tree(pts, leafsize=32, boxsize=box)
    out = [t.ball_sum(q, h, ints, kernel=TOPHAT, count=True)]
    out += [t.ball_sum(q, h, vals, kernel=kern, count=True) for kern in (CUBIC, WENDLAND)]
    t.close()
    return out


@pytest.mark.parametrize("case", cases_of(SUM_FRAMES), ids=units.case_id)
def test_ball_sum(gpu, case):
    """check_all of test_gpu_ball_sum (counts exact, integer sums exact, cubic
    and Wendland sums within its relative bound, unchanged) with h in units of
    the frame's scale; on the dyadic frames sums and counts are the base
    frame's bits (u = sqrt(d2) / h does not see the unit)."""
    name, box = case
    pts, q, h, _, _ = sum_inputs(name)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    cnt = sum_check_all(t, pts, q, h, box, 703)
    assert cnt.max() > 50 and cnt.min() == 0
    t.close()
    if name in SUM_DYADIC:
        base, _ = base_case(case)
        for (s, c), (sb, cb) in zip(ball_sum_outputs(case), ball_sum_outputs(base)):
            assert np.array_equal(c, cb)
            assert np.array_equal(s.view(np.uint32), sb.view(np.uint32))


PROFILE_SHARED = np.geomspace(0.004, 0.3, 12).astype(np.float32)
PROFILE_SCALED = np.geomspace(0.004, 0.08, 10).astype(np.float32)


def profile_inputs(name):
    pts, q = units.inputs(name, NF, MF)
    scale = scaled(name, unit_draws(711, 0.3, 3.0, MF))
    return pts, q, scaled(name, PROFILE_SHARED), scale


@functools.lru_cache(maxsize=None)
def profile_outputs(case):
    from nbodyhpc_amd import capi
    name, box = case
    pts, q, shared, scale = profile_inputs(name)
    vals = (0.5 + 1.5 * np.random.default_rng(712).random((NF, 2))).astype(np.float32)
    t = capi.Tree(pts, leafsize=32, boxsize=box)
    out = [t.ball_profile(q, shared, None, None), t.ball_profile(q, shared, vals, None),
           t.ball_profile(q, PROFILE_SCALED, None, scale),
           t.ball_profile(q, PROFILE_SCALED, vals, scale)]
    t.close()
    return out


@pytest.mark.parametrize("case", cases_of(SUM_FRAMES), ids=units.case_id)
def test_ball_profile(gpu, case):
    """check_all of test_gpu_ball_profile with shared radii in units of the
    frame's scale and with per-query scales in those units; on the dyadic
    frames the sums are the base frame's bits."""
    name, box = case
    pts, q, shared, scale = profile_inputs(name)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    cnt = profile_check_all(t, pts, q, box, shared, None, 713)
    assert cnt.sum(axis=1).min() > 20
    cnt = profile_check_all(t, pts, q, box, PROFILE_SCALED, scale, 714)
    assert cnt.sum() > 10 * MF
    t.close()
    if name in SUM_DYADIC:
        base, _ = base_case(case)
        for a, b in zip(profile_outputs(case), profile_outputs(base)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def gravity_inputs(name):
    pts, q = units.inputs(name, NG, MG)
    return pts, q, masses(NG, 721), (0.0, units.length(name, 0.02))


@functools.lru_cache(maxsize=None)
def gravity_outputs(name):
    from nbodyhpc_amd import capi
    pts, q, mass, eps = gravity_inputs(name)
    t = capi.Tree(pts, leafsize=16)
    out = [t.gravity(q, mass, theta=theta, eps=e) for theta in (0.0, 0.5) for e in eps]
    t.close()
    return out


@pytest.mark.parametrize("name", GRAVITY_FRAMES)
def test_gravity(gpu, name):
    """check_tree of test_gpu_gravity (the walk nbkd.h defines, its rounding
    bound unchanged) at theta 0 and 0.5, eps 0 and 0.02 of the scale; on the
    dyadic frames potentials are the base frame's x 2^-e and accelerations
    x 2^-2e."""
    pts, q, mass, eps = gravity_inputs(name)
    check_tree(gpu, pts, mass, q, leafsize=16, thetas=(0.0, 0.5), eps=eps, what=name).close()
    f = units.FRAMES[name]
    if f.base:
        s = 2.0 ** f.exp
        for (phi, acc), (bphi, bacc) in zip(gravity_outputs(name), gravity_outputs(f.base)):
            assert np.all(np.isfinite(phi)) and np.all(phi < 0)
            assert np.array_equal(phi, (bphi.astype(np.float64) / s).astype(np.float32))
            assert np.array_equal(acc, (bacc.astype(np.float64) / (s * s)).astype(np.float32))
