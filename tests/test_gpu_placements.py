"""The four placements of every streaming entry point, pinned to one another.

Queries (and the side arrays that follow them: h, scale, values, masses) are
host or device memory, the per-query outputs are host or device memory.  The
baseline is the device-in / device-out call, which never streams; the other
three placements stream in batches of host_batch = 64 (m = 209: four batches,
the last ragged), and host/host also runs as one batch (host_batch 0).  Every
result must be the baseline's under ==: each batch's slice of a side array
follows its queries, totals accumulate over the batches, and on the periodic
tree every batch has queries outside [0, L]^3 for the brute-force kernels.

The baseline's counts are tied once to the numpy float32 brute force of
tests/test_gpu_ball_sum.py (members), an independent reference."""
import functools

import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import assert_knn_equal
from tests.test_gpu_ball_sum import members

pytestmark = pytest.mark.gpu

N, M, LEAF, HB = 3000, 209, 16, 64
BOXES = (None, 1.0)
# rows moved out of [0, 1]^3 on the periodic tree: every batch of 64 has some
OUTSIDE_UP = [5, 17, 40, 70, 71, 100, 140, 150, 190, 200, 208]
OUTSIDE_DOWN = [0, 33, 63, 64, 99, 127, 128, 160, 192, 207]
R = 0.09
RADII = np.array([0.0, 0.03, 0.06, 0.06, 0.15], np.float32)
PROF_RADII = np.array([0.02, 0.05, 0.09, 0.2], np.float32)
E1 = np.array([0.02, 0.05, 0.08, 0.12], np.float32)
E2_PI = np.array([0.01, 0.03, 0.06, 0.12], np.float32)
E2_MU = np.array([0.25, 0.5, 0.75, 1.0], np.float32)
OBSERVER = np.array([-2.0, 0.5, 0.25], np.float32)
# (host_batch, queries on the device, outputs on the device); the baseline first
BASE = (0, True, True)
OTHERS = [(HB, False, False), (HB, True, False), (HB, False, True), (0, False, False)]


@functools.lru_cache(maxsize=None)
def inputs():
    pts = uniform(N, 901)
    q_in = uniform(M, 902)
    q_out = q_in.copy()
    q_out[OUTSIDE_UP] += np.float32(1.25)
    q_out[OUTSIDE_DOWN, 1] -= np.float32(0.5)
    rng = np.random.default_rng(903)
    h = (0.03 + 0.09 * np.arange(M) / M).astype(np.float32)       # distinct in every row
    scale = (0.5 + 1.0 * np.arange(M)[::-1] / M).astype(np.float32)  # likewise
    assert len(np.unique(h)) == M and len(np.unique(scale)) == M
    ints = rng.integers(1, 9, size=(N, 3)).astype(np.float32)
    mass = (0.5 + rng.random(N)).astype(np.float32)
    for a in (pts, q_in, q_out, h, scale, ints, mass):
        a.setflags(write=False)
    return pts, q_in, q_out, h, scale, ints, mass


def queries(box):
    _, q_in, q_out, *_ = inputs()
    return q_out if box else q_in


@pytest.fixture(scope="module")
def trees(gpu):
    pts = inputs()[0]
    ts = {box: gpu.Tree(pts, leafsize=LEAF, boxsize=box) for box in BOXES}
    yield ts
    for t in ts.values():
        t.close()


def run(gpu, call, inp, outs, placement):
    """call(in_ptrs, out_ptrs, flags) under one placement.  inp: the arrays
    that NBKD_INPUT_DEVICE places (None stays NULL), outs: (shape, dtype) of the
    arrays that NBKD_OUTPUT_DEVICE places (None stays NULL).  Returns what
    `call` returns and the outputs as numpy arrays."""
    from nbodyhpc_amd import hip
    hb, in_dev, out_dev = placement
    flags = (gpu.NBKD_INPUT_DEVICE if in_dev else 0) | (gpu.NBKD_OUTPUT_DEVICE if out_dev else 0)
    keep = [None if a is None else np.ascontiguousarray(a) for a in inp]
    if in_dev:
        keep = [None if a is None else hip.DeviceArray.from_numpy(a) for a in keep]
    in_ptrs = [None if a is None else (a.ptr if in_dev else a.ctypes.data) for a in keep]
    res = []
    for spec in outs:
        if spec is None:
            res.append(None)
        elif out_dev:
            res.append(hip.DeviceArray(*spec))
            res[-1].zero()
        else:
            res.append(np.zeros(*spec))
    out_ptrs = [None if o is None else (o.ptr if out_dev else o.ctypes.data) for o in res]
    old = gpu.get_tuning("host_batch")
    try:
        gpu.set_tuning("host_batch", hb)
        ret = call(in_ptrs, out_ptrs, flags)
        hip.synchronize()
    finally:
        gpu.set_tuning("host_batch", old)
    return ret, [None if o is None else (o.numpy() if out_dev else o) for o in res]


def same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} elements differ"


def matrix(gpu, call, inp, outs, what, equal=None):
    """the baseline's (return value, outputs), after every other placement has
    been compared with it"""
    ret0, out0 = run(gpu, call, inp, outs, BASE)
    for p in OTHERS:
        ret, out = run(gpu, call, inp, outs, p)
        tag = f"{what}, host_batch {p[0]}, queries {'device' if p[1] else 'host'}, " \
              f"outputs {'device' if p[2] else 'host'}"
        if equal:
            equal(out, out0, tag)
        else:
            for a, b in zip(out, out0):
                same(a, b, tag)
        same(ret, ret0, tag + " (totals)")
    return ret0, out0


@pytest.mark.parametrize("box", BOXES)
def test_knn(gpu, trees, box):
    t, q, k = trees[box], queries(box), 8
    L = gpu.lib()

    def call(i, o, flags):
        gpu._check(L.nbkd_query_knn(t.h, i[0], M, k, o[0], o[1], flags, None))

    def equal(out, out0, tag):
        assert_knn_equal(out[0], out[1], out0[0], out0[1], inputs()[0], q, box)

    _, (d, _) = matrix(gpu, call, [q], [((M, k), np.float32), ((M, k), np.uint32)], "knn", equal)
    assert np.all(d[:, 0] <= d[:, -1])


@pytest.mark.parametrize("k", [8, 1100])  # 1100: past the collect path, rows through scratch
@pytest.mark.parametrize("box", BOXES)
def test_kth(gpu, trees, box, k):
    t, q = trees[box], queries(box)
    L = gpu.lib()

    def call(i, o, flags):
        gpu._check(L.nbkd_query_kth(t.h, i[0], M, k, o[0], flags, None))

    _, (kth,) = matrix(gpu, call, [q], [((M,), np.float32)], f"kth k {k}")
    assert np.all(kth > 0)


@pytest.mark.parametrize("box", BOXES)
def test_ball_count(gpu, trees, box):
    t, q = trees[box], queries(box)
    L = gpu.lib()

    def call(i, o, flags):
        gpu._check(L.nbkd_query_ball_count(t.h, i[0], M, R, o[0], flags, None))

    _, (c,) = matrix(gpu, call, [q], [((M,), np.uint32)], "ball_count")
    ref = members(inputs()[0], q, np.full(M, R, np.float32), box)[0].sum(axis=1)
    assert np.array_equal(c, ref.astype(np.uint32))


@pytest.mark.parametrize("rows,totals", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("box", BOXES)
def test_ball_hist(gpu, trees, box, rows, totals):
    t, q = trees[box], queries(box)
    L = gpu.lib()
    nr = len(RADII)

    def call(i, o, flags):
        tot = np.zeros(nr, np.uint64) if totals else None
        gpu._check(L.nbkd_query_ball_hist(t.h, i[0], M, RADII.ctypes.data, nr, o[0],
                                          tot.ctypes.data if totals else None, flags, None))
        return tot

    tot, (c,) = matrix(gpu, call, [q], [((M, nr), np.uint32) if rows else None],
                       f"ball_hist rows {rows} totals {totals}")
    pts = inputs()[0]
    ref = np.stack([members(pts, q, np.full(M, r, np.float32), box)[0].sum(axis=1)
                    for r in RADII], axis=1)
    if rows:
        assert np.array_equal(c, ref.astype(np.uint32))
    if totals:
        assert np.array_equal(tot, ref.sum(axis=0, dtype=np.uint64))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("box", BOXES)
def test_ball_hist2(gpu, trees, box, mode):
    t, q = trees[box], queries(box)
    L = gpu.lib()
    e2 = E2_MU if mode else E2_PI

    def call(i, o, flags):
        tot = np.zeros((len(E1), len(e2)), np.uint64)
        gpu._check(L.nbkd_query_ball_hist2(t.h, i[0], M, mode, 2, E1.ctypes.data, len(E1),
                                           e2.ctypes.data, len(e2), tot.ctypes.data, flags, None))
        return tot

    tot, _ = matrix(gpu, call, [q], [], f"ball_hist2 mode {mode}")
    assert tot.sum() > M


@pytest.mark.parametrize("mode", [0, 1])
def test_ball_hist2_obs(gpu, trees, mode):
    t, q = trees[None], queries(None)
    L = gpu.lib()
    e2 = E2_MU if mode else E2_PI

    def call(i, o, flags):
        tot = np.zeros((len(E1), len(e2)), np.uint64)
        gpu._check(L.nbkd_query_ball_hist2_obs(t.h, i[0], M, mode, OBSERVER.ctypes.data,
                                               E1.ctypes.data, len(E1), e2.ctypes.data, len(e2),
                                               tot.ctypes.data, flags, None))
        return tot

    tot, _ = matrix(gpu, call, [q], [], f"ball_hist2_obs mode {mode}")
    assert tot.sum() > M


@pytest.mark.parametrize("want_sum,want_count", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("box", BOXES)
def test_ball_sum(gpu, trees, box, want_sum, want_count):
    t, q = trees[box], queries(box)
    pts, _, _, h, _, ints, _ = inputs()
    L = gpu.lib()
    nv = 3

    def call(i, o, flags):
        gpu._check(L.nbkd_query_ball_sum(t.h, i[0], M, i[1], i[2], nv, gpu.KERNEL_TOPHAT, o[0],
                                         o[1], flags, None))

    _, (s, c) = matrix(gpu, call, [q, h, ints],
                       [((M, nv), np.float32) if want_sum else None,
                        ((M,), np.uint32) if want_count else None],
                       f"ball_sum sum {want_sum} count {want_count}")
    mem = members(pts, q, h, box)[0]
    if want_count:
        assert np.array_equal(c, mem.sum(axis=1).astype(np.uint32))
    if want_sum:  # integer values: exact in any order
        assert np.array_equal(s, (mem.astype(np.float64) @ ints).astype(np.float32))


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("box", BOXES)
def test_ball_profile(gpu, trees, box, with_scale):
    t, q = trees[box], queries(box)
    _, _, _, _, scale, ints, _ = inputs()
    L = gpu.lib()
    nr, nv = len(PROF_RADII), 2
    vals = np.ascontiguousarray(ints[:, :nv])

    def call(i, o, flags):
        gpu._check(L.nbkd_query_ball_profile(t.h, i[0], M, i[1], PROF_RADII.ctypes.data, nr, i[2],
                                             nv, o[0], flags, None))

    _, (s,) = matrix(gpu, call, [q, scale if with_scale else None, vals],
                     [((M, nr, nv), np.float32)], f"ball_profile scale {with_scale}")
    assert np.all(s == np.rint(s)) and s.sum() > M


@pytest.mark.parametrize("phi,acc", [(True, False), (False, True), (True, True)])
def test_gravity(gpu, trees, phi, acc):
    t, q = trees[None], queries(None)
    mass = inputs()[6]
    L = gpu.lib()

    def call(i, o, flags):
        gpu._check(L.nbkd_gravity(t.h, i[0], M, i[1], 0.5, 0.01, o[0], o[1], flags, None))

    _, (p, a) = matrix(gpu, call, [q, mass],
                       [((M,), np.float32) if phi else None, ((M, 3), np.float32) if acc else None],
                       f"gravity phi {phi} acc {acc}")
    assert p is None or np.all(p < 0)
    assert a is None or np.all(np.isfinite(a))


def test_gravity_ewald(gpu, trees):
    """inside queries: a query outside [0, L]^3 gets NaN rows, which == rejects"""
    t, q = trees[1.0], inputs()[1]
    mass = inputs()[6]
    L = gpu.lib()

    def call(i, o, flags):
        gpu._check(L.nbkd_gravity_ewald(t.h, i[0], M, i[1], 0.5, 0.01, o[0], o[1], flags, None))

    _, (p, a) = matrix(gpu, call, [q, mass], [((M,), np.float32), ((M, 3), np.float32)],
                       "gravity_ewald")
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(a))


@pytest.mark.parametrize("box", BOXES)
def test_ball_csr_sorted(gpu, trees, box):
    """offsets are host memory in every placement; queries and ids are placed"""
    t, q = trees[box], queries(box)
    L = gpu.lib()
    fl = gpu.NBKD_SORTED
    off0 = np.zeros(M + 1, np.uint64)
    gpu._check(L.nbkd_query_ball_csr(t.h, q.ctypes.data, M, R, off0.ctypes.data, None, 0, fl, None))
    nnz = int(off0[-1])

    def call(i, o, flags):
        off = np.zeros(M + 1, np.uint64)
        gpu._check(L.nbkd_query_ball_csr(t.h, i[0], M, R, off.ctypes.data, o[0], nnz, flags | fl,
                                         None))
        return off

    off, (ids,) = matrix(gpu, call, [q], [((nnz,), np.uint32)], "ball_csr")
    same(off, off0, "ball_csr counts pass")
    mem = members(inputs()[0], q, np.full(M, R, np.float32), box)[0]
    assert np.array_equal(np.diff(off.astype(np.int64)), mem.sum(axis=1))
    assert np.array_equal(ids, np.nonzero(mem)[1].astype(np.uint32))
