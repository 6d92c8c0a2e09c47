"""The collect kernel's one-chunk instance (knn_collect.hip grp_packet ONE: a
tree with leaf size <= 64 stages every leaf whole, once, with no chunk loop
and no half-leaf boxes, its staging loads at 32-bit offsets) on the smallest
shapes at which it can go wrong, and the host's choice between it and the
general instance.  Every GPU case goes through the C ABI at no more than 5e4
points: rows against the oracle (tests.parity.assert_knn_equal, distances bit
for bit), and the two instances against each other in one library (the
"collect_one_chunk" knob): equal distances, equal ids, equal work counters."""
import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import assert_knn_equal
from tests.test_gpu_collect_walk import COUNTERS

KNOB = "collect_one_chunk"
P4_POINTS = 1 << 28          # points * 16 B (a staged point) must fit 32 bits
GROUP_POINTS = 1431655768    # the first multiple of 8 with points / 8 * 24 B >= 2^32
LEAF_NODES = 1 << 27         # node id * 32 B (a leaf's tight box) must fit 32 bits


@pytest.fixture
def knobs(gpu):
    names = (KNOB, "knn_seed_margin", "candidate_bytes")
    saved = {n: gpu.get_tuning(n) for n in names}
    yield gpu.set_tuning
    for n, v in saved.items():
        gpu.set_tuning(n, v)


def _run(gpu, pts, q, k, leaf, box):
    """Rows from the plain instance, then rows and the six work counters from
    the instrumented one (the form the pinned counter tests read)."""
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    try:
        d, i = t.query(q, k)
        gpu.stats_enable(True)
        try:
            ds, is_ = t.query(q, k)
            st = gpu.stats_read_all()
        finally:
            gpu.stats_enable(False)
    finally:
        t.close()
    assert np.array_equal(d, ds) and np.array_equal(i, is_)
    return d, i, {n: st[n] for n in COUNTERS}


def _both_paths(gpu, knobs, oracle, pts, q, k, leaf, box, one):
    """Oracle parity under the default, and knob on against knob off.  `one`:
    the host must pick the one-chunk instance for this tree when the knob is on."""
    knobs(KNOB, 1)
    assert gpu.collect_instance(leaf, len(pts), 1)[0] == one
    d1, i1, c1 = _run(gpu, pts, q, k, leaf, box)
    dr, ir = oracle.tree(pts, leaf, box).query(q, k, workers=8)
    assert_knn_equal(d1, i1, dr, ir, pts, q, box)
    knobs(KNOB, 0)
    assert not gpu.collect_instance(leaf, len(pts), 1)[0]
    d0, i0, c0 = _run(gpu, pts, q, k, leaf, box)
    assert np.array_equal(d1, d0)
    assert np.array_equal(i1, i0)
    assert c1 == c0


@pytest.mark.gpu
@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 129])
def test_small_trees(gpu, oracle, knobs, n, k, box):
    """A single leaf, a padded last leaf, leaves of every multiple of 8 and the
    leaf at the very end of the point array (its staging must not read past
    the points or the group boxes)."""
    pts = uniform(n, 700 + n)
    q = np.concatenate([pts, uniform(150, 800 + n)])
    _both_paths(gpu, knobs, oracle, pts, q, k, 64, box, True)


@pytest.mark.gpu
@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("leaf", [8, 32, 64])
def test_one_chunk_leaf_sizes(gpu, oracle, knobs, leaf, k, box):
    pts = uniform(20_000, 901)
    q = np.concatenate([pts[::4], uniform(1000, 902)])
    _both_paths(gpu, knobs, oracle, pts, q, k, leaf, box, True)


@pytest.mark.gpu
@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("leaf", [65, 128, 200])
def test_larger_leaves_take_the_general_instance(gpu, oracle, knobs, leaf, k, box):
    """The halves path (65, 128) and the runs-of-64 path (200): unchanged code,
    which the host must still pick."""
    pts = uniform(20_000, 903)
    q = np.concatenate([pts[::4], uniform(1000, 904)])
    _both_paths(gpu, knobs, oracle, pts, q, k, leaf, box, False)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [32, 100])
def test_rewalk_rounds(gpu, oracle, knobs, k):
    """A tiny seed margin fails most first-pass queries, so the device-counted
    instances of the kernel answer them: knob on against knob off."""
    from nbodyhpc_amd import synth
    knobs("knn_seed_margin", 0.05)
    knobs("candidate_bytes", 64 * 112 * 8 * (160 if k == 32 else 80))
    pts = synth.lognormal(30_000, 905, 1.0, grid=64)
    rows = []
    for on in (1, 0):
        knobs(KNOB, on)
        t = gpu.Tree(pts, leafsize=64, boxsize=1.0)
        rows.append(t.query(pts, k))
        t.close()
    dr, ir = oracle.tree(pts, 64, 1.0).query(pts, k, workers=8)
    assert_knn_equal(rows[0][0], rows[0][1], dr, ir, pts, pts, 1.0)
    assert np.array_equal(rows[0][0], rows[1][0])
    assert np.array_equal(rows[0][1], rows[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 63, 65, 4 * 64 + 1])
def test_packet_counts_off_the_block_size(gpu, oracle, knobs, m):
    """Packet counts that are not a multiple of the first pass's waves per
    block: the last block's spare waves take no packet."""
    pts = uniform(20_000, 906)
    _both_paths(gpu, knobs, oracle, pts, uniform(m, 907 + m), 32, 64, 1.0, True)


def test_host_picks_the_one_chunk_instance_by_leaf_size():
    """No device needed.  Leaf sizes up to 64 (the staged chunk) have no
    half-leaf boxes and one chunk per leaf; the knob turns the instance off."""
    from nbodyhpc_amd import capi
    saved = capi.get_tuning(KNOB), capi.get_tuning("collect_wide_addr")
    try:
        capi.set_tuning("collect_wide_addr", 0)
        capi.set_tuning(KNOB, 1)
        for leaf in (1, 8, 16, 32, 63, 64):
            assert capi.collect_instance(leaf, 100_000_000, 3_200_000) == (True, True), leaf
        for leaf in (65, 128, 200, 1 << 20):
            assert capi.collect_instance(leaf, 100_000_000, 3_200_000) == (False, True), leaf
        capi.set_tuning(KNOB, 0)
        assert capi.collect_instance(64, 100_000_000, 3_200_000) == (False, True)
        # the wide-address knob forces the wide form of all of it
        capi.set_tuning(KNOB, 1)
        capi.set_tuning("collect_wide_addr", 1)
        assert capi.collect_instance(64, 1000, 31) == (True, False)
        assert capi.collect_instance(128, 1000, 31) == (False, False)
    finally:
        capi.set_tuning(KNOB, saved[0])
        capi.set_tuning("collect_wide_addr", saved[1])


def test_host_checks_every_staging_offset():
    """No device needed.  Each of the three byte offsets just below and just
    above 2^32; a one-chunk tree that fails any takes the wide form, a tree of
    larger leaves is judged by its node count alone, as before."""
    from nbodyhpc_amd import capi
    assert capi.collect_stage_offsets(0, 0) == (True, True, True)
    # points are padded to a multiple of 8 first
    assert capi.collect_stage_offsets(P4_POINTS - 8, 1) == (True, True, True)
    assert capi.collect_stage_offsets(P4_POINTS - 7, 1) == (False, True, True)
    assert capi.collect_stage_offsets(P4_POINTS, 1) == (False, True, True)
    assert capi.collect_stage_offsets(GROUP_POINTS - 8, 1) == (False, True, True)
    assert capi.collect_stage_offsets(GROUP_POINTS - 7, 1) == (False, False, True)
    assert capi.collect_stage_offsets(GROUP_POINTS, 1) == (False, False, True)
    assert capi.collect_stage_offsets(8, LEAF_NODES - 1) == (True, True, True)
    assert capi.collect_stage_offsets(8, LEAF_NODES) == (True, True, False)
    assert capi.collect_stage_offsets(1 << 40, 1 << 40) == (False, False, False)
    saved = capi.get_tuning(KNOB), capi.get_tuning("collect_wide_addr")
    try:
        capi.set_tuning("collect_wide_addr", 0)
        capi.set_tuning(KNOB, 1)
        assert capi.collect_instance(64, P4_POINTS - 8, 1 << 23) == (True, True)
        assert capi.collect_instance(64, P4_POINTS, 1 << 23) == (True, False)
        assert capi.collect_instance(64, 8, LEAF_NODES - 1) == (True, True)
        assert capi.collect_instance(64, 8, LEAF_NODES) == (True, False)
        assert capi.collect_instance(128, P4_POINTS, 1 << 23) == (False, True)
        assert capi.collect_instance(128, 8, LEAF_NODES) == (False, False)
    finally:
        capi.set_tuning(KNOB, saved[0])
        capi.set_tuning("collect_wide_addr", saved[1])
