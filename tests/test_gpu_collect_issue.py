"""The collect kernel's walk after its scalar-issue rework (packet.hpp: the
32-bit-offset node loads, the hand-scheduled plain-metric descent
walk_descend, and the wide-address instance larger trees take) on the
smallest shapes at which each of its paths can go wrong.  Every GPU case goes
through the C ABI and is compared with the oracle, distances bit for bit
(tests.parity.assert_knn_equal), at no more than 5e4 points."""
import json

import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import assert_knn_equal
from tests.test_gpu_collect_walk import GOLDEN, counter_cases, grid_points, read_counters

NARROW_NODES = 1 << 27  # node id * 32 B (a cell box) must fit 32 bits


def _check(gpu, oracle, pts, q, k, leaf, box, workers=8):
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    d, i = t.query(q, k)
    t.close()
    dr, ir = oracle.tree(pts, leaf, box).query(q, k, workers=workers)
    assert_knn_equal(d, i, dr, ir, pts, q, box)


@pytest.fixture
def wide(gpu):
    """The wide-address instance, forced for trees of any size."""
    saved = gpu.get_tuning("collect_wide_addr")
    gpu.set_tuning("collect_wide_addr", 1)
    yield
    gpu.set_tuning("collect_wide_addr", saved)


@pytest.mark.gpu
@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("n", [65, 128, 129])
def test_two_and_three_levels(gpu, oracle, n, k, box):
    """A root with two leaves (65, 128) or a leaf and an internal node (129):
    a pop straight to a leaf, a visit with a single wanted child (k = 1: the
    seed ball is small), both children wanted at the root (k = 32), a popped
    far child no lane wants any more."""
    pts = uniform(n, 400 + n)
    q = np.concatenate([pts, uniform(150, 500 + n)])
    _check(gpu, oracle, pts, q, k, 64, box)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 63, 65, 4 * 64 + 1])
def test_partial_packets(gpu, oracle, m):
    """Packets with invalid lanes (seed -inf: they want no node) and packet
    counts that are not a multiple of the waves per block."""
    pts = uniform(20_000, 601)
    _check(gpu, oracle, pts, uniform(m, 602 + m), 32, 64, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("box", [None, 1.0])
def test_bound_collapsing_to_zero(gpu, oracle, box):
    """k = 1 self queries on the duplicate-heavy grid: the bound tightens to
    0, and a node at distance exactly 0 is still wanted (<=)."""
    g = grid_points()
    _check(gpu, oracle, g, g, 1, 64, box)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_ties_k32", "filament_periodic_k32", "filament_open_k32"])
def test_wide_address_instance(gpu, oracle, wide, name):
    """The instance trees of 2^27 nodes or more take, forced on small ones:
    same rows, and the same traversal as the recorded one."""
    pts, q, k, leaf, box = counter_cases()[name]
    assert gpu.collect_wide_addr(1000)
    _check(gpu, oracle, pts, q, k, leaf, box)
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert read_counters(gpu, pts, q, k, leaf, box) == want


def test_host_picks_the_instance_by_node_count():
    """No device needed: the selection function alone.  Below 2^27 nodes every
    box offset (id * 32 B) fits 32 bits; from there on the wide instance."""
    from nbodyhpc_amd import capi
    saved = capi.get_tuning("collect_wide_addr")
    try:
        capi.set_tuning("collect_wide_addr", 0)
        for nodes in (0, 1, 3_200_000, NARROW_NODES - 1):
            assert not capi.collect_wide_addr(nodes), nodes
        for nodes in (NARROW_NODES, NARROW_NODES + 1, 1 << 31, (1 << 32) - 1, 1 << 40):
            assert capi.collect_wide_addr(nodes), nodes
        capi.set_tuning("collect_wide_addr", 1)
        assert capi.collect_wide_addr(1) and capi.collect_wide_addr(NARROW_NODES)
    finally:
        capi.set_tuning("collect_wide_addr", saved)
