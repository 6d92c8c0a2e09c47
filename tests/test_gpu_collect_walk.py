"""The collect kernel's packet walk (packet.hpp walk_next_leaf, knn_collect.hip
grp_packet) on the smallest shapes at which it can go wrong.  Every case goes
through the C ABI and is compared with the oracle, distances bit for bit
(tests.parity.assert_knn_equal).  The last test pins the traversal itself: six
work counters of the collect pass must equal the values recorded from the
macro walk that this walk replaced, on the same seeded inputs
(tests/golden/collect_walk_counters.json): a walk that visits one node more
or fewer has changed."""
import json
import os

import numpy as np
import pytest

from tests.golden.inputs import uniform
from tests.parity import assert_knn_equal

pytestmark = pytest.mark.gpu

COUNTERS = ("node_visits", "leaves_reached", "points_staged", "pair_evals", "candidates",
            "sparse_iters")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "collect_walk_counters.json")


def _check(gpu, oracle, pts, q, k, leaf, box, workers=8):
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    d, i = t.query(q, k)
    t.close()
    dr, ir = oracle.tree(pts, leaf, box).query(q, k, workers=workers)
    assert_knn_equal(d, i, dr, ir, pts, q, box)


@pytest.fixture
def tuning(gpu):
    saved = {n: gpu.get_tuning(n) for n in ("knn_seed_margin", "candidate_bytes")}
    yield gpu.set_tuning
    for n, v in saved.items():
        gpu.set_tuning(n, v)


# ---------------------------------------------------------------- inputs (shared with the recorder)
def grid_points():
    """4097 points on a 1/16 grid of the unit box: split values tie with query
    coordinates (q - split == 0 takes the "not right" side) and many points
    are duplicates."""
    rng = np.random.Generator(np.random.PCG64(101))
    return (rng.integers(0, 16, size=(4097, 3)).astype(np.float32) / np.float32(16.0))


def filament_points():
    """30 000 uniform points and 20 000 on a thin diagonal filament: at
    leafsize 16 the tree is deep along it and both children are wanted at many
    levels in a row."""
    rng = np.random.Generator(np.random.PCG64(102))
    bg = rng.uniform(0, 1, size=(30_000, 3))
    s = rng.uniform(0.05, 0.95, size=(20_000, 1))
    fil = s + rng.normal(0, 2e-4, size=(20_000, 3))
    pts = np.concatenate([bg, np.clip(fil, 0, 1)]).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def counter_cases():
    """name -> (points, queries, k, leafsize, boxsize): cases 2, 4 and 5."""
    g = grid_points()
    f = filament_points()
    u = uniform(20_000, 105)
    return {
        "grid_ties_k32": (g, g, 32, 64, 1.0),
        "filament_periodic_k32": (f, f[::2], 32, 16, 1.0),
        "filament_open_k32": (f, f[::2], 32, 16, None),
        "halves_k16": (u, u, 16, 128, 1.0),
        "halves_k32": (u, u, 32, 128, 1.0),
    }


def read_counters(gpu, pts, q, k, leaf, box):
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    gpu.stats_enable(True)
    try:
        t.query(q, k)
        st = gpu.stats_read_all()
    finally:
        gpu.stats_enable(False)
        t.close()
    return {n: st[n] for n in COUNTERS}


# ---------------------------------------------------------------- cases
@pytest.mark.parametrize("box", [None, 1.0])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("n", [1, 17, 64])
def test_root_is_a_leaf(gpu, oracle, n, k, box):
    """The first pop finds a leaf; k > n pads the rows."""
    pts = uniform(n, 200 + n)
    q = np.concatenate([pts, uniform(150, 300 + n)])
    _check(gpu, oracle, pts, q, k, 64, box)


def test_ties_on_split_planes(gpu, oracle):
    """Case 2: every packet is near a face (the seed balls are wide at this
    density), so the periodic instance of the walk runs."""
    g = grid_points()
    _check(gpu, oracle, g, g, 32, 64, 1.0)


def test_plain_and_periodic_packets_in_one_launch(gpu, oracle):
    """The grid set in the middle half of a box of L = 4: its own points walk
    with the plain formulas, queries spread over the whole box (near the faces
    and across them) with the periodic ones."""
    g = grid_points() * np.float32(2.0) + np.float32(1.0)
    q = np.concatenate([g, uniform(3000, 103, L=4.0)])
    _check(gpu, oracle, g, q, 32, 64, 4.0)


@pytest.mark.parametrize("box", [None, 1.0])
def test_deep_stack(gpu, oracle, box):
    f = filament_points()
    _check(gpu, oracle, f, f[::2], 32, 16, box)


@pytest.mark.parametrize("k", [16, 32])
def test_leaves_staged_as_two_halves(gpu, oracle, k):
    u = uniform(20_000, 105)
    _check(gpu, oracle, u, u, k, 128, 1.0)


def test_open_tree_with_independent_queries(gpu, oracle):
    """2000 queries far outside the data's bounding box and 2000 spread over
    it: 64 consecutive queries share little of their walks."""
    pts = uniform(100_000, 106)
    rng = np.random.Generator(np.random.PCG64(107))
    far = (rng.uniform(-1, 1, size=(2000, 3)) * 50.0 + np.where(rng.uniform(size=(2000, 3)) < 0.5,
                                                                 -100.0, 100.0)).astype(np.float32)
    q = np.concatenate([far, uniform(2000, 108)])
    _check(gpu, oracle, pts, q[rng.permutation(len(q))], 32, 64, None)


@pytest.mark.parametrize("k", [32, 100])
def test_rewalk_instances(gpu, oracle, tuning, k):
    """A tiny seed margin fails most first-pass queries: the re-walk rounds
    (the device-counted instances of the kernel) answer them; the candidate
    budget cuts the first pass into at least three batches."""
    from nbodyhpc_amd import synth
    tuning("knn_seed_margin", 0.05)
    tuning("candidate_bytes", 64 * 112 * 8 * (160 if k == 32 else 80))
    pts = synth.lognormal(30_000, 109, 1.0, grid=64)
    _check(gpu, oracle, pts, pts, k, 64, 1.0)


@pytest.mark.parametrize("name", ["grid_ties_k32", "filament_periodic_k32", "filament_open_k32",
                                  "halves_k16", "halves_k32"])
def test_same_walk_counted(gpu, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = read_counters(gpu, *counter_cases()[name])
    assert got == want
