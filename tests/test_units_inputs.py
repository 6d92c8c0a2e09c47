"""Conditions on the inputs of tests/test_gpu_units.py, checked on the CPU: in
every frame of tests/units.py the C oracle's tree agrees with its own brute
force, no per-axis square is subnormal, periodic points lie inside the box, and
the oracle is exactly equivariant under the power-of-two scalings.  With these
a failure of a GPU test points at the HIP path, not at the reference."""
import functools

import numpy as np
import pytest

from tests import units
from tests.parity import assert_knn_equal

N, M, LEAF, K = 20_000, 1500, 32, 8
TINY = np.finfo(np.float32).tiny


@functools.lru_cache(maxsize=None)
def oracle_knn(name, box):
    from oracle.oracle import Oracle
    pts, q = units.inputs(name, N, M)
    t = Oracle().tree(pts, LEAF, box)
    d, i = t.query(q, K)
    return t.export(), d, i


@pytest.mark.parametrize("case", units.CASES, ids=units.case_id)
def test_oracle_tree_equals_brute_force(oracle, case):
    name, box = case
    pts, q = units.inputs(name, N, M)
    _, d, i = oracle_knn(name, box)
    db, ib = oracle.knn_brute(pts, q, K, box)
    assert np.all(np.isfinite(d)) and np.all(d[:, 1:] >= 0)
    assert_knn_equal(d, i, db, ib, pts, q, box)
    assert np.all(d[:M // 3, 0] == 0)  # the self rows
    # a radius of about two mean spacings, one several leaves wide, a realised distance
    t = oracle.tree(pts, LEAF, box)
    d2 = t.query(q, K, sqrt=False)[0]
    radii = [units.length(name, 0.074), units.length(name, 0.2), units.tie_radius(d2[:, K - 1])]
    if box is not None:
        radii.append(units.length(name, 0.499))
    assert radii[2] is not None
    for r in radii:
        c = oracle.ball_count(t, q, r)
        assert np.array_equal(c, oracle.ball_count_brute(pts, q, r, box)), r
        assert c.max() > 1
    assert oracle.ball_count(t, q, radii[2]).max() >= K


@pytest.mark.parametrize("case", units.CASES, ids=units.case_id)
def test_no_subnormal_squares_and_points_in_box(case):
    """Per-axis d * d (and the periodic images') between 300 queries and every
    point: zero or normal, and finite when summed."""
    name, box = case
    pts, q = units.inputs(name, N, M)
    assert pts.dtype == np.float32 and np.all(np.isfinite(pts))
    if box is not None:
        assert pts.min() >= 0 and pts.max() <= np.float32(box)
        assert q.min() >= 0 and q.max() <= np.float32(box)
    d = pts[None, :, :] - q[::5, None, :]
    images = [d] if box is None else [d, d - np.float32(box), d + np.float32(box)]
    for v in images:
        s = v * v
        assert s.dtype == np.float32
        assert not np.any((s != 0) & (s < TINY))
        assert np.all(np.isfinite((s[..., 0] + s[..., 1]) + s[..., 2]))


def test_zeros_frame_has_both_zeros():
    pts, q = units.inputs("zeros", N, M)
    x = pts[:, 0]
    assert np.all(x[:2 * units.NZERO] == 0)
    assert np.all(~np.signbit(x[:units.NZERO])) and np.all(np.signbit(x[units.NZERO:2 * units.NZERO]))
    assert (x < 0).sum() > N // 3 and (x > 0).sum() > N // 3
    assert np.array_equal(q[:M // 3].view(np.uint32), pts[:M // 3].view(np.uint32))


@pytest.mark.parametrize("n", [6000, 20_003, 60_000])
def test_coordinate_ties_only_where_meant(n):
    """No two points share a coordinate on an axis (so the node table is
    pinned), except in the frames whose float32 coordinates collide."""
    for name in units.FRAMES:
        pts, _ = units.inputs(name, n, 900)
        tie_free = all(len(np.unique(pts[:, a])) == n for a in range(3))
        assert tie_free == (name not in units.TIED), name


def test_zeros_frame_splits_among_the_zeros(oracle):
    """n = 20 003: the root's split (x, the median) falls on the rows tied at
    +-0.0, with zeros of both signs on its left"""
    pts = units.inputs("zeros", 20_003, 900)[0]
    nodes = oracle.tree(pts, 16).export()[0]
    assert nodes["dim"][0] == 0 and nodes["split"][0] == 0
    below = int((pts[:, 0] < 0).sum())
    assert below + units.NZERO < (20_008 // 2) // 8 * 8 < below + 2 * units.NZERO


def test_offset_frames_are_coarse():
    """At -3e5 a float32 step is 1/32: most coordinates collide."""
    pts, _ = units.inputs("off-3e5", N, M)
    assert np.all(pts * 32 == np.round(pts * 32))
    assert len(np.unique(pts[:, 0])) <= 33
    pts, _ = units.inputs("off1000", N, M)
    assert np.all(pts * 2 ** 14 == np.round(pts * 2 ** 14))


@pytest.mark.parametrize("name", units.DYADIC)
def test_oracle_is_equivariant(name):
    """Scaling points, queries and box by 2^e multiplies the oracle's distances
    and split values by exactly 2^e and leaves indices and node ranges alone."""
    f = units.FRAMES[name]
    s = np.float32(2.0 ** f.exp)
    base = units.FRAMES[f.base]
    assert np.array_equal(units.inputs(name, N, M)[0], units.inputs(f.base, N, M)[0] * s)
    for box, bbox in zip(f.boxes, base.boxes):
        (nodes, x, y, z, idx), d, i = oracle_knn(name, box)
        (bnodes, bx, by, bz, bidx), bd, bi = oracle_knn(f.base, bbox)
        assert np.array_equal(d, bd * s) and np.array_equal(i, bi)
        for key in ("dim", "left", "right"):
            assert np.array_equal(nodes[key], bnodes[key])
        internal = nodes["dim"] >= 0
        assert np.array_equal(nodes["split"][internal], bnodes["split"][internal] * s)
        assert np.array_equal(idx, bidx)
        real = idx < N  # (padding rows are FLT_MAX in every frame)
        assert np.array_equal(x[real], bx[real] * s) and np.array_equal(z[real], bz[real] * s)
