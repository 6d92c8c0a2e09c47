"""Inputs of tests/test_gpu_collect_scan.py, shared with the recorder of its
golden arrays (tests/golden/gen_collect_scan.py).  A case is
(points, queries, k, leafsize, boxsize, tuning, group): `tuning` are
nbkd_set_tuning values for the run, `group` names the cases that share points,
queries and box, so that their sorted distances are one array of which each
case's rows are the first k columns."""
import numpy as np

from tests.golden.inputs import uniform

STEP_N = (8, 64)
STEP_M = (1, 8, 9, 16, 17, 24, 63, 64, 65)
STEP_K = (1, 8)
SHAPE_N = (1, 7, 9, 65, 129, 1000, 20000)
SHAPE_LEAF = (8, 32, 64, 128)
SHAPE_K = (1, 32, 64)
SHAPE_BOX = (None, 1.0)
FULL_MARGIN = 200.0  # knn_seed_margin at which a seed ball covers the whole 64-point leaf


def near_faces(m, seed, L, r):
    """m points of [0, L]^3, each within r of one of the six faces"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = rng.uniform(0, L, size=(m, 3))
    ax = rng.integers(0, 3, size=m)
    d = rng.uniform(0, r, size=m)
    q[np.arange(m), ax] = np.where(rng.uniform(size=m) < 0.5, d, L - d)
    return q.astype(np.float32)


def seed_radius(n, L):
    """about the k = 1 seed radius at n points in a box of side L (mu = 7
    points expected in the ball), at most a quarter of the box"""
    return min(0.25 * L, L * (7.0 / (4.18879 * max(n, 1))) ** (1.0 / 3.0))


def shape_queries(pts, n, box, seed, L=1.0):
    a, b = (min(n, 8), 4) if n < 1000 else (40, 16)
    if box is None:
        return np.concatenate([pts[:a], uniform(2 * b, seed, L=L)])
    return np.concatenate([pts[:a], uniform(b, seed, L=L),
                           near_faces(b, seed + 1, L, 0.5 * seed_radius(n, L))])


def names():
    out = [f"steps-n{n}-m{m}-k{k}" for n in STEP_N for m in STEP_M for k in STEP_K]
    out += ["full-m64", "full-m63"]
    out += [f"shape-n{n}-leaf{leaf}-k{k}-{'open' if box is None else 'box'}"
            for n in SHAPE_N for leaf in SHAPE_LEAF for k in SHAPE_K for box in SHAPE_BOX]
    out += ["units-L205000", "overflow", "byte-edge"]
    return out


def case(name):
    f = name.split("-")
    if f[0] == "steps":
        n, m, k = int(f[1][1:]), int(f[2][1:]), int(f[3][1:])
        return (uniform(n, 1100 + n), uniform(m, 1200 + 70 * n + m), k, 64, None, {},
                f"steps-n{n}-m{m}")
    if f[0] == "full":
        # every query inside the one 64-point leaf, every seed ball over all of it
        pts = uniform(64, 1300)
        return pts, pts[:int(f[1][1:])], 32, 64, None, {"knn_seed_margin": FULL_MARGIN}, name
    if f[0] == "shape":
        n, leaf, k = int(f[1][1:]), int(f[2][4:]), int(f[3][1:])
        box = None if f[4] == "open" else 1.0
        pts = uniform(n, 1400 + n)
        return (pts, shape_queries(pts, n, box, 1500 + n), k, leaf, box, {},
                f"shape-n{n}-{f[4]}")
    if name == "units-L205000":
        L = 205000.0
        pts = uniform(20000, 1600, L=L)
        return pts, shape_queries(pts, 20000, L, 1601, L=L), 32, 64, L, {}, name
    if name == "overflow":
        # 100 coincident points: more than the k = 8 column (48 slots) holds
        pts = uniform(2000, 1700)
        pts = np.concatenate([pts, np.repeat(pts[:1], 99, axis=0)])
        return pts, np.concatenate([pts[:1], uniform(15, 1701)]), 8, 64, None, {}, name
    if name == "byte-edge":
        pts, q = byte_edge(BYTE_EDGE_VOID)
        return pts, q, 128, 64, None, {}, name
    raise KeyError(name)


BYTE_EDGE_VOID = 0.2  # the seed ball (about 0.15) then holds the 255 points alone: 255 <= 256 slots


def byte_edge(void):
    """One query at the centre of a void of the background (radius `void`), 255
    coincident points at 0.05 from it: one histogram bucket of its seed ball
    counts 255.  The k = 128 column holds 256."""
    c = np.array([0.5, 0.5, 0.5], np.float32)
    bg = uniform(20000, 1800)
    bg = bg[np.linalg.norm(bg - c, axis=1) > void]
    dup = np.repeat((c + np.array([0.05, 0.0, 0.0], np.float32))[None], 255, axis=0)
    return np.concatenate([bg, dup]).astype(np.float32), c[None].copy()
