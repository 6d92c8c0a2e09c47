"""Inputs in other length units (plain helpers, no tests).

Every GPU test elsewhere places its points in [0, L]^3 with L of order 1.  The
frames below carry one base set -- points on the 2^-16 lattice of [0, 1)^3 --
to the coordinates real inputs have: kpc/h and Mpc/h boxes, scales from 2^-45
to 2^55, sets centred on 0 and sets at a large offset.  A frame maps the base
coordinates x (float64) to float32(a * x + c), with an optional periodic box.

The lattice keeps every nonzero per-axis square normal down to scale 2^-45
(the smallest is (2^-61)^2 = 2^-122), and scale 2^55 keeps d2 below overflow
(3 * 2^110 at most).  tests/test_units_inputs.py checks these conditions, and
that the C oracle is a sound reference in every frame, on the CPU.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

LATTICE = 1 << 16
NZERO = 50  # zeros frame: rows [0, 50) have x = +0.0, rows [50, 100) x = -0.0


class Frame(NamedTuple):
    name: str
    a: float            # the scale: radii, linking lengths and softenings are fractions of it
    c: float            # the offset (added after scaling)
    boxes: tuple        # the metrics the frame runs with: None and/or a periodic box
    base: str | None    # dyadic frames: the frame this one is an exact power-of-two multiple of
    exp: int = 0        # ... and the exponent e: this = 2^e * base


def _frames():
    out = [Frame("unit", 1.0, 0.0, (None, 1.0), None)]
    for e in (-45, -20, 17, 40, 55):
        out.append(Frame(f"s{e:+d}", 2.0 ** e, 0.0, (None, 2.0 ** e), "unit", e))
    for L in (205000.0, 67.77, 2.5):
        out.append(Frame(f"L{L:g}", L, 0.0, (L,), None))
    out.append(Frame("centred", 1.0, -0.5, (None,), None))
    out.append(Frame("centred17", 2.0 ** 17, -0.5 * 2.0 ** 17, (None,), "centred", 17))
    out.append(Frame("off1000", 1.0, 1000.0, (None,), None))
    out.append(Frame("off-3e5", 1.0, -3.0e5, (None,), None))
    out.append(Frame("zeros", 1.0, -0.25, (None,), None))
    return {f.name: f for f in out}


FRAMES = _frames()
DYADIC = [f.name for f in FRAMES.values() if f.base]
PERIODIC_L = ["L205000", "L67.77", "L2.5"]
# (frame, box) for every metric a frame runs with
CASES = [(f.name, box) for f in FRAMES.values() for box in f.boxes]


def case_id(case):
    name, box = case
    return name + ("-periodic" if box is not None else "")


def lattice(n, seed):
    """(n, 3) float64 coordinates i / 2^16, i in [0, 2^16), drawn without
    replacement on each axis: no two rows share a coordinate, so no split value
    is tied and the node table is pinned (which of several points tied at a
    split go left is the partition's choice).  The frames
    that collapse coordinates in float32 (off1000, off-3e5, zeros) bring such
    ties back on purpose."""
    assert n <= LATTICE
    rng = np.random.Generator(np.random.PCG64(seed))
    ints = np.stack([rng.permutation(LATTICE)[:n] for _ in range(3)], axis=1)
    return ints.astype(np.float64) / LATTICE


TIED = ("off1000", "off-3e5", "zeros")  # frames with coordinates tied on an axis


def to_frame(name, x, points=True):
    """float32(a * x + c) of base coordinates x.  Periodic frames with a
    non-dyadic box clip to float32(L).  The zeros frame shifts x by -0.5 and y,
    z by -0.25, and, for points, puts +0.0 and -0.0 on x in the first rows."""
    f = FRAMES[name]
    x = np.asarray(x, np.float64)
    if name == "zeros":
        out = (x - np.array([0.5, 0.25, 0.25])).astype(np.float32)
        if points:
            out[:NZERO, 0] = np.float32(0.0)
            out[NZERO:2 * NZERO, 0] = np.float32(-0.0)
        return out
    out = (f.a * x + f.c).astype(np.float32)
    if name in PERIODIC_L:
        out = np.minimum(out, np.float32(f.a))
    return out


@functools.lru_cache(maxsize=None)
def base_inputs(n, m, seed):
    """base points (n, 3) and the base of the queries that are no self rows"""
    return lattice(n, seed), lattice(m - m // 3, seed + 1)


@functools.lru_cache(maxsize=None)
def inputs(name, n, m, seed=9018):
    """(points, queries) of a frame, float32: the queries are the first m // 3
    points (self rows) followed by independent lattice rows.  (With this seed
    and n = 20 003 the x median of the zeros frame falls among its zero rows,
    tests/test_units_inputs.py.)"""
    bp, bq = base_inputs(n, m, seed)
    pts = to_frame(name, bp)
    q = np.concatenate([pts[:m // 3], to_frame(name, bq, points=False)])
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


def length(name, fraction):
    """`fraction` of the frame's scale as a float: float32(fraction) * a, exact
    on the dyadic frames, rounded to float32 on the others"""
    return float(np.float32(float(np.float32(fraction)) * FRAMES[name].a))


def tie_radius(d2_rows):
    """A radius r with fl(r * r) equal to a realised squared distance: the
    first nonzero entry of the (m, k) float32 array whose square root squares
    back to it (None if there is none)."""
    v = np.asarray(d2_rows, np.float32).reshape(-1)
    r = np.sqrt(v)
    ok = np.flatnonzero((v > 0) & (r * r == v))
    return float(r[ok[0]]) if ok.size else None
