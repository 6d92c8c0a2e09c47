"""Conditions on the inputs of tests/test_gpu_units.py, checked on the CPU: in
every frame of tests/units.py the C oracle's tree agrees with its own brute
force, no per-axis square is subnormal, periodic points lie inside the box, and
the oracle is exactly equivariant under the power-of-two scalings.  With these
a failure of a GPU test points at the HIP path, not at the reference.

The second half does the same for tests/test_gpu_units_derived.py: for the
references of the group catalogue, the group potential, periodic gravity and
the deposit it decides, from the reference's own float32 steps, the frames in
which each is sound, and prints the frames admitted and left out."""
import functools

import numpy as np
import pytest

from tests import units
from tests.parity import assert_knn_equal
from tests.test_gpu_deposit import _particles
from tests.test_gpu_fof import brute_labels
from tests.test_gpu_gravity import masses as unit_masses
from tests.test_gpu_gravity_ewald import wrap32
from tests.test_gpu_group_catalog import SIZES, crafted_labels
from tests.test_gpu_group_catalog import oracle as catalog_oracle
from tests.test_gpu_group_potential import SIZES1, csr, group_d
from tests.test_gpu_units import MF, NF, fof_length

from . import ewald_oracle as eo

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


# ================================================================ derived kernels
# The references of tests/test_gpu_units_derived.py (group catalogue, group
# potential, periodic gravity, deposit): the frames each of them is sound in.
# The lists below are what the GPU file imports; each is asserted here to be
# exactly what the reference's own arithmetic admits, so no frame is chosen by
# looking at the GPU's answer and none is left out by hand.
F32 = np.float32
PERIODIC_CASES = [c for c in units.CASES if c[1] is not None]

# group catalogue: every frame runs; == where the lattice makes every sum exact
CATALOG_CASES = list(units.CASES)
CATALOG_EXACT = [c for c in units.CASES if c[0] not in units.PERIODIC_L]
# group potential: every frame (its terms are m / sqrt(d2 + eps2), never a cube)
POTENTIAL_CASES = list(units.CASES)
POTENTIAL_LEFT_OUT = {}
# periodic gravity: the Newtonian term forms inv^3 in float32
EWALD_CASES = [c for c in PERIODIC_CASES if c[0] not in ("s-45", "s+55")]
EWALD_LEFT_OUT = {"s-45": "inv^3 overflows", "s+55": "inv^3 underflows"}
# deposit: the dyadic scales a (positions a x, radii a r, ppu = 4 / a)
DEPOSIT_DYADIC = ["s-45", "s-20", "s+17", "s+40", "s+55"]
DEPOSIT_LEFT_OUT = {}


def is_normal(v):
    """finite, and zero or of normal magnitude, in the array's own dtype"""
    v = np.asarray(v)
    return bool(np.all(np.isfinite(v)) and not np.any((v != 0) & (np.abs(v) < np.finfo(v.dtype).tiny)))


def why_not_normal(v):
    v = np.asarray(v)
    if np.any(np.isnan(v)):
        return "is NaN"
    if np.any(np.isinf(v)):
        return "overflows"
    if np.any((v != 0) & (np.abs(v) < np.finfo(v.dtype).tiny)):
        return "underflows"
    return None


# ---------------------------------------------------------------- group catalogue
@functools.lru_cache(maxsize=None)
def catalog_inputs(name):
    """(points, integer weights 1..8, two integer value channels -7..7)"""
    pts, _ = units.inputs(name, NF, MF)
    rng = np.random.default_rng(811)
    w = rng.integers(1, 9, NF).astype(F32)
    v = rng.integers(-7, 8, (NF, 2)).astype(F32)
    w.setflags(write=False)
    v.setflags(write=False)
    return pts, w, v


def crafted_catalog_labels():
    return crafted_labels(NF, SIZES, 812)


def common_grid(values):
    """the largest power of two g with every value an integer multiple of it"""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[v != 0]
    m, e = np.frexp(v)
    k = (np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = np.log2((k & -k).astype(np.float64)).astype(np.int64)  # trailing zeros
    return 2.0 ** int((e - 53 + low).min())


@pytest.mark.parametrize("case", CATALOG_CASES, ids=units.case_id)
def test_group_catalogue_reference_is_exact_on_the_lattice(case):
    """Off the three non-dyadic boxes the NF points (and the box) lie on one
    power-of-two grid g a few 2^17 steps wide: every float32 p - head (and its
    image) is exact, and with integer weights 1..8 every float64 term and every
    partial sum of any subset is an integer below 2^53 in units of g (g^2): the
    numpy oracle's moments equal integer arithmetic's and do not depend on the
    summation order, so the GPU test may demand ==."""
    name, box = case
    pts, w, v = catalog_inputs(name)
    if case not in CATALOG_EXACT:
        assert name in units.PERIODIC_L
        print(f"catalogue {units.case_id(case)}: relative bound (float32(L x) is rounded and clipped)")
        return
    g = common_grid(pts if box is None else np.concatenate([pts.reshape(-1), [F32(box)]]))
    n = pts.astype(np.float64) / g
    assert np.array_equal(n, np.round(n)) and np.abs(n).max() < 2.0 ** 53
    n = n.astype(np.int64)
    w64 = w.astype(np.int64)
    worst = 0.0
    for lab in (crafted_catalog_labels(), np.zeros(NF, np.uint32)):  # one group of all: any subset
        head, size, off, rows, mom, dmax, ab = catalog_oracle(pts, box, lab, 1, w, v)
        rows = rows.astype(np.int64)
        d = n[rows] - n[lab[rows]]
        if box is not None:
            Lg = int(round(float(F32(box)) / g))
            assert Lg * g == float(F32(box))
            r = d.copy()
            r = np.where(np.abs(d - Lg) < np.abs(r), d - Lg, r)
            r = np.where(np.abs(d + Lg) < np.abs(r), d + Lg, r)
            d = r
        assert np.abs(d).max() < 2 ** 24  # a float32 holds it: p - head is exact
        seg = off[:-1].astype(np.int64)
        ww = w64[rows]
        m1 = np.add.reduceat(ww[:, None] * d, seg, axis=0)
        m2 = np.add.reduceat(ww * (d * d).sum(axis=1), seg)
        assert np.array_equal(mom[:, 0], np.add.reduceat(ww, seg).astype(np.float64))
        assert np.array_equal(mom[:, 1:4], m1.astype(np.float64) * g)
        assert np.array_equal(mom[:, 4], m2.astype(np.float64) * g * g)
        assert np.array_equal(dmax, (np.maximum.reduceat(np.abs(d).max(axis=1), seg) * g).astype(F32))
        assert np.array_equal(mom[:, 5:], np.round(mom[:, 5:]))
        # sum |t| bounds every partial sum of every order
        worst = max(worst, float(ab[:, 1:4].max() / g), float(ab[:, 4].max() / (g * g)),
                    float(ab[:, 5:].max()))
    print(f"catalogue {units.case_id(case)}: exact, g = 2^{int(np.log2(g))}, largest sum |t| "
          f"2^{np.log2(worst):.1f} steps")
    assert worst < 2.0 ** 53


@pytest.mark.parametrize("name", units.DYADIC)
def test_group_catalogue_inputs_scale(name):
    f = units.FRAMES[name]
    a, b = catalog_inputs(name), catalog_inputs(f.base)
    assert np.array_equal(a[0], b[0] * F32(2.0 ** f.exp))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- group potential
@functools.lru_cache(maxsize=None)
def fof_labels_ref(name, box, f):
    """brute-force FoF labels of the NF points at f mean spacings.  A dyadic
    frame has its base frame's labels: 2^e commutes with d2 <= b2 (asserted for
    the distances by test_oracle_is_equivariant)."""
    fr = units.FRAMES[name]
    if fr.base:
        return fof_labels_ref(fr.base, None if box is None else box / fr.a, f)
    return brute_labels(units.inputs(name, NF, MF)[0], fof_length(name, f), box)


def potential_lists(labels):
    """(offsets, members): the largest group of a labelling with at most 2500
    members (the oracle is O(size^2) in time and memory), rows ascending, then
    SIZES1 dealt from a fixed shuffle of all rows"""
    lab = np.asarray(labels)
    cnt = np.bincount(lab)
    cnt[cnt > 2500] = 0
    big = np.flatnonzero(lab == cnt.argmax()).astype(np.uint32)
    dealt = np.random.default_rng(821).permutation(NF)[:sum(SIZES1)].astype(np.uint32)
    return csr([len(big)] + list(SIZES1)), np.concatenate([big, dealt])


def potential_masses():
    return unit_masses(NF, 822)


def potential_terms(pts, mass, off, mem, eps, L):
    """the float32 d2, inv and m * inv of every ordered pair of every group, as
    test_gpu_group_potential.oracle forms them"""
    eps2 = F32(eps) * F32(eps)
    out = []
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        if b - a < 2:
            continue
        rows = mem[a:b]
        d = group_d(pts[rows], L)
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        on = d2 != 0
        with np.errstate(all="ignore"):
            inv = F32(1.0) / np.sqrt(d2 + eps2)
            t = mass[rows][None, :] * inv
        assert t.dtype == F32
        out.append((d2[on], inv[on], t[on]))
    return [np.concatenate([o[j] for o in out]) for j in range(3)]


def potential_verdict(case):
    """None if the float32 reference stays inside float32 at eps = 0 and 0.02
    of the scale, else what leaves it"""
    name, box = case
    pts = units.inputs(name, NF, MF)[0]
    off, mem = potential_lists(fof_labels_ref(name, box, 0.87))
    for eps in (0.0, units.length(name, 0.02)):
        for what, v in zip(("d2", "1 / sqrt(d2 + eps2)", "m / sqrt(d2 + eps2)"),
                           potential_terms(pts, potential_masses(), off, mem, eps, box)):
            assert v.size > 1000
            why = why_not_normal(v)
            if why:
                return f"{what} {why} (eps {eps!r})"
    return None


@pytest.mark.parametrize("case", units.CASES, ids=units.case_id)
def test_group_potential_reference_stays_in_float32(case):
    verdict = potential_verdict(case)
    print(f"potential {units.case_id(case)}: {'admitted' if verdict is None else 'left out: ' + verdict}")
    assert (verdict is None) == (case in POTENTIAL_CASES), verdict
    if verdict is not None:
        assert POTENTIAL_LEFT_OUT[case[0]] in verdict


# ---------------------------------------------------------------- periodic gravity
NE, ME = 3003, 300


def ewald_inputs(name):
    pts, q = units.inputs(name, NE, ME)
    return pts, q, unit_masses(NE, 831), (0.0, units.length(name, 0.02))


def ewald_verdict(case):
    """None if nbkd.h's float32 steps stay normal between the ME queries and
    the NE points: iL, iL2, sc, mu iL2 (mu from the lightest point to the whole
    set) and the Newtonian term's inv, inv^3 and mu inv^3"""
    name, box = case
    pts, q, mass, epss = ewald_inputs(name)
    L = F32(box)
    with np.errstate(all="ignore"):
        iL = F32(1.0) / L
        iL2 = iL * iL
        sc = F32(128.0) * iL
        mus = np.array([mass.min(), mass.max(), mass.sum(dtype=np.float64)], F32)
        for what, v in (("iL", iL), ("iL2", iL2), ("sc", sc), ("mu iL", mus * iL), ("mu iL2", mus * iL2)):
            why = why_not_normal(v)
            if why:
                return f"{what} {why}"
        d = wrap32(pts[None, :, :] - q[:, None, :], L)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        on = d2 != 0
        for eps in epss:
            inv = F32(1.0) / np.sqrt(d2[on] + F32(eps) * F32(eps))
            inv3 = (inv * inv) * inv
            w = np.broadcast_to(mass[None, :], d2.shape)[on] * inv3
            assert w.dtype == F32
            for what, v in (("d2", d2[on]), ("inv", inv), ("inv^3", inv3), ("mu inv^3", w)):
                why = why_not_normal(v)
                if why:
                    return f"{what} {why} (eps {eps!r})"
    return None


@pytest.mark.parametrize("case", PERIODIC_CASES, ids=units.case_id)
def test_ewald_reference_stays_in_float32(case):
    verdict = ewald_verdict(case)
    print(f"ewald {units.case_id(case)}: {'admitted' if verdict is None else 'left out: ' + verdict}")
    assert (verdict is None) == (case in EWALD_CASES), verdict
    if verdict is not None:
        assert EWALD_LEFT_OUT[case[0]] in verdict


@pytest.mark.parametrize("name", [n for n in units.DYADIC if units.FRAMES[n].boxes[-1] is not None])
def test_ewald_interpolation_does_not_see_the_unit(name):
    """eo.interpolate (the table in nbkd.h's float32 steps) over the wrapped
    offsets of a dyadic frame returns the base frame's values and corner maxima
    exactly: |d| * sc is the same float."""
    from nbodyhpc_amd import capi
    f = units.FRAMES[name]
    table = capi.ewald_table()
    pts, q = units.inputs(name, NE, ME)
    bpts, bq = units.inputs(f.base, NE, ME)
    d = wrap32(pts[None, ::7, :] - q[:, None, :], f.a).reshape(-1, 3)
    bd = wrap32(bpts[None, ::7, :] - bq[:, None, :], 1.0).reshape(-1, 3)
    assert np.array_equal(d, bd * F32(f.a))
    got, cmax = eo.interpolate(table, d, f.a)
    ref, rmax = eo.interpolate(table, bd, 1.0)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and np.array_equal(cmax, rmax)
    assert len(d) > 100_000 and np.abs(bd).max() == 0.5


# ---------------------------------------------------------------- deposit
DEPOSIT_GRID, DEPOSIT_PPU = (40, 33, 29), 4.0
DEPOSIT_BOX = np.array(DEPOSIT_GRID) / DEPOSIT_PPU


@functools.lru_cache(maxsize=None)
def deposit_unit(periodic):
    """the set of test_volume_mixed_radii, 300 particles: radii 0.05 (below a
    voxel) to 2.5 (half the box) in a 10 x 8.25 x 7.25 box at 4 voxels per unit"""
    xyz, w, r = _particles(np.random.default_rng(11 + periodic), 300, DEPOSIT_BOX,
                           [0.05, 0.2, 0.5, 1.3, 2.5])
    for a in (xyz, w, r):
        a.setflags(write=False)
    return xyz, w, r


def deposit_frame(name, periodic):
    """(xyz, w, r, ppu, period) of a frame: positions a x (+ c box on the
    centred and offset frames: the grid's origin stays 0), radii a r, ppu =
    4 / a.  Exact on the dyadic frames, rounded to float32 on the others."""
    f = units.FRAMES[name]
    xyz, w, r = deposit_unit(periodic)
    if name == "zeros":
        shift = np.array([-0.5, -0.25, -0.25]) * DEPOSIT_BOX
    else:
        shift = f.c / f.a * DEPOSIT_BOX
    p = (f.a * (xyz.astype(np.float64) + shift)).astype(F32)
    rr = (f.a * r.astype(np.float64)).astype(F32)
    period = tuple(float(v) for v in (f.a * DEPOSIT_BOX).astype(F32)) if periodic else (-1.0,) * 3
    return p, w, rr, float(F32(DEPOSIT_PPU / f.a)), period


@functools.lru_cache(maxsize=None)
def deposit_ref(name, periodic):
    from oracle.oracle import Oracle
    p, w, r, ppu, period = deposit_frame(name, periodic)
    g = Oracle().deposit(p, w, r, DEPOSIT_GRID, ppu, period, 4, 0)
    g.setflags(write=False)
    return g


def deposit_verdict(name):
    """None if the oracle's float32 steps that see the unit stay normal and its
    grid is the unit frame's, else what fails.

    The oracle (and the kernel) form the ball's volume from o = r * ppu, in
    voxels: dens = w / (4/3 pi o^3) never sees the length unit, and a grid value
    is weight per voxel.  Scaling (x, r, ppu) to (a x, a r, ppu / a) therefore
    leaves the grid unchanged (a factor a^0, not a^-3).  What does see the unit
    is x * ppu, r * ppu, (z -+ r) * ppu, the slice planes s / ppu, z - depth
    and r * r - zoff * zoff."""
    for periodic in (False, True):
        p, w, r, ppu, period = deposit_frame(name, periodic)
        with np.errstate(all="ignore"):
            o = r * F32(ppu)
            checks = (("ppu", F32(ppu)), ("1 / ppu", F32(1.0 / ppu)), ("r * r", r * r),
                      ("r^3 in voxels", (o * o) * o),
                      ("w / volume", w / (F32(4.0) / F32(3.0) * F32(3.14159265358979) * o * o * o)),
                      ("x * ppu", p * F32(ppu)))
        for what, v in checks:
            why = why_not_normal(v)
            if why:
                return f"{what} {why}"
        if not np.array_equal(deposit_ref(name, periodic), deposit_ref("unit", periodic)):
            return "the oracle's grid is not the unit frame's"
    return None


@pytest.mark.parametrize("name", DEPOSIT_DYADIC)
def test_deposit_oracle_does_not_see_the_unit(name):
    verdict = deposit_verdict(name)
    print(f"deposit {name}: {'admitted' if verdict is None else 'left out: ' + verdict}")
    if name in ("s-20", "s+17"):
        assert verdict is None
    assert (verdict is None) == (name not in DEPOSIT_LEFT_OUT), verdict
    if verdict is not None:
        assert DEPOSIT_LEFT_OUT[name] in verdict
    assert deposit_ref("unit", True).max() > 0


@pytest.mark.parametrize("name", ["unit"] + units.PERIODIC_L)
def test_deposit_oracle_keeps_the_weight(name):
    """Non-dyadic boxes round a x and a r, so single sub-samples change side;
    the periodic grid must still hold the total weight (1) to the S^3 sampling
    error, the 0.02 of test_knn_smoothing_lengths_feed_the_deposit."""
    p, w, r, ppu, period = deposit_frame(name, True)
    from oracle.oracle import Oracle
    w1 = (w / w.sum(dtype=np.float64)).astype(F32)
    total = float(Oracle().deposit(p, w1, r, DEPOSIT_GRID, ppu, period, 4, 0).sum())
    print(f"deposit {name}: periodic grid total {total:.5f}")
    assert abs(total - 1.0) < 0.02
