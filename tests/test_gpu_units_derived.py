"""The group, periodic-gravity and deposit kernels on coordinates away from the
unit box: nbkd_group_catalog (KDTree.fof_catalog), nbkd_group_potential
(KDTree.unbind), nbkd_gravity_ewald (KDTree.gravity_ewald) and nbkd_deposit in
the frames of tests/units.py, each against the reference its own test file
already has, with that file's bound unchanged.

Which frames a reference is sound in is decided on the CPU, by
tests/test_units_inputs.py, from the reference's own arithmetic; the lists are
imported from there.  On the power-of-two frames the GPU's outputs must also be
the base frame's scaled: 2^e commutes with every IEEE operation the kernels
perform, and the summation orders are the same."""
import functools

import numpy as np
import pytest

from tests import units
from tests.test_gpu_deposit import _close
from tests.test_gpu_gravity_ewald import check as ewald_check
from tests.test_gpu_gravity_ewald import direct as ewald_direct
from tests.test_gpu_gravity_ewald import tree_walk
from tests.test_gpu_group_catalog import compare as catalog_compare
from tests.test_gpu_group_catalog import oracle as catalog_oracle
from tests.test_gpu_group_potential import NONE, assert_within, host_minpos, unbind_ref
from tests.test_gpu_group_potential import oracle as potential_oracle
from tests.test_gpu_units import MF, NF, base_case, cases_of, fof_length, scaled
from tests.test_units_inputs import (CATALOG_CASES, CATALOG_EXACT, DEPOSIT_DYADIC, DEPOSIT_GRID,
                                     DEPOSIT_LEFT_OUT, EWALD_CASES, NE, ME,
                                     POTENTIAL_CASES, catalog_inputs, crafted_catalog_labels,
                                     deposit_frame, deposit_ref, ewald_inputs, is_normal,
                                     potential_lists, potential_masses)

pytestmark = pytest.mark.gpu

F32 = np.float32
FS = (0.5, 0.87)


def ids_of(cases):
    return [units.case_id(c) for c in cases]


# ---------------------------------------------------------------- group catalogue
def straddling_groups(pts, box, got):
    """the kept groups that lie across a face of the box and are compact: a
    member more than L/2 from the head along an axis as stored, none as
    unwrapped (dmax < L/2)"""
    head, size, off, mem, _, dmax = got
    half = F32(0.5) * F32(box)
    far = np.abs(pts[mem] - np.repeat(pts[head], size, axis=0)).max(axis=1) > half
    across = np.add.reduceat(far.astype(np.int64), off[:-1].astype(np.int64)) > 0
    return np.flatnonzero(across & (dmax < half))


@functools.lru_cache(maxsize=None)
def catalog_outputs(case):
    """the GPU's catalogues of a case: FoF labels at 0.5 and 0.87 mean spacings
    and the crafted labelling, each with min_members 1 and 2"""
    from nbodyhpc_amd import capi
    name, box = case
    pts, w, v = catalog_inputs(name)
    t = capi.Tree(pts, leafsize=32, boxsize=box)
    out = {}
    for f in FS:
        lab, siz, ng = t.fof(fof_length(name, f))
        assert 1 < ng < NF
        for mm in (1, 2):
            out[f, mm] = (lab, t.group_catalog(lab, mm, weight=w, values=v))
    lab = crafted_catalog_labels()
    for mm in (1, 2):
        out["crafted", mm] = (lab, t.group_catalog(lab, mm, weight=w, values=v))
    t.close()
    return out


@pytest.mark.parametrize("case", CATALOG_CASES, ids=ids_of(CATALOG_CASES))
def test_group_catalog(gpu, case):
    """Heads, sizes, offsets, members and dmax with ==; the float64 moments
    with == on the lattice frames (every term and partial sum is an exact
    integer multiple of the lattice step there, tests/test_units_inputs.py) and
    within compare's bound in the boxes of 205000, 67.77 and 2.5, whose
    float32(L x) is rounded.  On a periodic frame some kept group must lie
    across a face of the box."""
    name, box = case
    pts, w, v = catalog_inputs(name)
    exact = case in CATALOG_EXACT
    assert exact == (name not in units.PERIODIC_L)
    for key, (lab, got) in catalog_outputs(case).items():
        mm = key[1]
        catalog_compare(got, catalog_oracle(pts, box, lab, mm, w, v), exact=exact)
        G = len(got[0])
        assert G > 1 and got[4].shape == (G, 9)
        assert got[1].min() >= mm and (mm == 2 or len(got[3]) == NF)
        if box is not None and key[0] == 0.87:
            across = straddling_groups(pts, box, got)
            print(f"{units.case_id(case)} mm {mm}: {len(across)} of {G} groups across a face")
            assert len(across) > 0
    # the crafted sizes reach the wave-crossing combine path
    assert int(catalog_outputs(case)["crafted", 2][1][1].max()) == 513


@pytest.mark.parametrize("case", cases_of(units.DYADIC), ids=ids_of(cases_of(units.DYADIC)))
def test_group_catalog_equivariance(gpu, case):
    """A power-of-two frame's catalogue is the base frame's: lists identical,
    first moments x 2^e, the second moment x 2^2e, dmax x 2^e, the value
    channels unchanged, all under ==."""
    base, s = base_case(case)
    s = float(s)
    for key, (lab, got) in catalog_outputs(case).items():
        blab, ref = catalog_outputs(base)[key]
        assert np.array_equal(lab, blab)
        for j in range(4):
            assert np.array_equal(got[j], ref[j])
        assert np.array_equal(got[4][:, 0], ref[4][:, 0])
        assert np.array_equal(got[4][:, 1:4], ref[4][:, 1:4] * s)
        assert np.array_equal(got[4][:, 4], ref[4][:, 4] * s * s)
        assert np.array_equal(got[4][:, 5:], ref[4][:, 5:])
        assert np.array_equal(got[5], ref[5] * F32(s))
        assert got[5].max() > 0


# ---------------------------------------------------------------- KDTree.fof_catalog and the chain
CHAIN_CASES = [("L205000", 205000.0), ("L67.77", 67.77), ("s-20", 2.0 ** -20)]


def corner_clumps(L):
    """Two clumps of 65 float32 points across the corner (0, 0, 0) of a box
    float32(L), every coordinate a multiple of the float32 step u just below L
    (so L - a is exact).  Clump A: 32 pairs (a, a, a), (L - a, L - a, L - a)
    and one point at +a_33: its centre is a_33 / 65 on each axis.  Clump B: 32
    such pairs and the largest float32 below L: its centre lies u / 65 below L,
    closer to L than any float32 below L is."""
    L = F32(L)
    u = L - np.nextafter(L, F32(0))
    a = (np.arange(1, 34) * 64).astype(F32) * u
    b = (np.arange(1, 33) * 64 + 32).astype(F32) * u
    assert np.all((L - a) + a == L) and np.all((L - b) + b == L)
    A = np.concatenate([a[:32], L - a[:32], a[32:]])
    B = np.concatenate([b, L - b, [L - u]])
    assert A.dtype == F32 and B.dtype == F32 and len(A) == 65 and len(B) == 65
    return np.repeat(A[:, None], 3, 1), np.repeat(B[:, None], 3, 1), float(a[32]) / 65, float(u)


def canonical_without(lab, rows):
    """the labelling with `rows` taken out of their groups (each left as a
    singleton): every other group's label is its smallest remaining row"""
    n = len(lab)
    keep = np.ones(n, bool)
    keep[rows] = False
    rest = np.flatnonzero(keep)
    first = np.full(n, n, np.int64)
    np.minimum.at(first, lab[rest], rest)
    out = np.arange(n, dtype=np.uint32)
    out[rest] = first[lab[rest]]
    return out


@functools.lru_cache(maxsize=None)
def chain_catalogue(name, box):
    from nbodyhpc_amd.kdtree import KDTree
    pts = units.inputs(name, NF, MF)[0].copy()
    A, B, _, _ = corner_clumps(box)
    pts[:65], pts[65:130] = A, B
    # rows 130 .. 193: a chain k L / 64 along x, its member 32 exactly L/2 from the head
    pts[130:194] = np.stack([np.arange(64, dtype=F32) * (F32(box) / F32(64)),
                             np.full(64, F32(0.25) * F32(box)),
                             np.full(64, F32(0.75) * F32(box))], axis=1)
    assert pts[162, 0] - pts[130, 0] == F32(0.5) * F32(box)
    t = KDTree(pts, leafsize=32, boxsize=box)
    lab, _ = t.fof_labels(fof_length(name, 0.87))
    lab = canonical_without(lab, np.arange(194))
    lab[:65], lab[65:130], lab[130:194] = 0, 65, 130
    return pts, t, lab, t.fof_catalog(None, min_members=5, labels=lab, members=True)


@pytest.mark.parametrize("name,box", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_fof_catalog_centres_are_legal_queries(gpu, name, box):
    """`center` of KDTree.fof_catalog feeds profile, so_mass and gravity_ewald
    of the same tree: cast to float32 it must lie in [0, float32(L)), and
    neither call may answer a centre with a NaN row.  The two constructed
    groups across the corner have the centres their construction gives."""
    pts, t, lab, cat = chain_catalogue(name, box)
    L32 = F32(box)
    L = float(L32)
    assert float(t.boxsize) == L
    G = len(cat["head"])
    assert G > 1
    _, _, hand_a, u = corner_clumps(box)
    ga, gb = (int(np.flatnonzero(cat["head"] == h)[0]) for h in (0, 65))
    assert cat["size"][ga] == 65 and cat["size"][gb] == 65
    assert not cat["spans_box"][ga] and not cat["spans_box"][gb]
    assert cat["spans_box"][int(np.flatnonzero(cat["head"] == 130)[0])]  # the chain
    # float64 rounding of 65 terms below 2200 u, and of head + mean
    tol = 65 * 2.0 ** -52 * 2200 * u + 2.0 ** -52 * L
    assert np.all(np.abs(cat["center"][ga] - hand_a) <= tol)
    # clump B: u / 65 below L, the same place as 0 to within a float32 step of L
    cb = cat["center"][gb]
    away = np.minimum(np.abs(cb - (L - u / 65)), L - np.abs(cb - (L - u / 65)))
    assert np.all(away <= u / 65 + tol)
    c32 = cat["center"].astype(F32)
    assert np.all(c32 >= 0) and np.all(c32 < L32), \
        f"{np.count_nonzero(~(c32 < L32))} centre coordinates are float32(L) after the cast"
    assert np.all((cat["center"] >= 0) & (cat["center"] < L))
    radii = scaled(name, np.geomspace(0.01, 0.2, 8).astype(F32))
    prof = t.profile(cat["center"], radii)
    assert prof.shape == (G, 8) and np.all(np.isfinite(prof)) and prof.sum() > G
    assert prof[ga].sum() >= 65 and prof[gb].sum() >= 65
    phi, acc = t.gravity_ewald(cat["center"], theta=0.5, softening=units.length(name, 0.02))
    assert np.all(np.isfinite(phi)) and np.all(np.isfinite(acc)) and np.all(phi != 0)


def test_fof_catalog_spans_box_on_a_dyadic_frame(gpu):
    """spans_box (dmax >= L/2 in float32) of the 2^-20 frame is the unit
    frame's, and so are the lists; the centres scale to a float64 rounding."""
    _, _, _, cat = chain_catalogue("s-20", 2.0 ** -20)
    _, _, _, ref = chain_catalogue("unit", 1.0)
    for key in ("head", "size", "offsets", "members", "spans_box", "mass"):
        assert np.array_equal(cat[key], ref[key]), key
    assert cat["spans_box"].any() and not cat["spans_box"].all()
    assert np.allclose(cat["rms_radius"], ref["rms_radius"] * 2.0 ** -20, rtol=1e-12, atol=0)


# ---------------------------------------------------------------- group potential
@functools.lru_cache(maxsize=None)
def potential_outputs(case):
    """(offsets, members, {eps: (phi, minpos)}) with the member lists taken
    from the GPU's own catalogue at 0.87 mean spacings"""
    from nbodyhpc_amd import capi
    name, box = case
    pts = units.inputs(name, NF, MF)[0]
    off, mem = potential_lists(catalog_outputs(case)[0.87, 1][0])
    t = capi.Tree(pts, leafsize=32, boxsize=box)
    out = {eps: t.group_potential(off, mem, potential_masses(), eps=eps)
           for eps in (0.0, units.length(name, 0.02))}
    t.close()
    return off, mem, out


@pytest.mark.parametrize("case", POTENTIAL_CASES, ids=ids_of(POTENTIAL_CASES))
def test_group_potential(gpu, case):
    """The largest FoF group at 0.87 mean spacings of at most 2500 members (799
    open, 2482 periodic, 54 at -3e5 where most coordinates collide) and the
    tile-edge sizes of SIZES1, at eps 0 and 0.02 of the scale: phi == the
    float32 definition, within assert_within of the float64 sum, minpos ==
    host_minpos."""
    name, box = case
    pts = units.inputs(name, NF, MF)[0]
    off, mem, outs = potential_outputs(case)
    size = np.diff(off.astype(np.int64))
    assert size[0] >= 50 and 1025 in size and (size == 0).sum() == 2
    for eps, (phi, minpos) in outs.items():
        p32, p64, sabs = potential_oracle(pts, potential_masses(), off, mem, eps, box)
        assert is_normal(p32) and np.count_nonzero(p32) > len(mem) // 2
        assert np.array_equal(phi, p32), eps
        assert_within(phi, p64, sabs, f"{units.case_id(case)} eps {eps!r}")
        assert np.array_equal(minpos, host_minpos(phi, off))
        assert minpos[6] == NONE and minpos[0] != NONE


@pytest.mark.parametrize("case", cases_of(units.DYADIC), ids=ids_of(cases_of(units.DYADIC)))
def test_group_potential_equivariance(gpu, case):
    """phi of a power-of-two frame is the base frame's x 2^-e under ==, minpos
    equal."""
    assert case in POTENTIAL_CASES
    base, s = base_case(case)
    off, mem, outs = potential_outputs(case)
    boff, bmem, bouts = potential_outputs(base)
    assert np.array_equal(off, boff) and np.array_equal(mem, bmem)
    for (eps, (phi, minpos)), (beps, (bphi, bminpos)) in zip(outs.items(), bouts.items()):
        assert eps == beps * float(s)
        assert np.array_equal(phi, (bphi.astype(np.float64) / float(s)).astype(F32))
        assert np.array_equal(minpos, bminpos) and np.all(phi[:int(off[1])] < 0)


UNBIND_CASES = [("L205000", 205000.0), ("s-20", None)]


@pytest.mark.parametrize("name,box", UNBIND_CASES, ids=[units.case_id(c) for c in UNBIND_CASES])
def test_unbind(gpu, name, box):
    """KDTree.unbind against unbind_ref on the FoF groups of 20 or more members
    at 0.87 mean spacings that need no periodic image (unbind_ref sums open
    distances; asserted: its phi is the minimum-image phi), velocities drawn
    with a dispersion per axis of 0.6 sqrt|phi| of each member, so that the reference
    drops between 5 % and 95 % of the members."""
    from nbodyhpc_amd.kdtree import KDTree
    pts = units.inputs(name, NF, MF)[0]
    t = KDTree(pts, leafsize=32, boxsize=box)
    cat = t.fof_catalog(fof_length(name, 0.87), min_members=20, members=True)
    off, mem = cat["offsets"].astype(np.int64), cat["members"]
    if box is not None:
        half = F32(0.5) * F32(box)
        head = np.repeat(cat["head"], cat["size"])
        inner = np.add.reduceat((np.abs(pts[mem] - pts[head]).max(axis=1) >= half / 2)
                                .astype(np.int64), off[:-1]) == 0
    else:
        inner = np.ones(len(cat["size"]), bool)
    pick = np.flatnonzero(inner)[:6]
    assert len(pick) > 1
    lists = [mem[off[g]:off[g + 1]] for g in pick]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    mem = np.concatenate(lists).astype(np.uint32)
    eps = units.length(name, 0.002)
    phi0 = potential_oracle(pts, None, off, mem, eps)[0]
    assert np.array_equal(phi0, potential_oracle(pts, None, off, mem, eps, box)[0])
    assert is_normal(phi0) and np.all(phi0 < 0)
    vel = np.zeros((NF, 3))
    vel[mem] = np.random.default_rng(841).normal(0.0, 1.0, (len(mem), 3)) \
        * (0.6 * np.sqrt(np.abs(phi0.astype(np.float64))))[:, None]
    r_off, r_mem, r_energy, r_it = unbind_ref(pts, vel, off, mem, eps, 5)
    dropped = 1.0 - len(r_mem) / len(mem)
    print(f"{name}: {len(pick)} groups, {len(mem)} members, the reference drops {dropped:.1%} in "
          f"{r_it} iterations")
    assert 0.05 < dropped < 0.95 and r_it >= 2
    # no energy on a rounding edge
    assert np.abs(r_energy).min() > 1e-9 * np.abs(phi0).max()
    res = t.unbind(off, mem, vel, softening=eps, min_members=5)
    assert res["iterations"] == r_it
    assert np.array_equal(res["offsets"], r_off.astype(np.uint64))
    assert np.array_equal(res["members"], r_mem)
    # both sides form E in float64; their mean velocities differ by the order of
    # a sum of at most 800 terms: 800 * 2^-53 = 1e-13 of v^2 ~ |phi|
    assert np.all(np.abs(res["energy"] - r_energy) <= 1e-12 * np.abs(phi0).max())


# ---------------------------------------------------------------- periodic gravity
EWALD_DYADIC = [c for c in EWALD_CASES if units.FRAMES[c[0]].base]
THETAS = (0.0, 0.5)


def edge_queries(q, L):
    """q with rows on the faces: (0, 0, 0), (L, L, L), and three rows moved to
    0 or float32(L) along one axis"""
    L = F32(L)
    q = q.copy()
    q[-1], q[-2] = 0, L
    q[-3, 0], q[-4, 1], q[-5, 2] = L, 0, L
    return q


@functools.lru_cache(maxsize=None)
def ewald_outputs(case):
    from nbodyhpc_amd import capi
    name, box = case
    pts, q, mass, epss = ewald_inputs(name)
    q = edge_queries(q, box)
    t = capi.Tree(pts, leafsize=16, boxsize=box)
    exported = t.export()
    out = {(theta, eps): t.gravity_ewald(q, mass, theta=theta, eps=eps)
           for theta in THETAS for eps in epss}
    t.close()
    return exported, q, out


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("case", EWALD_CASES, ids=ids_of(EWALD_CASES))
def test_gravity_ewald_tree_oracle(gpu, case, theta):
    """Oracle B (the walk nbkd.h defines over the exported tree, its bound
    unchanged): 3003 lattice points (padding rows), leafsize 16, 300 queries, a
    third of them self rows and five on faces of the box (coordinates exactly 0
    and exactly float32(L)), theta 0 and 0.5, eps 0 and 0.02 of the scale."""
    name, box = case
    pts, _, mass, epss = ewald_inputs(name)
    exported, q, outs = ewald_outputs(case)
    assert NE % 8 != 0 and (q == F32(box)).any() and (q == 0).any()
    assert q.min() >= 0 and q.max() <= F32(box)
    for eps in epss:
        phi, acc = outs[theta, eps]
        assert np.all(np.isfinite(phi)) and np.all(np.isfinite(acc))
        s = tree_walk(exported, NE, mass, q, theta, eps, box)
        assert s.T.min() > 1 and (theta == 0 or s.accepted.sum() > 0)
        if theta == 0:
            assert np.all(s.T[:ME // 3] == NE - 1)  # the self rows
        ewald_check(phi, acc, s, f"{units.case_id(case)} theta {theta} eps {eps!r}")


@pytest.mark.parametrize("case", EWALD_DYADIC, ids=ids_of(EWALD_DYADIC))
def test_gravity_ewald_equivariance(gpu, case):
    """phi x 2^-e and acc x 2^-2e of the unit box under ==, as test_gravity
    shows for the open sum: iL, iL2 and sc are powers of two times the unit
    box's, and |d| * sc is the same float."""
    base, s = base_case(case)
    s = float(s)
    _, q, outs = ewald_outputs(case)
    _, bq, bouts = ewald_outputs(base)
    assert np.array_equal(q, bq * F32(s))
    for (phi, acc), (bphi, bacc) in zip(outs.values(), bouts.values()):
        assert np.all(phi != 0)
        assert np.array_equal(phi, (bphi.astype(np.float64) / s).astype(F32))
        assert np.array_equal(acc, (bacc.astype(np.float64) / (s * s)).astype(F32))


NA, MA = 257, 128


@pytest.mark.parametrize("name", units.PERIODIC_L)
def test_gravity_ewald_direct_sum(gpu, name):
    """Oracle A, the float64 Ewald sum with no table, in the three non-dyadic
    boxes: 257 points, 128 queries (64 of them self rows), with the
    interpolation allowance of DESIGN.md ("Interpolation error") unchanged."""
    box = units.FRAMES[name].a
    pts, q = units.inputs(name, NA, MA)
    mass = ewald_inputs(name)[2][:NA]
    q = np.concatenate([pts[:MA // 2], q[MA // 3:MA // 3 + MA // 2]])
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for eps in (0.0, units.length(name, 0.02)):
        phi, acc = t.gravity_ewald(q, mass, theta=0.0, eps=eps)
        s = ewald_direct(pts, mass, q, eps, box, True)
        assert np.all(s.T[:MA // 2] == NA - 1) and np.all(s.T[MA // 2:] == NA)
        ewald_check(phi, acc, s, f"oracle A {name} eps {eps!r}", interp=True)
    t.close()


@pytest.mark.parametrize("case", EWALD_CASES, ids=ids_of(EWALD_CASES))
def test_gravity_ewald_faces_are_one_place(gpu, case):
    """Points on a grid of 8192 float32 steps of L (p and L - p exact, none at
    L/2): a query entered at 0 and at float32(L) along any set of axes is the
    same place, every offset is the same float, and at theta = 0 the walk sums
    the same terms in the same order: the rows are equal under ==."""
    name, box = case
    L = F32(box)
    u = L - np.nextafter(L, F32(0))
    h = F32(8192) * u
    kmax = int(L / h)
    assert 1000 <= kmax <= 2048
    rng = np.random.default_rng(851)
    pts = rng.integers(1, kmax, (517, 3)).astype(F32) * h
    pts = pts[np.all(pts + pts != L, axis=1)]
    assert np.all((L - pts) + pts == L) and len(pts) > 500
    yz = rng.integers(1, kmax, (8, 3)).astype(F32) * h
    lo, hi = yz.copy(), yz.copy()
    for j in range(8):  # every subset of axes but the empty one (7 twice)
        for a in range(3):
            if (j % 7 + 1) >> a & 1:
                lo[j, a], hi[j, a] = 0, L
    mass = ewald_inputs(name)[2][:len(pts)]
    t = gpu.Tree(pts, leafsize=16, boxsize=box)
    for eps in (0.0, units.length(name, 0.02)):
        p0, a0 = t.gravity_ewald(lo, mass, theta=0.0, eps=eps)
        p1, a1 = t.gravity_ewald(hi, mass, theta=0.0, eps=eps)
        assert np.all(np.isfinite(p0)) and np.all(np.isfinite(a0)) and np.all(p0 != 0)
        assert np.array_equal(p0, p1) and np.array_equal(a0, a1)
    t.close()


@pytest.mark.parametrize("name", ["L67.77", "L205000"])
def test_gravity_ewald_wrapper_wraps_with_the_trees_box(gpu, name):
    """KDTree.gravity_ewald takes points outside the box to their wrapped
    copies: -1e-9, L, L (1 + 2^-24) and 2.5 L (L the Python float the tree was
    built with, which at 67.77 is not the tree's float32 box) each come back
    finite and equal to the result at the position wrapped by float32(L)."""
    from fractions import Fraction
    from nbodyhpc_amd.kdtree import KDTree
    L = units.FRAMES[name].a
    pts = units.inputs(name, NA, MA)[0]
    t = KDTree(pts, leafsize=16, boxsize=L)
    Lt = Fraction(float(t.boxsize))
    assert float(t.boxsize) == float(F32(L))
    coords = [-1e-9, L, L * (1 + 2.0 ** -24), 2.5 * L]
    q = np.array([[c, 0.25 * L, 0.75 * L] for c in coords]
                 + [[0.5 * L, c, 0.125 * L] for c in coords]
                 + [[c, c, c] for c in coords])

    def wrapped(c):
        w = Fraction(c) - Lt * (Fraction(c) // Lt)
        w = F32(float(w))
        return F32(0) if w >= F32(L) else w

    qw = np.array([[wrapped(c) for c in row] for row in q], F32)
    assert np.all(qw >= 0) and np.all(qw < F32(L))
    eps = units.length(name, 0.02)
    phi, acc = t.gravity_ewald(q, softening=eps, theta=0.5)
    wphi, wacc = t.gravity_ewald(qw.astype(np.float64), softening=eps, theta=0.5)
    assert np.all(np.isfinite(phi)) and np.all(np.isfinite(acc)) and np.all(phi != 0)
    assert np.array_equal(phi, wphi) and np.array_equal(acc, wacc)


# ---------------------------------------------------------------- deposit
DEPOSIT_ADMITTED = [n for n in DEPOSIT_DYADIC if n not in DEPOSIT_LEFT_OUT]
DEPOSIT_CASES = [(n, p) for n in ["unit"] + DEPOSIT_ADMITTED + units.PERIODIC_L
                 for p in (False, True)]
DEPOSIT_OUTSIDE = ["centred", "centred17", "zeros", "off1000", "off-3e5"]


def gpu_deposit(name, periodic, window=None):
    from nbodyhpc_amd import capi
    p, w, r, ppu, period = deposit_frame(name, periodic)
    return capi.deposit(p, w, r, DEPOSIT_GRID, ppu, period=period, window=window)


@pytest.mark.parametrize("name,periodic", DEPOSIT_CASES,
                         ids=[n + ("-periodic" if p else "") for n, p in DEPOSIT_CASES])
def test_deposit(gpu, name, periodic):
    """300 balls of radii 0.05 to 2.5 of the scale on a 40 x 33 x 29 grid at
    ppu = 4 / a against the oracle in the same frame, RTOL and ATOL_FRAC
    unchanged.  The ball's volume is formed in voxels (o = r * ppu), so a grid
    value is weight per voxel and does not see the unit: on the dyadic frames
    the grid is also compared with the unit frame's oracle, with no factor.
    The kernel adds with float32 atomics in no fixed order, so == between two
    GPU grids would be the wrong demand; the tolerance is the demand."""
    got = gpu_deposit(name, periodic)
    ref = deposit_ref(name, periodic)
    assert got.shape == DEPOSIT_GRID and got.dtype == F32
    assert np.count_nonzero(got) > got.size // 10 and ref.max() > 0
    _close(got, ref)
    if name in DEPOSIT_ADMITTED:
        _close(got, deposit_ref("unit", periodic))


def test_deposit_column_window_at_205000(gpu):
    got = gpu_deposit("L205000", True, window=(13, 14))
    assert got.shape == (14, 33, 29) and np.count_nonzero(got) > 0
    _close(got, deposit_ref("L205000", True)[13:27])


@pytest.mark.parametrize("name", DEPOSIT_OUTSIDE)
def test_deposit_mostly_outside_the_grid(gpu, name):
    """The grid's origin is 0: the centred frames (the set shifted by half its
    box, 1/8 of the centres inside) and the offset frames (the whole set 1000
    boxes above or 3e5 below the grid: every clamp of a sprite range is taken
    and nothing is written) run once, non-periodic."""
    got = gpu_deposit(name, False)
    ref = deposit_ref(name, False)
    _close(got, ref)
    if name.startswith("off"):
        assert not ref.any() and not got.any()
    else:
        assert np.count_nonzero(got) > 0 and np.count_nonzero(ref) > 0
