"""Per-group potentials (nbkd_group_potential, group_potential.hip) against two
numpy oracles written here.  New (no reference counterpart).

oracle32 evaluates nbkd.h's definition: float32 d, d2, r2, inv and m*inv (on a
periodic tree the per-axis minimum over the three images), then a sequential
float64 sum (cumsum) in list order, negated and rounded to float32.  Square
root and division are correctly rounded on both sides, so out_phi is compared
with ==.  oracle64 forms the terms in float64 from the float32 d; the bound is
|phi - phi64| <= 17 * 2^-24 * sum |t|: fewer than 16 roundings per term (as in
test_gpu_gravity.py) plus the final rounding to float32; the float64 sum's own
error is below 2^-40 of that."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
NONE = 0xFFFFFFFF


# ---------------------------------------------------------------- oracles
def group_d(P, L):
    """d[i, j] = p_j - p_i in float32; periodic: the per-axis minimum image"""
    d = P[None, :, :] - P[:, None, :]
    if L is not None:
        L = np.float32(L)
        d = np.minimum(np.minimum(np.abs(d), np.abs(d - L)), np.abs(d + L))
    assert d.dtype == np.float32
    return d


def oracle(pts, mass, off, mem, eps, L=None):
    """(phi32 (K,) float32 by the definition, phi64 (K,), sum |t| (K,))"""
    K = len(mem)
    phi32, phi64, sabs = np.zeros(K, np.float32), np.zeros(K), np.zeros(K)
    eps2 = np.float32(eps) * np.float32(eps)
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        if a == b:
            continue
        rows = mem[a:b]
        m = np.ones(b - a, np.float32) if mass is None else mass[rows].astype(np.float32)
        d = group_d(pts[rows], L)
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        on = d2 != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.float32(1.0) / np.sqrt(d2 + eps2)
            t = m[None, :] * inv
        assert d2.dtype == np.float32 and inv.dtype == np.float32 and t.dtype == np.float32
        t = np.where(on, t, np.float32(0.0))
        phi32[a:b] = (-(t.astype(np.float64).cumsum(axis=1)[:, -1])).astype(np.float32)
        d64 = d.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t64 = m[None, :].astype(np.float64) / np.sqrt((d64 * d64).sum(axis=2)
                                                          + float(np.float32(eps)) ** 2)
        t64 = np.where(on, t64, 0.0)
        phi64[a:b] = -t64.sum(axis=1)
        sabs[a:b] = np.abs(t64).sum(axis=1)
    return phi32, phi64, sabs


def host_minpos(phi, off, skip=()):
    """the smallest e of each group with the lowest phi; NONE for an empty or
    skipped group"""
    out = np.full(len(off) - 1, NONE, np.uint32)
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        if b > a and g not in skip:
            out[g] = a + int(np.argmin(phi[a:b]))
    return out


def assert_within(phi, phi64, sabs, what):
    err = np.abs(phi.astype(np.float64) - phi64)
    bound = 17 * U24 * sabs
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0), initial=0))
    print(f"{what}: worst fraction of the rounding bound {worst:.3f}")
    assert np.all(err <= bound), what


def csr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def cube(n, seed):
    return (np.random.default_rng(seed).random((n, 3)) - 0.5).astype(np.float32)


def masses(n, seed):
    return (0.5 + np.random.default_rng(seed).random(n)).astype(np.float32)


# ---------------------------------------------------------------- 1. tile edges
SIZES1 = [1, 2, 63, 64, 65, 0, 255, 256, 257, 513, 0, 1025]


@functools.lru_cache(maxsize=None)
def case1():
    n = 3000
    pts, mass = cube(n, 701), masses(n, 702)
    off = csr(SIZES1)
    mem = np.random.default_rng(703).permutation(n)[:int(off[-1])].astype(np.uint32)
    for a in (pts, mass, off, mem):
        a.setflags(write=False)
    return pts, mass, off, mem


@functools.lru_cache(maxsize=None)
def ref1(eps):
    pts, mass, off, mem = case1()
    return oracle(pts, mass, off, mem, eps)


@pytest.mark.parametrize("eps", [0.0, 0.05])
def test_tile_edges(gpu, eps):
    pts, mass, off, mem = case1()
    t = gpu.Tree(pts, leafsize=16)
    phi, minpos = t.group_potential(off, mem, mass, eps=eps)
    p32, p64, sabs = ref1(eps)
    assert np.array_equal(phi, p32)
    assert_within(phi, p64, sabs, f"tile edges eps {eps}")
    assert np.array_equal(minpos, host_minpos(phi, off))
    assert minpos[5] == NONE and minpos[10] == NONE
    # either output alone is the same output
    assert np.array_equal(t.group_potential(off, mem, mass, eps=eps, minpos=False)[0], phi)
    assert np.array_equal(t.group_potential(off, mem, mass, eps=eps, phi=False)[1], minpos)


# ---------------------------------------------------------------- 2. many small groups
def test_many_small_groups(gpu):
    n = 4000
    pts = cube(n, 711)
    off = csr([20] * 200)
    mem = np.random.default_rng(712).permutation(n).astype(np.uint32)
    t = gpu.Tree(pts, leafsize=64)
    phi, minpos = t.group_potential(off, mem, None, eps=0.01)
    p32, p64, sabs = oracle(pts, None, off, mem, 0.01)
    assert np.array_equal(phi, p32)
    assert_within(phi, p64, sabs, "small groups")
    assert np.array_equal(minpos, host_minpos(phi, off))
    ones = t.group_potential(off, mem, np.ones(n, np.float32), eps=0.01)
    assert np.array_equal(ones[0], phi) and np.array_equal(ones[1], minpos)


# ---------------------------------------------------------------- 3. one large group
def test_one_group_of_3000(gpu):
    n = 3000
    pts, mass = cube(n, 721), masses(n, 722)
    off = csr([n])
    mem = np.random.default_rng(723).permutation(n).astype(np.uint32)
    t = gpu.Tree(pts, leafsize=64)
    phi, minpos = t.group_potential(off, mem, mass, eps=0.0)
    p32, p64, sabs = oracle(pts, mass, off, mem, 0.0)
    assert np.array_equal(phi, p32)
    assert_within(phi, p64, sabs, "one group of 3000")
    assert np.array_equal(minpos, host_minpos(phi, off))


# ---------------------------------------------------------------- 4. periodic
def test_periodic_minimum_image(gpu):
    """Clumps across a corner and a face of the box (L = 1) on the dyadic grid
    2^-10: every difference and image is exact, so shifting the box by 1/2
    changes no d and no bit of phi."""
    rng = np.random.default_rng(731)
    k = rng.integers(-50, 51, (400, 3))
    centre = np.where(np.arange(400)[:, None] < 200, [0, 0, 0], [0, 512, 512])
    grid = (centre + k) % 1024  # rows 0..199 round the corner, 200..399 across the face x = 0
    fill = rng.integers(0, 1024, (600, 3))
    pts = (np.concatenate([grid, fill]) / 1024.0).astype(np.float32)
    assert np.any(pts[:200] > 0.9) and np.any(pts[:200] < 0.1)
    mass = masses(1000, 732)
    off = csr([200, 200, 150])
    mem = np.concatenate([rng.permutation(200), 200 + rng.permutation(200),
                          400 + rng.permutation(600)[:150]]).astype(np.uint32)
    t = gpu.Tree(pts, leafsize=16, boxsize=1.0)
    phi, minpos = t.group_potential(off, mem, mass, eps=0.002)
    p32, p64, sabs = oracle(pts, mass, off, mem, 0.002, L=1.0)
    assert np.array_equal(phi, p32)
    assert_within(phi, p64, sabs, "periodic")
    assert np.array_equal(minpos, host_minpos(phi, off))
    # the wrapped sum is not the plain one: the straddling clumps need the images
    plain = oracle(pts, mass, off, mem, 0.002)[0]
    assert not np.array_equal(plain[:400], phi[:400])
    moved = ((np.concatenate([grid, fill]) + 512) % 1024 / 1024.0).astype(np.float32)
    t2 = gpu.Tree(moved, leafsize=16, boxsize=1.0)
    phi2, minpos2 = t2.group_potential(off, mem, mass, eps=0.002)
    assert np.array_equal(phi2, phi) and np.array_equal(minpos2, minpos)
    # in the middle of the box no image is needed
    assert np.array_equal(oracle(moved, mass, off[:2], mem[:200], 0.002)[0], phi[:200])


# ---------------------------------------------------------------- 5. degenerate
def test_degenerate(gpu):
    n = 17  # one padded leaf
    pts, mass = cube(n, 741), masses(n, 742)
    pts[5] = pts[4]                     # two coincident points
    pts[7:11] = pts[7]                  # a group of coincident points
    mass[[12, 14, 15]] = 0.0            # a zero-mass subset
    groups = [[0, 1, 2, 1, 3],          # a repeated row
              [4, 5, 6],
              [7, 8, 9, 10],
              [11, 12, 13, 14, 15, 16],
              [12, 14, 15]]             # only massless members
    off = csr([len(g) for g in groups])
    mem = np.concatenate(groups).astype(np.uint32)
    t = gpu.Tree(pts, leafsize=16)
    for eps in (0.0, 0.05):
        phi, minpos = t.group_potential(off, mem, mass, eps=eps)
        p32, p64, sabs = oracle(pts, mass, off, mem, eps)
        assert np.array_equal(phi, p32), eps
        assert_within(phi, p64, sabs, f"degenerate eps {eps}")
        assert np.array_equal(minpos, host_minpos(phi, off))
        assert phi[1] == phi[3]                         # the repeated row adds nothing to itself
        assert np.all(phi[8:12] == 0) and minpos[2] == 8    # all coincident
        assert np.all(phi[18:21] == 0) and minpos[4] == 18  # no mass at all
        # the coincident pair sees only the third member, whatever the softening
        d = pts[6] - pts[4]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        want = -(mass[6] * (np.float32(1) / np.sqrt(d2 + np.float32(eps) * np.float32(eps))))
        assert phi[5] == want and phi[6] == want


def test_wide_dynamic_range(gpu):
    """Separations from 2^-60 to 2^60 in one group: squared distances on both
    sides of 2^-96, where the sum kernel changes between its short and its plain
    form of 1 / sqrt (both correctly rounded: == the oracle), all normal."""
    rng = np.random.default_rng(745)
    u = rng.normal(0.0, 1.0, (121, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pts = (u * 2.0 ** np.arange(-60, 61)[:, None]).astype(np.float32)
    mass = masses(121, 746)
    off = csr([121])
    mem = rng.permutation(121).astype(np.uint32)
    t = gpu.Tree(pts, leafsize=16)
    for eps in (0.0, 2.0 ** -50):
        phi, minpos = t.group_potential(off, mem, mass, eps=eps)
        p32, p64, sabs = oracle(pts, mass, off, mem, eps)
        assert np.all(np.isfinite(p32)) and np.all(p32 < 0)
        assert np.array_equal(phi, p32), eps
        assert_within(phi, p64, sabs, f"wide range eps {eps}")
        assert np.array_equal(minpos, host_minpos(phi, off))


# ---------------------------------------------------------------- 6. max_members
def test_max_members(gpu):
    pts, mass, off, mem = case1()
    t = gpu.Tree(pts, leafsize=16)
    phi, minpos = t.group_potential(off, mem, mass, eps=0.05, max_members=64)
    p32 = ref1(0.05)[0]
    skipped = [g for g, s in enumerate(SIZES1) if s > 64]
    assert skipped == [4, 6, 7, 8, 9, 11]
    big = np.zeros(len(mem), bool)
    for g in skipped:
        big[int(off[g]):int(off[g + 1])] = True
    assert np.all(np.isnan(phi[big]))
    assert np.array_equal(phi[~big], p32[~big])
    assert np.array_equal(minpos, host_minpos(p32, off, skip=skipped))


# ---------------------------------------------------------------- 7. validation
def test_invalid_lists_are_counted_and_nothing_is_written(gpu):
    n = 500
    t = gpu.Tree(cube(n, 751), leafsize=16)
    good_off = np.array([0, 5, 8], np.uint64)
    good_mem = np.arange(8, dtype=np.uint32)
    bad_mem = good_mem.copy()
    bad_mem[3] = n
    cases = [(good_off, bad_mem, 2, b"1 violations"),
             (np.array([0, 5, 3, 8], np.uint64), good_mem, 3, b"1 violations"),
             (np.array([1, 5, 8], np.uint64), good_mem, 2, b"1 violations"),
             (np.array([0, 5, 7], np.uint64), good_mem, 2, b"1 violations")]
    for off, mem, G, word in cases:
        phi = np.full(8 + 16, 77.0, np.float32)
        minpos = np.full(G + 16, 77, np.uint32)
        st = gpu.lib().nbkd_group_potential(t.h, off.ctypes.data, mem.ctypes.data, G, 8, None,
                                            ctypes.c_float(0.0), 0, phi.ctypes.data + 32,
                                            minpos.ctypes.data + 32, 0, None)
        msg = gpu.lib().nbkd_last_error()
        assert st == gpu.NBKD_EINVAL and word in msg, (off, msg)
        assert np.all(phi == 77.0) and np.all(minpos == 77)
    with pytest.raises(gpu.NbkdError) as e:
        t.group_potential(good_off, bad_mem)
    assert e.value.status == gpu.NBKD_EINVAL
    phi, minpos = t.group_potential(good_off, good_mem)
    assert np.all(phi < 0) and np.all(minpos != NONE)


# ---------------------------------------------------------------- 8. determinism
def test_determinism(gpu):
    from nbodyhpc_amd import hip
    pts, mass, off, mem = case1()
    G, K, guard = len(off) - 1, len(mem), 64
    t = gpu.Tree(pts, leafsize=16)
    phi, minpos = t.group_potential(off, mem, mass, eps=0.05)
    again = t.group_potential(off, mem, mass, eps=0.05)
    assert np.array_equal(again[0], phi) and np.array_equal(again[1], minpos)
    for leaf in (64, 128):
        other = gpu.Tree(pts, leafsize=leaf).group_potential(off, mem, mass, eps=0.05)
        assert np.array_equal(other[0], phi) and np.array_equal(other[1], minpos), leaf
    # device buffers on a caller's stream, guard words round each output
    doff, dmem = hip.DeviceArray.from_numpy(off), hip.DeviceArray.from_numpy(mem)
    dmass = hip.DeviceArray.from_numpy(mass)
    s = hip.Stream()

    def run(want_phi, want_minpos):
        dphi = hip.DeviceArray.from_numpy(np.full(guard + K + guard, -7.0, np.float32))
        dmin = hip.DeviceArray.from_numpy(np.full(guard + G + guard, 7, np.uint32))
        t.group_potential_device(doff.ptr, dmem.ptr, G, K, dmass.ptr, 0.05, 0,
                                 dphi.ptr + 4 * guard if want_phi else None,
                                 dmin.ptr + 4 * guard if want_minpos else None, stream=s.handle)
        s.synchronize()
        hp, hm = dphi.numpy(), dmin.numpy()
        assert np.all(hp[:guard] == -7.0) and np.all(hp[guard + K:] == -7.0)
        assert np.all(hm[:guard] == 7) and np.all(hm[guard + G:] == 7)
        return hp[guard:guard + K], hm[guard:guard + G]

    dp, dm = run(True, True)
    assert np.array_equal(dp, phi) and np.array_equal(dm, minpos)
    dp, untouched = run(True, False)
    assert np.array_equal(dp, phi) and np.all(untouched == 7)
    untouched, dm = run(False, True)
    assert np.array_equal(dm, minpos) and np.all(untouched == -7.0)
    # replaced ids: members and masses are still input rows
    t.set_ids((np.random.default_rng(761).permutation(len(pts)) + 1_000_000).astype(np.uint32))
    after = t.group_potential(off, mem, mass, eps=0.05)
    assert np.array_equal(after[0], phi) and np.array_equal(after[1], minpos)


# ---------------------------------------------------------------- 9. Python surface
THETA9, THETA9_ERROR = 0.6, 1.2e-2  # DESIGN.md, gravity tests: worst relative potential error


def test_python_surface(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    rng = np.random.default_rng(771)
    n, nclump = 6000, 8
    centres = rng.random((nclump, 3))
    centres[0] = [0.997, 0.5, 0.004]  # across two faces of the box
    clump = centres[rng.integers(0, nclump, 3500)] + rng.normal(0.0, 0.008, (3500, 3))
    small = np.repeat(rng.random((6, 3)), 50, axis=0) + rng.normal(0.0, 0.004, (300, 3))
    pts = (np.concatenate([clump, small, rng.random((2200, 3))]) % 1.0).astype(np.float32)
    pts[pts >= 1.0] = 0.0
    mass = masses(n, 772)
    eps, G = 0.005, 4.30091e-6
    t = KDTree(pts, leafsize=32, boxsize=1.0)
    cat = t.fof_catalog(0.2 * n ** (-1.0 / 3.0), min_members=20, members=True)
    off, mem = cat["offsets"], cat["members"]
    size = np.diff(off.astype(np.int64))
    assert size.max() > 300 and not cat["spans_box"].any()
    phi, most = t.group_potential(off, mem, mass, softening=eps, G=G)
    assert phi.dtype == np.float64 and phi.shape == mem.shape
    assert most.dtype == np.int64 and most.shape == size.shape
    p32, p64, sabs = oracle(pts, mass, off, mem, eps, L=1.0)
    assert np.array_equal(phi, G * p32.astype(np.float64))
    assert_within(p32, p64, sabs, "KDTree.group_potential")
    assert np.array_equal(most, mem[host_minpos(p32, off)].astype(np.int64))
    # groups above max_direct: a temporary non-periodic tree of the unwrapped group
    large = size > 100
    assert large.any() and not large.all()
    in_large = np.repeat(large, size)
    approx, most_a = t.group_potential(off, mem, mass, softening=eps, G=G, max_direct=100,
                                       theta=THETA9)
    exact, most_e = t.group_potential(off, mem, mass, softening=eps, G=G, max_direct=100,
                                      theta=0.0)
    assert np.array_equal(approx[~in_large], phi[~in_large])
    assert np.array_equal(most_a[~large], most[~large])
    rel = np.abs(approx - exact)[in_large] / np.abs(exact[in_large])
    print(f"theta {THETA9}: worst relative difference from theta 0 on the temporary tree "
          f"{rel.max():.3e}")
    assert rel.max() <= THETA9_ERROR
    for g in np.flatnonzero(large):
        a, b = int(off[g]), int(off[g + 1])
        assert most_a[g] == mem[a + int(np.argmin(approx[a:b]))]
        assert most_e[g] == mem[a + int(np.argmin(exact[a:b]))]
    # theta 0 on the temporary tree is the same sum in float32: (T + 16) 2^-24
    # for T <= 1000 sequential terms (6.1e-5), and the unwrapped offsets are
    # rounded once more, 2^-24 against r >= eps = 0.005 (1.2e-5 per term)
    assert np.allclose(exact[in_large], phi[in_large], rtol=1e-4, atol=0)
    # an empty group: -1
    off2 = np.concatenate([off[:1], off]).astype(np.uint64)
    most2 = t.group_potential(off2, mem, mass, softening=eps, G=G)[1]
    assert most2[0] == -1 and np.array_equal(most2[1:], most)


# ---------------------------------------------------------------- 10. unbind
def unbind_ref(pts, vel, off, mem, eps, min_members, max_iter=20):
    """KDTree.unbind with unit masses, G = 1 and the == oracle for phi"""
    off, mem = off.astype(np.int64), mem.copy()
    G = len(off) - 1
    it = 0
    while True:
        phi = oracle(pts, None, off, mem, eps)[0].astype(np.float64)
        energy = np.zeros(len(mem))
        for g in range(G):
            a, b = off[g], off[g + 1]
            if b > a:
                v = vel[mem[a:b]].astype(np.float64)
                dv = v - v.mean(axis=0)
                energy[a:b] = 0.5 * (dv * dv).sum(axis=1) + phi[a:b]
        if it >= max_iter:
            break
        it += 1
        keep = ~(energy >= 0)
        for g in range(G):
            if keep[off[g]:off[g + 1]].sum() < min_members:
                keep[off[g]:off[g + 1]] = False
        if keep.all():
            break
        cnt = np.array([keep[off[g]:off[g + 1]].sum() for g in range(G)])
        mem, off = mem[keep], np.concatenate([[0], np.cumsum(cnt)])
    return off, mem, energy, it


def test_unbind(gpu):
    from nbodyhpc_amd.kdtree import KDTree
    rng = np.random.default_rng(781)
    clump = rng.normal(0.0, 0.05, (40, 3))
    inter = rng.normal(0.0, 0.03, (6, 3))       # interlopers inside the clump
    fast = rng.normal(0.0, 0.05, (3, 3)) + 5.0  # a small group elsewhere
    rest = rng.random((51, 3)) * 10.0 - 20.0
    pts = np.concatenate([clump, inter, fast, rest]).astype(np.float32)
    n, eps = len(pts), 0.01
    off = csr([46, 3])
    mem = np.concatenate([rng.permutation(46), [46, 47, 48]]).astype(np.uint32)
    t = KDTree(pts, leafsize=16)
    phi0 = t.group_potential(off, mem, softening=eps)[0]
    vesc = float(np.sqrt(2.0 * np.abs(phi0[:46]).max()))  # the clump's largest escape speed
    vel = rng.normal(0.0, 0.01 * vesc, (n, 3))            # cold
    u = rng.normal(0.0, 1.0, (3, 3))
    u *= 10.0 * vesc / np.linalg.norm(u, axis=1)[:, None]
    vel[40:46] = np.concatenate([u, -u])                  # 10 x the escape speed, no net momentum
    vel[46:49] = 3.0 * np.sqrt(2.0 * np.abs(phi0[46:]).max()) * np.eye(3)
    res = t.unbind(off, mem, vel, softening=eps, min_members=5)
    r_off, r_mem, r_energy, r_it = unbind_ref(pts, vel, off, mem, eps, 5)
    assert res["iterations"] == r_it and res["iterations"] >= 2
    assert np.array_equal(res["offsets"], r_off.astype(np.uint64))
    assert np.array_equal(res["members"], r_mem)
    # the interlopers went in iteration 1, the clump stayed, the trio was emptied
    assert np.array_equal(res["members"], mem[:46][mem[:46] < 40])
    assert np.array_equal(res["offsets"], np.array([0, 40, 40], np.uint64))
    assert res["iterations"] == 2
    assert np.array_equal(res["most_bound"][1:], [-1]) and 0 <= res["most_bound"][0] < 40
    assert res["phi"].shape == (40,) and np.all(res["energy"] < 0)
    assert np.allclose(res["energy"], r_energy, rtol=1e-12, atol=0)
    # no energy sits on a rounding edge: |E| is far above the rounding of phi
    assert np.abs(r_energy).min() > 1e-3 * np.abs(res["phi"]).max()
    one = t.unbind(off, mem, vel, softening=eps, min_members=5, max_iter=1)
    assert one["iterations"] == 1 and np.array_equal(one["members"], res["members"])
    assert np.array_equal(one["phi"], res["phi"])
