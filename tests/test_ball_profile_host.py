"""CPU tests of the radial-profile boundary (nbkd_query_ball_profile): the
symbol is declared, bound and exported, every argument check runs before any
device call and leaves the output alone, the two type stubs agree, the Python
wrappers (profile / so_mass) reject bad arguments without a device, and
so_mass's bracket and interpolation logic is right with profile replaced by a
numpy brute force."""
import ctypes
import math
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOL = 4.0 / 3.0 * math.pi


def test_symbol_declared_bound_and_exported():
    assert "nbkd_query_ball_profile" in capi.header_symbols()
    assert "nbkd_query_ball_profile" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_query_ball_profile")
    assert capi.NBKD_MAX_RADII == 32
    txt = open(capi.HEADER).read()
    assert "#define NBKD_MAX_RADII 32" in txt
    assert "per-bin, not cumulative" in txt


class Args:
    """A well-formed call on a stand-in tree handle.  The argument checks (and
    m == 0) return before the handle is looked at, so no device is needed; the
    output holds a sentinel."""

    def __init__(self):
        self.tree = ctypes.create_string_buffer(1 << 16)
        self.q = np.zeros((4, 3), np.float32)
        self.scale = np.ones(4, np.float32)
        self.radii = np.array([0.1, 0.2, 0.2, 0.4], np.float32)
        self.v = np.ones((8, 4), np.float32)
        self.s = np.full((4, 4, 4), 77.0, np.float32)

    def call(self, **kw):
        a = dict(tree=ctypes.addressof(self.tree), q=self.q.ctypes.data, m=4,
                 scale=self.scale.ctypes.data, radii=self.radii, nr=None,
                 values=self.v.ctypes.data, nv=4, out_sum=self.s.ctypes.data)
        a.update(kw)
        r = a["radii"]
        if r is not None:
            r = np.ascontiguousarray(r, np.float32)
        nr = a["nr"] if a["nr"] is not None else (0 if r is None else len(r))
        L = capi.lib()
        st = L.nbkd_query_ball_profile(a["tree"], a["q"], a["m"], a["scale"],
                                       None if r is None else r.ctypes.data, nr, a["values"],
                                       a["nv"], a["out_sum"], 0, None)
        return st, L.nbkd_last_error()

    def untouched(self):
        return bool(np.all(self.s == 77.0))


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"NULL"),
    (dict(q=None), b"NULL"),
    (dict(radii=None, nr=4), b"NULL"),
    (dict(out_sum=None), b"NULL"),
    (dict(nr=0), b"number of radii"),
    (dict(nr=-1), b"number of radii"),
    (dict(radii=np.linspace(0.1, 1, 33)), b"number of radii"),
    (dict(nv=0), b"channels"),
    (dict(nv=5), b"channels"),
    (dict(nv=-1), b"channels"),
    (dict(values=None, nv=2), b"nv == 1"),
    (dict(radii=[0.1, 0.3, 0.2]), b"ascending"),
    (dict(radii=[0.1, float("nan")]), b"NaN, infinite or negative"),
    (dict(radii=[0.1, float("inf")]), b"NaN, infinite or negative"),
    (dict(radii=[-0.5, 0.1]), b"NaN, infinite or negative"),
    (dict(m=1 << 32), b"2^32"),
])
def test_invalid_arguments_rejected_before_any_device_call(kw, word):
    a = Args()
    st, msg = a.call(**kw)
    assert st == capi.NBKD_EINVAL
    assert word in msg, msg
    assert msg.startswith(b"nbkd_query_ball_profile") or b"2^32" in msg
    assert a.untouched()


def test_no_queries_is_ok():
    a = Args()
    st, _ = a.call(m=0)
    assert st == capi.NBKD_OK
    assert a.untouched()
    # scale and values are optional
    st, _ = a.call(m=0, scale=None, values=None, nv=1)
    assert st == capi.NBKD_OK


def test_type_stubs_declare_ball_profile_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def ball_profile(" in a
    assert a == b


def wrapper(n=10):
    """A KDTree whose native part was never constructed: the wrappers check
    their arguments before they reach it."""
    from nbodyhpc_amd.kdtree import KDTree
    t = KDTree.__new__(KDTree)
    t._n_input = n
    return t


Q = np.zeros((3, 3), np.float32)


def test_profile_rejects_bad_radii():
    t = wrapper()
    for radii, word in (([[0.1, 0.2]], "1-D"), ([], "empty"), (np.linspace(0.1, 1, 33), "at most"),
                        ([0.1, float("nan")], "finite"), ([0.1, float("inf")], "finite"),
                        ([-0.1, 0.1], "finite"), ([0.2, 0.1], "ascending")):
        with pytest.raises(ValueError, match=word):
            t.profile(Q, radii)


def test_profile_rejects_bad_scale_and_values():
    t = wrapper()
    r = [0.1, 0.2]
    for scale in (-1.0, float("nan"), float("inf"), [1.0, -1.0, 1.0]):
        with pytest.raises(ValueError, match="finite"):
            t.profile(Q, r, scale=scale)
    with pytest.raises(ValueError, match="broadcast"):
        t.profile(Q, r, scale=[1.0, 2.0])
    with pytest.raises(ValueError, match="values"):
        t.profile(Q, r, values=np.zeros(9))
    with pytest.raises(ValueError, match="values"):
        t.profile(Q, r, values=np.zeros((11, 2)))
    with pytest.raises(ValueError, match="values"):
        t.profile(Q, r, values=np.zeros((10, 2, 2)))
    with pytest.raises(ValueError, match="channels"):
        t.profile(Q, r, values=np.zeros((10, 5)))


def test_so_mass_rejects_bad_arguments():
    t = wrapper()
    with pytest.raises(ValueError, match="nbins"):
        t.so_mass(Q, 1.0, 0.1, nbins=1)
    with pytest.raises(ValueError, match="nbins"):
        t.so_mass(Q, 1.0, 0.1, nbins=33)
    with pytest.raises(ValueError, match="refine"):
        t.so_mass(Q, 1.0, 0.1, refine=-1)
    for r_max, r_min in ((0.0, None), (-1.0, None), (float("nan"), None), (float("inf"), None),
                         (0.1, 0.0), (0.1, 0.1), (0.1, 0.2), (0.1, float("nan"))):
        with pytest.raises(ValueError, match="r_min and r_max"):
            t.so_mass(Q, 1.0, r_max, r_min=r_min)
    for od in (0.0, -1.0, float("nan"), float("inf"), [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match="overdensity"):
            t.so_mass(Q, od, 0.1)
    with pytest.raises(ValueError, match="broadcast"):
        t.so_mass(Q, [1.0, 2.0], 0.1)
    with pytest.raises(ValueError, match="centres"):
        t.so_mass(np.zeros((3, 2)), 1.0, 0.1)
    with pytest.raises(ValueError, match="mass"):
        t.so_mass(Q, 1.0, 0.1, mass=np.ones(9))
    with pytest.raises(ValueError, match="mass"):
        t.so_mass(Q, 1.0, 0.1, mass=np.ones((10, 1)))


# ---------------------------------------------------------------- so_mass logic
class Brute:
    """profile() by numpy brute force in the plain metric: thresholds in
    float32 as nbkd.h defines them, d2 in float32, the running sum in float64.
    Records each call's (radii, scale)."""

    def __init__(self, pts, mass=None):
        self.pts = np.asarray(pts, np.float32)
        self.mass = np.ones(len(pts)) if mass is None else np.asarray(mass, np.float64)
        self.calls = []

    def __call__(self, points, radii, values=None, scale=None, cumulative=False):
        assert cumulative
        q = np.asarray(points, np.float32)
        r = np.asarray(radii, np.float32)
        s = np.ones(len(q), np.float32) if scale is None else np.asarray(scale, np.float32)
        self.calls.append((r.copy(), None if scale is None else s.copy()))
        e = r[None, :] * s[:, None]
        t = np.minimum(e * e, np.finfo(np.float32).max)
        d = self.pts[None, :, :] - q[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        w = self.mass if values is None else np.asarray(values, np.float64)
        return ((d2[:, :, None] <= t[:, None, :]) * w[None, :, None]).sum(axis=1)

    def enclosed(self, centre, r):
        """M(d2 <= fl(r * r)) around one centre, r a float32"""
        d = self.pts - np.asarray(centre, np.float32)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return float(self.mass[d2 <= np.float32(r) * np.float32(r)].sum())


RMIN = 0.015  # beyond the innermost member: the density at r_min is far above the threshold


def shells(centre, radii, seed):
    """one point at each of the given distances from the centre, random directions"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(len(radii), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.asarray(centre) + d * np.asarray(radii)[:, None]


def so_tree(pts, monkeypatch, mass=None):
    t = wrapper(len(pts))
    b = Brute(pts, mass)
    monkeypatch.setattr(t, "profile", b, raising=False)
    return t, b


def test_so_mass_brackets_and_interpolates(monkeypatch):
    """Members at n * 0.01 (n = 1..60): M(<= r) = floor(r / 0.01), the mean
    density falls like n^-2, one crossing.  Three centres: a clump (status 0), an
    empty place (status 1: nothing within r_min, density 0), a dense clump that
    never falls below the threshold within r_max (status 2)."""
    c0, c1, c2 = [0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [20.0, 0.0, 0.0]
    pts = np.concatenate([shells(c0, 0.01 * np.arange(1, 61), 1),
                          shells(c2, 0.001 * np.arange(1, 401), 2)])
    t, b = so_tree(pts, monkeypatch)
    # the density at n = 20: 20 / (VOL 0.2^3); the threshold sits between n = 20 and 21
    delta = 19.5 / (VOL * 0.2 ** 3)
    res = t.so_mass(np.array([c0, c1, c2]), delta, 0.5, r_min=RMIN, nbins=32, refine=2)
    assert list(res["status"]) == [0, 1, 2]
    assert res["status"].dtype == np.int32
    assert res["r_lo"].dtype == np.float32 and res["m_lo"].dtype == np.float64
    for name in ("radius", "mass", "r_lo", "r_hi", "m_lo", "m_hi"):
        assert np.all(np.isnan(res[name][1:])), name
    r_lo, r_hi = res["r_lo"][0], res["r_hi"][0]
    assert res["m_lo"][0] == b.enclosed(c0, r_lo) and res["m_hi"][0] == b.enclosed(c0, r_hi)
    assert res["m_lo"][0] / (VOL * float(r_lo) ** 3) >= delta
    assert res["m_hi"][0] / (VOL * float(r_hi) ** 3) < delta
    # three passes: the shared grid, then two in units of the bracket's lower edge
    assert len(b.calls) == 3
    assert b.calls[0][1] is None and len(b.calls[0][0]) == 32
    ratio = (0.5 / RMIN) ** (1 / 31)
    for radii, scale in b.calls[1:]:
        assert radii[0] == 1.0 and len(scale) == 1  # only the centre with a bracket
        assert abs(radii[-1] / (ratio * (1 + 2.0 ** -20)) - 1) < 2.0 ** -22
        ratio = float(radii[-1]) ** (1 / 31)
    assert r_hi / r_lo <= ratio * (1 + 2.0 ** -20)
    assert r_lo <= res["radius"][0] <= r_hi
    # log-log interpolation inside the bracket
    rho_lo = res["m_lo"][0] / (VOL * float(r_lo) ** 3)
    rho_hi = res["m_hi"][0] / (VOL * float(r_hi) ** 3)
    f = math.log(rho_lo / delta) / math.log(rho_lo / rho_hi)
    assert res["radius"][0] == pytest.approx(float(r_lo) * (float(r_hi) / float(r_lo)) ** f,
                                             rel=1e-14)
    assert res["mass"][0] == pytest.approx(delta * VOL * res["radius"][0] ** 3, rel=1e-14)
    # the step profile dips below the threshold inside the shell of 19 members
    # (r > 0.19827) and for good inside that of 20 (r > 0.2017); within a shell
    # the density is a power law, which the log-log interpolation follows exactly
    assert res["m_lo"][0] == res["m_hi"][0] and res["m_lo"][0] in (19.0, 20.0)
    assert res["radius"][0] == pytest.approx((res["m_lo"][0] / (VOL * delta)) ** (1 / 3), rel=1e-12)


def test_so_mass_refine_zero_and_masses(monkeypatch):
    pts = shells([0.0, 0.0, 0.0], 0.01 * np.arange(1, 61), 3)
    mass = np.full(60, 2.5)
    t, b = so_tree(pts, monkeypatch, mass)
    delta = 2.5 * 19.5 / (VOL * 0.2 ** 3)
    res = t.so_mass(np.zeros((1, 3)), delta, 0.5, mass=mass, r_min=RMIN, nbins=16, refine=0)
    assert len(b.calls) == 1 and res["status"][0] == 0
    grid = b.calls[0][0]
    k = int(np.searchsorted(grid, res["r_hi"][0]))
    assert grid[k] == res["r_hi"][0] and grid[k - 1] == res["r_lo"][0]
    assert res["m_hi"][0] == b.enclosed([0, 0, 0], grid[k]) and res["m_hi"][0] % 2.5 == 0
    # N-D centres: the dict's arrays take their shape
    res2 = t.so_mass(np.zeros((2, 1, 3)), delta, 0.5, mass=mass, r_min=RMIN, nbins=16, refine=0)
    assert res2["radius"].shape == (2, 1) and np.all(res2["radius"] == res["radius"][0])


def test_so_mass_failed_refinement_keeps_the_bracket(monkeypatch):
    """A refinement pass that does not bracket a crossing leaves the earlier
    bracket: once with every refined edge at or above the threshold (no k*),
    once with the density below it already at the bracket's lower edge
    (k* == 0)."""
    pts = shells([0.0, 0.0, 0.0], 0.01 * np.arange(1, 61), 4)
    t, b = so_tree(pts, monkeypatch)
    delta = 19.5 / (VOL * 0.2 ** 3)
    coarse = t.so_mass(np.zeros((1, 3)), delta, 0.5, r_min=RMIN, nbins=32, refine=0)
    assert coarse["status"][0] == 0
    # the refinement's profile reports an enclosed mass that stays above the
    # threshold at every refined edge
    first = Brute(pts)

    def stubborn(points, radii, values=None, scale=None, cumulative=False):
        if scale is None:
            return first(points, radii, values, scale, cumulative)
        return np.full((len(points), len(radii)), 1e9)

    monkeypatch.setattr(t, "profile", stubborn, raising=False)
    res = t.so_mass(np.zeros((1, 3)), delta, 0.5, r_min=RMIN, nbins=32, refine=1)
    for name in ("status", "r_lo", "r_hi", "m_lo", "m_hi", "radius", "mass"):
        assert res[name][0] == coarse[name][0], name
    # and one below the threshold already at the bracket's lower edge
    def empty(points, radii, values=None, scale=None, cumulative=False):
        if scale is None:
            return first(points, radii, values, scale, cumulative)
        return np.zeros((len(points), len(radii)))

    monkeypatch.setattr(t, "profile", empty, raising=False)
    res = t.so_mass(np.zeros((1, 3)), delta, 0.5, r_min=RMIN, nbins=32, refine=1)
    for name in ("status", "r_lo", "r_hi", "m_lo", "m_hi", "radius", "mass"):
        assert res[name][0] == coarse[name][0], name
