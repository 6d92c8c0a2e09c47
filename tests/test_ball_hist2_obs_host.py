"""CPU tests of the observer-frame pair counts (nbkd_query_ball_hist2_obs): the
symbol is declared, bound and exported, every argument check runs before any
device call and leaves the output alone, m == 0 zeroes the output, the two type
stubs agree, the Python wrappers reject bad arguments without a device,
landy_szalay / xi_rppi_ls / xi_smu_ls are the formulas of their docstrings when
fed synthetic counts, and the float32 reference the GPU tests compare with
agrees with the float64 geometry up to the pairs that lie on an edge."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi
from tests import aniso_obs_ref as ob
from tests.aniso_ref import RPPI, SMU
from tests.golden.inputs import uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.uint64(77)
FN = "nbkd_query_ball_hist2_obs"


def test_symbol_declared_bound_and_exported():
    assert FN in capi.header_symbols()
    assert FN in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), FN)
    assert hasattr(capi.Tree, "ball_hist2_obs") and hasattr(capi.Tree, "ball_hist2_obs_device")
    txt = open(capi.HEADER).read()
    for words in ("l2 > 0 ? fminf(fl(x / l2), s2) : 0", "rp2  = fl(s2 - pi2)",
                  "fall into the same bin", "mirror images about it",
                  "Out of scope: pair weights, per-query rows, jackknife regions, periodic",
                  "the bisector"):
        assert words in txt, words


class Args:
    """A well-formed call on a stand-in tree handle.  The argument checks (and
    m == 0) return before the handle is looked at, so no device is needed; the
    output holds a sentinel."""

    def __init__(self):
        self.tree = ctypes.create_string_buffer(1 << 16)
        self.q = np.zeros((4, 3), np.float32)
        self.out = np.full((32, 64), SENTINEL, np.uint64)

    def call(self, **kw):
        a = dict(tree=ctypes.addressof(self.tree), q=self.q.ctypes.data, m=4, mode=capi.NBKD_HIST2_SMU,
                 obs=[0.5, 0.5, -2.0], e1=[0.1, 0.2, 0.2, 0.4], n1=None,
                 e2=[0.0, 0.5, 0.5, 1.0], n2=None, out=self.out.ctypes.data)
        a.update(kw)
        e1 = None if a["e1"] is None else np.ascontiguousarray(a["e1"], np.float32)
        e2 = None if a["e2"] is None else np.ascontiguousarray(a["e2"], np.float32)
        o = None if a["obs"] is None else np.ascontiguousarray(a["obs"], np.float32)
        n1 = a["n1"] if a["n1"] is not None else len(e1)
        n2 = a["n2"] if a["n2"] is not None else len(e2)
        L = capi.lib()
        st = L.nbkd_query_ball_hist2_obs(a["tree"], a["q"], a["m"], a["mode"],
                                         None if o is None else o.ctypes.data,
                                         None if e1 is None else e1.ctypes.data, n1,
                                         None if e2 is None else e2.ctypes.data, n2, a["out"], 0,
                                         None)
        return st, L.nbkd_last_error()

    def untouched(self):
        return bool(np.all(self.out == SENTINEL))


RP = dict(mode=capi.NBKD_HIST2_RPPI)


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"NULL"),
    (dict(q=None), b"NULL"),
    (dict(obs=None), b"NULL"),
    (dict(e1=None, n1=4), b"NULL"),
    (dict(e2=None, n2=4), b"NULL"),
    (dict(out=None), b"NULL"),
    (dict(mode=2), b"unknown mode 2"),
    (dict(mode=-1), b"unknown mode -1"),
    (dict(obs=[float("nan"), 0, 0]), b"observer component 0 is NaN or infinite"),
    (dict(obs=[0, float("inf"), 0]), b"observer component 1 is NaN or infinite"),
    (dict(obs=[0, 0, float("-inf")]), b"observer component 2 is NaN or infinite"),
    (dict(n1=0), b"number of first-axis edges"),
    (dict(n1=-1), b"number of first-axis edges"),
    (dict(e1=np.linspace(0.1, 1, 33)), b"number of first-axis edges"),
    (dict(n2=0), b"number of second-axis edges"),
    (dict(e2=np.linspace(0.0, 1, 65)), b"got 65"),
    (dict(e2=np.linspace(0.0, 1, 65), **RP), b"got 65"),
    (dict(e1=[0.1, 0.3, 0.2]), b"first-axis edges must be ascending (edge 2"),
    (dict(e2=[0.1, 0.3, 0.2]), b"second-axis edges must be ascending (edge 2"),
    (dict(e1=[0.1, float("nan")]), b"first-axis edge 1 is NaN, infinite or negative"),
    (dict(e1=[0.1, float("inf")]), b"first-axis edge 1 is NaN, infinite or negative"),
    (dict(e1=[-0.5, 0.1]), b"first-axis edge 0 is NaN, infinite or negative"),
    (dict(e2=[float("nan"), 0.1]), b"second-axis edge 0 is NaN, infinite or negative"),
    (dict(e2=[0.1, float("inf")], **RP), b"second-axis edge 1 is NaN, infinite or negative"),
    (dict(e2=[-0.5, 0.1]), b"second-axis edge 0 is NaN, infinite or negative"),
    (dict(e2=[0.5, 1.0, 1.5]), b"second-axis edge 2 is above 1"),
    (dict(e2=[0.5, np.nextafter(np.float32(1), np.float32(2))]), b"edge 1 is above 1"),
    (dict(m=1 << 32), b"2^32"),
])
def test_invalid_arguments_rejected_before_any_device_call(kw, word):
    a = Args()
    st, msg = a.call(**kw)
    assert st == capi.NBKD_EINVAL
    assert word in msg, msg
    assert msg.startswith(b"nbkd_query_ball_hist2_obs:")
    assert a.untouched()


def test_the_fixed_axis_messages_are_unchanged():
    """the shared edge check still names nbkd_query_ball_hist2 for that call"""
    e = np.array([0.3, 0.2], np.float32)
    out = np.zeros(4, np.uint64)
    q = np.zeros((1, 3), np.float32)
    tree = ctypes.create_string_buffer(1 << 16)
    L = capi.lib()
    st = L.nbkd_query_ball_hist2(ctypes.addressof(tree), q.ctypes.data, 1, 0, 2, e.ctypes.data, 2,
                                 e.ctypes.data, 2, out.ctypes.data, 0, None)
    assert st == capi.NBKD_EINVAL
    assert L.nbkd_last_error().startswith(b"nbkd_query_ball_hist2: the first-axis edges")


def test_pi_edges_may_pass_one():
    a = Args()
    st, _ = a.call(m=0, e2=[0.5, 1.0, 1.5], **RP)
    assert st == capi.NBKD_OK


def test_no_queries_zeroes_the_output():
    a = Args()
    st, _ = a.call(m=0)
    assert st == capi.NBKD_OK
    flat = a.out.reshape(-1)
    assert np.all(flat[:16] == 0) and np.all(flat[16:] == SENTINEL)


def test_type_stubs_declare_query_ball_hist2_obs_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def query_ball_hist2_obs(" in a
    assert a == b
    from nbodyhpc_amd.kdtree import cKDTree
    assert hasattr(cKDTree, "query_ball_hist2_obs")


def wrapper(n=10, periodic=False, box=0.0):
    """A KDTree whose native part was never constructed: the wrappers check
    their arguments before they reach it.  (The class attributes stand in for
    the native properties.)"""
    from nbodyhpc_amd.kdtree import KDTree

    class Fake(KDTree):
        pass

    Fake.periodic = periodic
    Fake.boxsize = box
    t = Fake.__new__(Fake)
    t._n_input = n
    return t


Q = np.zeros((3, 3), np.float32)
OK = [0.1, 0.2]


def test_count_methods_reject_a_bad_observer():
    t = wrapper()
    o = (0.5, 0.5, -2.0)
    for fn in (t.count_pairs_rppi, t.count_pairs_smu):
        for los in (0, 1):
            with pytest.raises(ValueError, match="give los or observer, not both"):
                fn(Q, OK, OK, los=los, observer=o)
        for bad in ((0.5, 0.5), (0.5, 0.5, 0.5, 0.5), [[0.5, 0.5, 0.5]], 1.0,
                    (0.5, float("nan"), 0.5), (float("inf"), 0.5, 0.5), (1e39, 0.0, 0.0), "abc"):
            with pytest.raises(ValueError, match="observer must be 3 finite coordinates"):
                fn(Q, OK, OK, observer=bad)
        # the edge checks still come first
        with pytest.raises(ValueError, match="ascending"):
            fn(Q, [0.2, 0.1], OK, observer=o)
    for fn in (t.pair_counts_rppi, t.pair_counts_smu):
        t.points = lambda: Q
        with pytest.raises(ValueError, match="not both"):
            fn(OK, OK, los=0, observer=o)
    p = wrapper(periodic=True, box=1.0)
    for fn in (p.count_pairs_rppi, p.count_pairs_smu):
        with pytest.raises(ValueError, match="non-periodic"):
            fn(Q, OK, OK, observer=o)


def test_ls_methods_reject_bad_arguments():
    t, r = wrapper(), wrapper(20)
    with pytest.raises(ValueError, match="randoms must be a KDTree"):
        t.xi_rppi_ls(None, [0.1, 0.2], 0.1, 4)
    with pytest.raises(ValueError, match="randoms must be a KDTree"):
        t.xi_smu_ls(np.zeros((5, 3)), [0.1, 0.2], 4)
    with pytest.raises(ValueError, match="periodicity"):
        t.xi_rppi_ls(wrapper(periodic=True, box=1.0), [0.1, 0.2], 0.1, 4)
    p = wrapper(periodic=True, box=1.0)
    with pytest.raises(ValueError, match="periodicity and box size"):
        p.xi_smu_ls(wrapper(periodic=True, box=2.0), [0.1, 0.2], 4)
    with pytest.raises(ValueError, match="half the box"):
        p.xi_rppi_ls(wrapper(periodic=True, box=1.0), [0.1, 0.51], 0.1, 4)
    with pytest.raises(ValueError, match="half the box"):
        p.xi_smu_ls(wrapper(periodic=True, box=1.0), [0.1, 0.51], 4)
    with pytest.raises(ValueError, match="two edges"):
        t.xi_rppi_ls(r, [0.1], 0.1, 4)
    with pytest.raises(ValueError, match="strictly"):
        t.xi_smu_ls(r, [0.1, 0.1, 0.2], 4)
    for n2 in (0, 65, 2.5):
        with pytest.raises(ValueError, match="npi"):
            t.xi_rppi_ls(r, [0.1, 0.2], 0.1, n2)
        with pytest.raises(ValueError, match="nmu"):
            t.xi_smu_ls(r, [0.1, 0.2], n2)
    for pi_max in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pi_max"):
            t.xi_rppi_ls(r, [0.1, 0.2], pi_max, 4)
    # no half-box limit without a box
    t.points = r.points = lambda: Q
    with pytest.raises(ValueError, match="not both"):
        t.xi_rppi_ls(r, [0.1, 7.0], 9.0, 4, los=1, observer=(0, 0, 0))


def synthetic(shape, seed):
    return np.random.default_rng(seed).integers(1, 10_000, size=shape).astype(np.uint64)


def test_landy_szalay_is_its_formula():
    from nbodyhpc_amd.kdtree import landy_szalay
    dd, dr, rr = synthetic((4, 5), 1), synthetic((4, 5), 2), synthetic((4, 5), 3)
    rr[1, 2] = 0
    rr[3, 0] = 0
    dd[3, 0] = 0
    nd, nr = 3000, 6011
    xi = landy_szalay(dd, dr, rr, nd, nr)
    assert xi.dtype == np.float64 and xi.shape == (4, 5)
    for i in range(4):
        for l in range(5):
            if rr[i, l] == 0:
                assert math.isnan(xi[i, l])
                continue
            a = float(dd[i, l]) / (nd * (nd - 1))
            b = float(dr[i, l]) / (nd * nr)
            c = float(rr[i, l]) / (nr * (nr - 1))
            assert xi[i, l] == pytest.approx((a - 2 * b + c) / c, rel=1e-12)
    assert np.isnan(xi).sum() == 2
    # randoms that are the data: DD = DR' = RR gives 0
    same = landy_szalay(dd, dd.astype(np.float64) * nd / (nd - 1), dd, nd, nd)
    assert np.allclose(same[dd > 0], 0.0, atol=1e-12)


def fake_trees(monkeypatch, nd, nr, tables):
    """data and random wrappers whose count method returns tables[(tree, queries)]"""
    t, r = wrapper(nd), wrapper(nr)
    seen = []
    monkeypatch.setattr(t, "points", lambda: "data", raising=False)
    monkeypatch.setattr(r, "points", lambda: "randoms", raising=False)
    for tree, name in ((t, "data"), (r, "randoms")):
        def fake(points, e1, e2, los=2, observer=None, name=name):
            seen.append(dict(tree=name, points=points, e1=np.array(e1), e2=np.array(e2), los=los,
                             observer=observer))
            return tables[(name, points)]
        monkeypatch.setattr(tree, "count_pairs_rppi", fake, raising=False)
        monkeypatch.setattr(tree, "count_pairs_smu", fake, raising=False)
    return t, r, seen


def ls_by_hand(dd, dr, rr, nd, nr):
    out = np.full(dd.shape, np.nan)
    for idx in np.ndindex(*dd.shape):
        if rr[idx] != 0:
            c = float(rr[idx]) / (nr * (nr - 1))
            out[idx] = (float(dd[idx]) / (nd * (nd - 1)) - 2 * float(dr[idx]) / (nd * nr) + c) / c
    return out


def test_xi_rppi_ls_is_its_formula(monkeypatch):
    nd, nr, npi, pi_max = 3000, 7001, 7, 1.1
    rp = np.array([0.03, 0.05, 0.1, 0.3, 0.7], np.float32)
    tables = {("data", "data"): synthetic((5, npi), 1), ("randoms", "data"): synthetic((5, npi), 2),
              ("randoms", "randoms"): synthetic((5, npi), 3)}
    tables[("randoms", "randoms")][2, 3] = 0
    t, r, seen = fake_trees(monkeypatch, nd, nr, tables)
    o = (0.5, 0.5, -2.0)
    xi, wp = t.xi_rppi_ls(r, rp, pi_max, npi, observer=o)
    assert [(c["tree"], c["points"]) for c in seen] == [("data", "data"), ("randoms", "data"),
                                                        ("randoms", "randoms")]
    pe = np.array([np.float32(pi_max * (l + 1) / npi) for l in range(npi)], np.float32)
    for c in seen:
        assert c["observer"] == o and c["los"] == 2
        assert c["e1"].dtype == np.float32 and np.array_equal(c["e1"], rp)
        assert c["e2"].dtype == np.float32 and np.array_equal(c["e2"], pe)
    want = ls_by_hand(tables[("data", "data")][1:], tables[("randoms", "data")][1:],
                      tables[("randoms", "randoms")][1:], nd, nr)
    assert xi.shape == (4, npi) and wp.shape == (4,) and xi.dtype == np.float64
    assert math.isnan(xi[1, 3]) and np.isnan(xi).sum() == 1 and math.isnan(wp[1])
    ok = ~np.isnan(want)
    assert np.allclose(xi[ok], want[ok], rtol=1e-12, atol=0)
    p = [0.0] + [float(x) for x in pe]
    for i in (0, 2, 3):
        acc = sum(want[i, l] * (p[l + 1] - p[l]) for l in range(npi))
        assert wp[i] == pytest.approx(2.0 * acc, rel=1e-12)
    # a fixed axis: no observer reaches the count methods
    del seen[:]
    t.xi_rppi_ls(r, rp, pi_max, npi, los=0)
    assert [c["los"] for c in seen] == [0, 0, 0] and all(c["observer"] is None for c in seen)


def test_xi_smu_ls_is_its_formula(monkeypatch):
    nd, nr, nmu = 4000, 9000, 6
    s = np.array([0.5, 1.0, 2.0, 4.5, 9.0, 20.0], np.float32)
    tables = {("data", "data"): synthetic((6, nmu), 4), ("randoms", "data"): synthetic((6, nmu), 5),
              ("randoms", "randoms"): synthetic((6, nmu), 6)}
    tables[("randoms", "randoms")][5, 0] = 0
    t, r, seen = fake_trees(monkeypatch, nd, nr, tables)
    xi, poles = t.xi_smu_ls(r, s, nmu, observer=[1.0, 2.0, 3.0])
    me = np.array([np.float32((l + 1) / nmu) for l in range(nmu)], np.float32)
    assert len(seen) == 3 and all(np.array_equal(c["e2"], me) for c in seen)
    assert all(np.array_equal(c["e1"], s) and c["observer"] == [1.0, 2.0, 3.0] for c in seen)
    want = ls_by_hand(tables[("data", "data")][1:], tables[("randoms", "data")][1:],
                      tables[("randoms", "randoms")][1:], nd, nr)
    assert sorted(poles) == [0, 2, 4] and xi.shape == (5, nmu)
    assert math.isnan(xi[4, 0]) and np.isnan(xi).sum() == 1
    ok = ~np.isnan(want)
    assert np.allclose(xi[ok], want[ok], rtol=1e-12, atol=0)
    u = [0.0] + [float(x) for x in me]
    leg = {0: lambda x: 1.0, 2: lambda x: 0.5 * (3 * x * x - 1),
           4: lambda x: (35 * x ** 4 - 30 * x * x + 3) / 8.0}
    for i in range(4):
        for ell in (0, 2, 4):
            acc = sum(want[i, l] * leg[ell](0.5 * (u[l + 1] + u[l])) * (u[l + 1] - u[l])
                      for l in range(nmu))
            assert poles[ell][i] == pytest.approx((2 * ell + 1) * acc, rel=1e-12, abs=1e-13)
        assert math.isnan(poles[0][4])
    _, only = t.xi_smu_ls(r, s, nmu, ells=(2,), los=1)
    assert list(only) == [2] and np.array_equal(only[2][:4], poles[2][:4])
    assert [c["los"] for c in seen[3:]] == [1, 1, 1]


def test_auto_counts_pass_the_observer_on(monkeypatch):
    t = wrapper(10)
    ordered = np.array([[30, 4], [6, 8]], np.uint64)
    seen = []

    def fake(points, e1, e2, los=2, observer=None):
        seen.append(observer)
        return ordered

    monkeypatch.setattr(t, "points", lambda: None, raising=False)
    monkeypatch.setattr(t, "count_pairs_rppi", fake, raising=False)
    monkeypatch.setattr(t, "count_pairs_smu", fake, raising=False)
    o = (1.0, 2.0, 3.0)
    for got in (t.pair_counts_rppi([1], [1], observer=o), t.pair_counts_smu([1], [1], observer=o)):
        assert got.dtype == np.uint64 and np.array_equal(got, [[10, 2], [3, 4]])
    assert seen == [o, o]


# ------------------------------------------------- the float32 reference itself
# (no zero rp or s edge: rp2 = fl(s2 - pi2) of a pair along the line of sight
# has an absolute error of a few ulps of s2, so rp = 0 is not resolved to 1e-4
# of the last edge; the zero mu and pi edges are resolved)
G_E1 = np.array([0.01, 0.02, 0.05, 0.05, 0.11], np.float32)
G_PI = np.array([0.0, 0.005, 0.02, 0.02, 0.3], np.float32)
G_MU = np.array([0.0, 0.25, 0.5, 0.5, 1.0], np.float32)
GEOMETRIES = {"outside": ((0.5, 0.5, -2.0), 0.0), "inside": ((0.5, 0.5, 0.5), 0.0),
              "offset": ((0.0, 0.0, 0.0), 1000.0)}


@functools.lru_cache(maxsize=None)
def geometry_inputs(shift):
    pts = (uniform(6000, 401) + np.float32(shift)).astype(np.float32)
    q = (uniform(1500, 402) + np.float32(shift)).astype(np.float32)
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


@pytest.mark.parametrize("mode, e2", [(RPPI, G_PI), (SMU, G_MU)], ids=["rppi", "smu"])
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_float32_reference_against_the_float64_geometry(name, mode, e2):
    """The counts differ by no more than the number of pairs within 1e-4 (of
    the last edge) of an edge.  Measured: a summed difference of 0 in every
    case, against 264 to 315 such pairs in (rp, pi) and 48 to 59 in (s, mu)."""
    o, shift = GEOMETRIES[name]
    pts, q = geometry_inputs(shift)
    ref = ob.hist2_obs_ref(pts, q, G_E1, e2, mode, o, chunk=128)
    geo, near = ob.hist2_obs_geo(pts, q, G_E1, e2, mode, o, chunk=128)
    diff = int(np.abs(ref.astype(np.int64) - geo.astype(np.int64)).sum())
    print(f"{name} mode {mode}: summed difference {diff}, near-edge pairs {near}, "
          f"total {int(ref.sum())}")
    assert ref.sum() > 10_000
    assert diff <= near
