"""CPU tests of the anisotropic pair-count boundary (nbkd_query_ball_hist2): the
symbol is declared, bound and exported, every argument check runs before any
device call and leaves the output alone, m == 0 zeroes the output, the two type
stubs agree, the Python wrappers reject bad arguments without a device, and
xi_rppi / xi_smu are the formulas of their docstrings when fed synthetic
counts."""
import ctypes
import math
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.uint64(77)


def test_symbol_declared_bound_and_exported():
    assert "nbkd_query_ball_hist2" in capi.header_symbols()
    assert "nbkd_query_ball_hist2" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_query_ball_hist2")
    assert (capi.NBKD_HIST2_RPPI, capi.NBKD_HIST2_SMU, capi.NBKD_MAX_LOS_BINS) == (0, 1, 64)
    txt = open(capi.HEADER).read()
    assert "#define NBKD_HIST2_RPPI 0" in txt
    assert "#define NBKD_HIST2_SMU  1" in txt
    assert "#define NBKD_MAX_LOS_BINS 64" in txt
    assert "no per-query rows, no pair weights and no jackknife" in txt
    assert "hist2_flush_visits" in txt


class Args:
    """A well-formed call on a stand-in tree handle.  The argument checks (and
    m == 0) return before the handle is looked at, so no device is needed; the
    output holds a sentinel."""

    def __init__(self):
        self.tree = ctypes.create_string_buffer(1 << 16)
        self.q = np.zeros((4, 3), np.float32)
        self.out = np.full((32, 64), SENTINEL, np.uint64)

    def call(self, **kw):
        a = dict(tree=ctypes.addressof(self.tree), q=self.q.ctypes.data, m=4,
                 mode=capi.NBKD_HIST2_SMU, los=2, e1=[0.1, 0.2, 0.2, 0.4], n1=None,
                 e2=[0.0, 0.5, 0.5, 1.0], n2=None, out=self.out.ctypes.data)
        a.update(kw)
        e1 = None if a["e1"] is None else np.ascontiguousarray(a["e1"], np.float32)
        e2 = None if a["e2"] is None else np.ascontiguousarray(a["e2"], np.float32)
        n1 = a["n1"] if a["n1"] is not None else len(e1)
        n2 = a["n2"] if a["n2"] is not None else len(e2)
        L = capi.lib()
        st = L.nbkd_query_ball_hist2(a["tree"], a["q"], a["m"], a["mode"], a["los"],
                                     None if e1 is None else e1.ctypes.data, n1,
                                     None if e2 is None else e2.ctypes.data, n2, a["out"], 0,
                                     None)
        return st, L.nbkd_last_error()

    def untouched(self):
        return bool(np.all(self.out == SENTINEL))


RPPI = dict(mode=capi.NBKD_HIST2_RPPI)


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"NULL"),
    (dict(q=None), b"NULL"),
    (dict(e1=None, n1=4), b"NULL"),
    (dict(e2=None, n2=4), b"NULL"),
    (dict(out=None), b"NULL"),
    (dict(mode=2), b"unknown mode 2"),
    (dict(mode=-1), b"unknown mode -1"),
    (dict(los=3), b"los must be 0, 1 or 2, got 3"),
    (dict(los=-1), b"los must be 0, 1 or 2, got -1"),
    (dict(n1=0), b"number of first-axis edges"),
    (dict(n1=-1), b"number of first-axis edges"),
    (dict(e1=np.linspace(0.1, 1, 33)), b"number of first-axis edges"),
    (dict(n2=0), b"number of second-axis edges"),
    (dict(e2=np.linspace(0.0, 1, 65)), b"got 65"),
    (dict(e2=np.linspace(0.0, 1, 65), **RPPI), b"got 65"),
    (dict(e1=[0.1, 0.3, 0.2]), b"first-axis edges must be ascending (edge 2"),
    (dict(e2=[0.1, 0.3, 0.2]), b"second-axis edges must be ascending (edge 2"),
    (dict(e1=[0.1, float("nan")]), b"first-axis edge 1 is NaN, infinite or negative"),
    (dict(e1=[0.1, float("inf")]), b"first-axis edge 1 is NaN, infinite or negative"),
    (dict(e1=[-0.5, 0.1]), b"first-axis edge 0 is NaN, infinite or negative"),
    (dict(e2=[float("nan"), 0.1]), b"second-axis edge 0 is NaN, infinite or negative"),
    (dict(e2=[0.1, float("inf")], **RPPI), b"second-axis edge 1 is NaN, infinite or negative"),
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
    assert msg.startswith(b"nbkd_query_ball_hist2")
    assert a.untouched()


def test_pi_edges_may_pass_one():
    """the bound of 1 belongs to mu edges only: with m == 0 an (rp, pi) call
    with pi edges above 1 is fine"""
    a = Args()
    st, _ = a.call(m=0, e2=[0.5, 1.0, 1.5], **RPPI)
    assert st == capi.NBKD_OK


def test_no_queries_zeroes_the_output():
    a = Args()
    st, _ = a.call(m=0)
    assert st == capi.NBKD_OK
    flat = a.out.reshape(-1)
    assert np.all(flat[:16] == 0) and np.all(flat[16:] == SENTINEL)


def test_tuning_knobs_exist():
    for name in ("hist2_flush_visits", "hist2_copies"):
        assert capi.get_tuning(name) == 0.0
        capi.set_tuning(name, 3)
        try:
            assert capi.get_tuning(name) == 3.0
        finally:
            capi.set_tuning(name, 0)


def test_type_stubs_declare_query_ball_hist2_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def query_ball_hist2(" in a
    assert a == b


def wrapper(n=10, periodic=True, box=1.0):
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


def test_count_pairs_reject_bad_edges():
    t = wrapper()
    for fn, second in ((t.count_pairs_rppi, "pi"), (t.count_pairs_smu, "mu")):
        first = "rp" if second == "pi" else "s"
        ok = [0.1, 0.2]
        for bad, word in (([[0.1, 0.2]], "1-D"), ([], "empty"), ([0.1, float("nan")], "finite"),
                          ([0.1, float("inf")], "finite"), ([-0.1, 0.1], "finite"),
                          ([0.2, 0.1], "ascending")):
            with pytest.raises(ValueError, match=word):
                fn(Q, bad, ok)
            with pytest.raises(ValueError, match=word):
                fn(Q, ok, bad)
        with pytest.raises(ValueError, match=f"{first} holds 33 edges: at most 32"):
            fn(Q, np.linspace(0.1, 1, 33), ok)
        with pytest.raises(ValueError, match=f"{second} holds 65 edges: at most 64"):
            fn(Q, ok, np.linspace(0.0, 1, 65))
        for los in (-1, 3, 1.5, None):
            with pytest.raises(ValueError, match="los"):
                fn(Q, ok, ok, los=los)
    with pytest.raises(ValueError, match="<= 1"):
        t.count_pairs_smu(Q, [0.1], [0.5, 1.5])


def test_xi_reject_bad_arguments():
    t = wrapper(periodic=False)
    with pytest.raises(ValueError, match="periodic"):
        t.xi_rppi([0.1, 0.2], 0.1, 4)
    with pytest.raises(ValueError, match="periodic"):
        t.xi_smu([0.1, 0.2], 4)
    t = wrapper()
    with pytest.raises(ValueError, match="two edges"):
        t.xi_rppi([0.1], 0.1, 4)
    with pytest.raises(ValueError, match="strictly"):
        t.xi_smu([0.1, 0.1, 0.2], 4)
    for npi in (0, 65, 2.5):
        with pytest.raises(ValueError, match="npi"):
            t.xi_rppi([0.1, 0.2], 0.1, npi)
        with pytest.raises(ValueError, match="nmu"):
            t.xi_smu([0.1, 0.2], npi)
    with pytest.raises(ValueError, match="half the box"):
        t.xi_rppi([0.1, 0.51], 0.1, 4)
    with pytest.raises(ValueError, match="half the box"):
        t.xi_rppi([0.1, 0.2], 0.51, 4)
    with pytest.raises(ValueError, match="half the box"):
        t.xi_smu([0.1, 0.51], 4)
    for pi_max in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pi_max"):
            t.xi_rppi([0.1, 0.2], pi_max, 4)


def synthetic(shape, seed):
    return np.random.default_rng(seed).integers(1, 10_000, size=shape).astype(np.uint64)


def test_xi_rppi_is_its_formula(monkeypatch):
    n, L = 5000, 2.5
    t = wrapper(n, box=L)
    rp = np.array([0.03, 0.05, 0.1, 0.3, 0.7], np.float32)
    npi, pi_max = 7, 1.1
    counts = synthetic((5, npi), 1)
    seen = {}

    def fake(points, e1, e2, los=2):
        seen.update(points=points, e1=np.array(e1), e2=np.array(e2), los=los)
        return counts

    monkeypatch.setattr(t, "count_pairs_rppi", fake, raising=False)
    monkeypatch.setattr(t, "points", lambda: "own points", raising=False)
    xi, wp = t.xi_rppi(rp, pi_max, npi, los=1)
    assert seen["points"] == "own points" and seen["los"] == 1
    assert seen["e1"].dtype == np.float32 and np.array_equal(seen["e1"], rp)
    pe = np.array([np.float32(pi_max * (l + 1) / npi) for l in range(npi)], np.float32)
    assert seen["e2"].dtype == np.float32 and np.array_equal(seen["e2"], pe)
    assert xi.shape == (4, npi) and wp.shape == (4,) and xi.dtype == np.float64
    p = [0.0] + [float(x) for x in pe]
    for i in range(4):
        lo, hi = float(rp[i]), float(rp[i + 1])
        acc = 0.0
        for l in range(npi):
            v = math.pi * (hi * hi - lo * lo) * 2.0 * (p[l + 1] - p[l])
            want = float(counts[i + 1, l]) / (n * (n / L ** 3) * v) - 1.0
            assert xi[i, l] == pytest.approx(want, rel=1e-12)
            acc += want * (p[l + 1] - p[l])
        assert wp[i] == pytest.approx(2.0 * acc, rel=1e-12)


def test_xi_smu_is_its_formula(monkeypatch):
    n, L = 4000, 67.77
    t = wrapper(n, box=L)
    s = np.array([0.5, 1.0, 2.0, 4.5, 9.0, 20.0], np.float32)
    nmu = 6
    counts = synthetic((6, nmu), 2)
    seen = {}

    def fake(points, e1, e2, los=2):
        seen.update(e1=np.array(e1), e2=np.array(e2), los=los)
        return counts

    monkeypatch.setattr(t, "count_pairs_smu", fake, raising=False)
    monkeypatch.setattr(t, "points", lambda: None, raising=False)
    xi, poles = t.xi_smu(s, nmu)
    assert seen["los"] == 2 and np.array_equal(seen["e1"], s)
    me = np.array([np.float32((l + 1) / nmu) for l in range(nmu)], np.float32)
    assert np.array_equal(seen["e2"], me) and me[-1] == np.float32(1.0)
    assert sorted(poles) == [0, 2, 4] and xi.shape == (5, nmu)
    u = [0.0] + [float(x) for x in me]
    leg = {0: lambda x: 1.0, 2: lambda x: 0.5 * (3 * x * x - 1),
           4: lambda x: (35 * x ** 4 - 30 * x * x + 3) / 8.0}
    for i in range(5):
        lo, hi = float(s[i]), float(s[i + 1])
        acc = {0: 0.0, 2: 0.0, 4: 0.0}
        for l in range(nmu):
            v = (4.0 * math.pi / 3.0) * (hi ** 3 - lo ** 3) * (u[l + 1] - u[l])
            want = float(counts[i + 1, l]) / (n * (n / L ** 3) * v) - 1.0
            assert xi[i, l] == pytest.approx(want, rel=1e-12)
            mid = 0.5 * (u[l + 1] + u[l])
            for ell in acc:
                acc[ell] += want * leg[ell](mid) * (u[l + 1] - u[l])
        for ell in acc:
            assert poles[ell][i] == pytest.approx((2 * ell + 1) * acc[ell], rel=1e-12, abs=1e-13)
    _, only = t.xi_smu(s, nmu, ells=(2,))
    assert list(only) == [2] and np.array_equal(only[2], poles[2])


def test_auto_counts_remove_self_pairs_and_halve(monkeypatch):
    t = wrapper(10)
    ordered = np.array([[30, 4], [6, 8]], np.uint64)
    monkeypatch.setattr(t, "points", lambda: None, raising=False)
    monkeypatch.setattr(t, "count_pairs_rppi", lambda *a, **k: ordered, raising=False)
    monkeypatch.setattr(t, "count_pairs_smu", lambda *a, **k: ordered, raising=False)
    for got in (t.pair_counts_rppi([1], [1]), t.pair_counts_smu([1], [1])):
        assert got.dtype == np.uint64 and np.array_equal(got, [[10, 2], [3, 4]])
    assert ordered[0, 0] == 30
