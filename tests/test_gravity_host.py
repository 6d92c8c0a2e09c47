"""CPU tests of the gravity boundary (nbkd_gravity): the symbol is declared,
bound and exported, every argument check that needs no live tree runs before
the handle is looked at and leaves the outputs alone, the two type stubs agree,
and the Python wrappers (gravity / potential) reject bad arguments without a
device."""
import ctypes
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_exported():
    assert "nbkd_gravity" in capi.header_symbols()
    assert "nbkd_gravity" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_gravity")
    assert hasattr(capi.Tree, "gravity") and hasattr(capi.Tree, "gravity_device")
    txt = open(capi.HEADER).read()
    doc = txt[:txt.index("nbkd_status nbkd_gravity(")]
    doc = doc[doc.rindex("/*"):]
    # the definition and the determinism statement
    for phrase in ("s2 <= (theta*theta)*d2", "inv = 1.0f / sqrtf(r2)", "d2 == 0 adds nothing",
                   "no floating-point atomics", "equal under ==", "Ewald"):
        assert phrase in doc, phrase


class Args:
    """A well-formed call on a stand-in tree handle.  The argument checks (and
    m == 0) return before the handle is looked at, so no device is needed; the
    outputs hold a sentinel."""

    def __init__(self):
        self.tree = ctypes.create_string_buffer(1 << 16)
        self.q = np.zeros((4, 3), np.float32)
        self.mass = np.ones(8, np.float32)
        self.phi = np.full(4, 77.0, np.float32)
        self.acc = np.full((4, 3), 77.0, np.float32)

    def call(self, **kw):
        a = dict(tree=ctypes.addressof(self.tree), q=self.q.ctypes.data, m=4,
                 mass=self.mass.ctypes.data, theta=0.5, eps=0.01,
                 out_phi=self.phi.ctypes.data, out_acc=self.acc.ctypes.data)
        a.update(kw)
        L = capi.lib()
        st = L.nbkd_gravity(a["tree"], a["q"], a["m"], a["mass"], a["theta"], a["eps"],
                            a["out_phi"], a["out_acc"], 0, None)
        return st, L.nbkd_last_error()

    def untouched(self):
        return bool(np.all(self.phi == 77.0) and np.all(self.acc == 77.0))


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"NULL"),
    (dict(q=None), b"NULL"),
    (dict(out_phi=None, out_acc=None), b"both NULL"),
    (dict(theta=float("nan")), b"theta"),
    (dict(theta=-0.1), b"theta"),
    (dict(theta=1.0), b"theta"),
    (dict(theta=2.0), b"theta"),
    (dict(theta=float("inf")), b"theta"),
    (dict(eps=float("nan")), b"eps"),
    (dict(eps=-1.0), b"eps"),
    (dict(eps=float("inf")), b"eps"),
    (dict(m=1 << 32), b"2^32"),
])
def test_invalid_arguments_rejected_before_the_handle_is_looked_at(kw, word):
    a = Args()
    st, msg = a.call(**kw)
    assert st == capi.NBKD_EINVAL
    assert word in msg, msg
    assert a.untouched()


def test_no_queries_is_ok():
    a = Args()
    st, _ = a.call(m=0)
    assert st == capi.NBKD_OK
    assert a.untouched()


def test_type_stubs_declare_gravity_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def gravity(" in a
    assert a == b


def wrapper(n=10):
    """A KDTree whose native part was never constructed: the wrappers check
    their arguments before they reach it."""
    from nbodyhpc_amd.kdtree import KDTree
    t = KDTree.__new__(KDTree)
    t._n_input = n
    return t


Q = np.zeros((3, 3), np.float32)


@pytest.mark.parametrize("mass", [np.ones(9), np.ones((10, 2)), np.ones((10, 1)), 1.0])
def test_gravity_rejects_mass_of_the_wrong_shape(mass):
    with pytest.raises(ValueError, match="mass must be"):
        wrapper().gravity(Q, mass=mass)
    with pytest.raises(ValueError, match="mass must be"):
        wrapper().potential(Q, mass=mass)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_gravity_rejects_bad_masses(bad):
    m = np.ones(10)
    m[3] = bad
    with pytest.raises(ValueError, match="finite and >= 0"):
        wrapper().gravity(Q, mass=m)
    with pytest.raises(ValueError, match="finite and >= 0"):
        wrapper().potential(Q, mass=m)


@pytest.mark.parametrize("theta", [-0.1, 1.0, 1.5, float("nan"), float("inf"), 1.0 - 1e-12])
def test_gravity_rejects_theta_outside_the_unit_interval(theta):
    with pytest.raises(ValueError, match="theta"):
        wrapper().gravity(Q, theta=theta)
    with pytest.raises(ValueError, match="theta"):
        wrapper().potential(Q, theta=theta)


@pytest.mark.parametrize("eps", [-1e-3, float("nan"), float("inf"), 1e39])
def test_gravity_rejects_bad_softening(eps):
    with pytest.raises(ValueError, match="softening"):
        wrapper().gravity(Q, softening=eps)
    with pytest.raises(ValueError, match="softening"):
        wrapper().potential(Q, softening=eps)


def test_gravity_needs_an_output():
    with pytest.raises(ValueError, match="at least one"):
        wrapper().gravity(Q, potential=False, acceleration=False)
