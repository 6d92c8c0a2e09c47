"""CPU tests of the group-potential boundary (nbkd_group_potential): the symbol
is declared, bound and exported, every argument check that needs no device
runs before any device call and leaves the outputs alone, the two type stubs
agree, and the Python wrappers (group_potential, unbind) reject bad arguments
without a device."""
import ctypes
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_exported():
    assert "nbkd_group_potential" in capi.header_symbols()
    assert "nbkd_group_potential" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_group_potential")
    txt = open(capi.HEADER).read()
    doc = txt[txt.index("per-group potentials"):txt.index("nbkd_status nbkd_group_potential(")]
    assert "equal under ==" in doc  # the determinism statement
    assert "Scratch:" in doc
    assert "1e12 terms" in doc and "max_members" in doc  # the cost warning
    assert "dmax < L/2" in doc  # where the periodic result is meaningful


class Args:
    """A well-formed call on a stand-in tree handle (zeroed memory: a tree of
    no points).  The argument checks return before the handle is looked at,
    so no device is needed; the outputs hold a sentinel."""

    def __init__(self):
        self.tree = ctypes.create_string_buffer(1 << 16)
        self.off = np.array([0, 3, 8], np.uint64)
        self.mem = np.arange(8, dtype=np.uint32)
        self.mass = np.ones(8, np.float32)
        self.phi = np.full(8, 77.0, np.float32)
        self.minpos = np.full(2, 77, np.uint32)

    def call(self, **kw):
        a = dict(tree=ctypes.addressof(self.tree), off=self.off.ctypes.data,
                 mem=self.mem.ctypes.data, ng=2, nm=8, mass=self.mass.ctypes.data, eps=0.0,
                 maxm=0, phi=self.phi.ctypes.data, minpos=self.minpos.ctypes.data)
        a.update(kw)
        L = capi.lib()
        st = L.nbkd_group_potential(a["tree"], a["off"], a["mem"], a["ng"], a["nm"], a["mass"],
                                    ctypes.c_float(a["eps"]), a["maxm"], a["phi"], a["minpos"],
                                    0, None)
        return st, L.nbkd_last_error()

    def untouched(self):
        return bool(np.all(self.phi == 77)) and bool(np.all(self.minpos == 77))


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"NULL"),
    (dict(off=None), b"NULL"),
    (dict(mem=None), b"NULL"),
    (dict(phi=None, minpos=None), b"both NULL"),
    (dict(eps=float("nan")), b"eps"),
    (dict(eps=-1.0), b"eps"),
    (dict(eps=float("inf")), b"eps"),
    (dict(nm=1 << 32), b"2^32"),
    (dict(ng=1 << 32), b"2^32"),
])
def test_invalid_arguments_rejected_before_any_device_call(kw, word):
    a = Args()
    st, msg = a.call(**kw)
    assert st == capi.NBKD_EINVAL
    assert word in msg, msg
    assert a.untouched()


def test_no_groups_is_ok_and_writes_nothing():
    a = Args()
    st, _ = a.call(ng=0, nm=0)
    assert st == capi.NBKD_OK
    assert a.untouched()


def test_no_members_is_ok_and_marks_every_group_empty():
    a = Args()
    st, _ = a.call(nm=0)
    assert st == capi.NBKD_OK
    assert bool(np.all(a.phi == 77))
    assert bool(np.all(a.minpos == 0xFFFFFFFF))


def test_type_stubs_declare_group_potential_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def group_potential(" in a
    assert a == b


def wrapper(n=10):
    """A KDTree whose native part was never constructed: group_potential and
    unbind check their arguments before they reach it."""
    from nbodyhpc_amd.kdtree import KDTree
    t = KDTree.__new__(KDTree)
    t._n_input = n
    return t


OFF = np.array([0, 4, 10])
MEM = np.arange(10)


def test_group_potential_rejects_bad_arguments():
    t = wrapper()
    with pytest.raises(ValueError, match="offsets"):
        t.group_potential(np.zeros((2, 2), np.int64), MEM)
    with pytest.raises(ValueError, match="offsets"):
        t.group_potential(np.array([]), MEM)
    with pytest.raises(ValueError, match="offsets"):
        t.group_potential(np.array([0.0, 4.0, 10.0]), MEM)
    with pytest.raises(ValueError, match="offsets"):
        t.group_potential(np.array([1, 4, 10]), MEM)
    with pytest.raises(ValueError, match="offsets"):
        t.group_potential(np.array([0, 4, 9]), MEM)
    with pytest.raises(ValueError, match="offsets"):
        t.group_potential(np.array([0, 11, 10]), MEM)
    with pytest.raises(ValueError, match="members"):
        t.group_potential(OFF, MEM.reshape(5, 2))
    with pytest.raises(ValueError, match="members"):
        t.group_potential(OFF, MEM + 1)  # row 10 of 10 points
    with pytest.raises(ValueError, match="members"):
        t.group_potential(OFF, MEM - 1)
    with pytest.raises(ValueError, match="mass"):
        t.group_potential(OFF, MEM, mass=np.ones(9))
    with pytest.raises(ValueError, match="mass"):
        t.group_potential(OFF, MEM, mass=np.ones((10, 2)))
    with pytest.raises(ValueError, match="mass"):
        t.group_potential(OFF, MEM, mass=-np.ones(10))
    with pytest.raises(ValueError, match="mass"):
        t.group_potential(OFF, MEM, mass=np.full(10, np.nan))
    for bad in (-0.1, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="softening"):
            t.group_potential(OFF, MEM, softening=bad)
    with pytest.raises(ValueError, match="theta"):
        t.group_potential(OFF, MEM, theta=1.0)
    with pytest.raises(ValueError, match="max_direct"):
        t.group_potential(OFF, MEM, max_direct=0)


def test_unbind_rejects_bad_arguments():
    t = wrapper()
    vel = np.zeros((10, 3))
    with pytest.raises(ValueError, match="offsets"):
        t.unbind(np.array([0, 4, 9]), MEM, vel)
    with pytest.raises(ValueError, match="members"):
        t.unbind(OFF, MEM + 1, vel)
    with pytest.raises(ValueError, match="mass"):
        t.unbind(OFF, MEM, vel, mass=np.ones(3))
    with pytest.raises(ValueError, match="mass"):
        t.unbind(OFF, MEM, vel, mass=np.full(10, np.inf))
    with pytest.raises(ValueError, match="softening"):
        t.unbind(OFF, MEM, vel, softening=-1.0)
    with pytest.raises(ValueError, match="velocities"):
        t.unbind(OFF, MEM, np.zeros((9, 3)))
    with pytest.raises(ValueError, match="velocities"):
        t.unbind(OFF, MEM, np.zeros(10))
    with pytest.raises(ValueError, match="max_iter"):
        t.unbind(OFF, MEM, vel, max_iter=-1)
