"""CPU tests of the group-catalogue boundary (nbkd_group_catalog): the symbol
is declared, bound and exported, every argument check runs before any device
call and leaves the outputs alone, the two type stubs agree, and the Python
wrapper (fof_catalog) rejects bad arguments without a device."""
import ctypes
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_exported():
    assert "nbkd_group_catalog" in capi.header_symbols()
    assert "nbkd_group_catalog" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_group_catalog")
    txt = open(capi.HEADER).read()
    assert "#define NBKD_GROUP_MOMENTS(nv) (5 + 2 * (nv))" in txt
    doc = txt[txt.index("the group catalogue"):txt.index("#define NBKD_GROUP_MOMENTS")]
    assert "equal under ==" in doc  # the determinism statement
    assert "Scratch:" in doc


class Args:
    """A well-formed call on a stand-in tree handle (zeroed memory: a tree of
    no points).  The argument checks return before the handle is looked at,
    so no device is needed; the outputs hold a sentinel."""

    def __init__(self):
        self.tree = ctypes.create_string_buffer(1 << 16)
        self.label = np.zeros(8, np.uint32)
        self.w = np.ones(8, np.float32)
        self.v = np.ones((8, 4), np.float32)
        self.ng = ctypes.c_uint64(77)
        self.nm = ctypes.c_uint64(77)
        self.head = np.full(8, 77, np.uint32)
        self.size = np.full(8, 77, np.uint32)
        self.off = np.full(9, 77, np.uint64)
        self.mem = np.full(8, 77, np.uint32)
        self.mom = np.full((8, 13), 77.0, np.float64)
        self.dmax = np.full(8, 77.0, np.float32)

    def call(self, **kw):
        a = dict(tree=ctypes.addressof(self.tree), label=self.label.ctypes.data,
                 weight=self.w.ctypes.data, values=self.v.ctypes.data, nv=4, min_members=1,
                 gcap=8, mcap=8, ng=ctypes.byref(self.ng), nm=ctypes.byref(self.nm))
        a.update(kw)
        L = capi.lib()
        st = L.nbkd_group_catalog(a["tree"], a["label"], a["weight"], a["values"], a["nv"],
                                  a["min_members"], a["gcap"], a["mcap"], a["ng"], a["nm"],
                                  self.head.ctypes.data, self.size.ctypes.data,
                                  self.off.ctypes.data, self.mem.ctypes.data,
                                  self.mom.ctypes.data, self.dmax.ctypes.data, 0, None)
        return st, L.nbkd_last_error()

    def arrays_untouched(self):
        return all(bool(np.all(x == 77)) for x in (self.head, self.size, self.off, self.mem,
                                                   self.mom, self.dmax))

    def untouched(self):
        return self.arrays_untouched() and self.ng.value == 77 and self.nm.value == 77


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"NULL"),
    (dict(label=None), b"NULL"),
    (dict(ng=None), b"NULL"),
    (dict(nm=None), b"NULL"),
    (dict(nv=5), b"channels"),
    (dict(nv=-1), b"channels"),
    (dict(values=None, nv=2), b"nv == 0"),
    (dict(nv=0), b"nv == 0"),
])
def test_invalid_arguments_rejected_before_any_device_call(kw, word):
    a = Args()
    st, msg = a.call(**kw)
    assert st == capi.NBKD_EINVAL
    assert word in msg, msg
    assert a.untouched()


def test_no_points_is_ok_with_zero_counts():
    a = Args()
    st, _ = a.call()
    assert st == capi.NBKD_OK
    assert a.ng.value == 0 and a.nm.value == 0
    assert a.arrays_untouched()


def test_type_stubs_declare_group_moments_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def group_moments(" in a
    assert a == b


def wrapper(n=10):
    """A KDTree whose native part was never constructed: fof_catalog checks
    its arguments before it reaches it."""
    from nbodyhpc_amd.kdtree import KDTree
    t = KDTree.__new__(KDTree)
    t._n_input = n
    return t


def test_fof_catalog_rejects_bad_arguments():
    t = wrapper()
    lab = np.arange(10)
    with pytest.raises(ValueError, match="linking_length"):
        t.fof_catalog(None)
    with pytest.raises(ValueError, match="mass"):
        t.fof_catalog(0.1, mass=np.ones(9))
    with pytest.raises(ValueError, match="mass"):
        t.fof_catalog(0.1, mass=np.ones((10, 2)))
    with pytest.raises(ValueError, match="values"):
        t.fof_catalog(0.1, values=np.zeros(9))
    with pytest.raises(ValueError, match="values"):
        t.fof_catalog(0.1, values=np.zeros((11, 2)))
    with pytest.raises(ValueError, match="values"):
        t.fof_catalog(0.1, values=np.zeros((10, 2, 2)))
    with pytest.raises(ValueError, match="channels"):
        t.fof_catalog(0.1, values=np.zeros((10, 5)))
    with pytest.raises(ValueError, match="labels"):
        t.fof_catalog(None, labels=lab[:9])
    with pytest.raises(ValueError, match="labels"):
        t.fof_catalog(0.1, labels=np.zeros((10, 2)))
    # a bad mass is reported although labels are given and well-formed
    with pytest.raises(ValueError, match="mass"):
        t.fof_catalog(None, labels=lab, mass=np.ones(3))
