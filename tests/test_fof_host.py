"""CPU tests of the friends-of-friends boundary (nbkd_fof): the symbol is
declared, bound and exported, its argument checks run before any device call,
and both type stubs declare fof_labels."""
import ctypes
import os

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_exported():
    assert "nbkd_fof" in capi.header_symbols()
    assert "nbkd_fof" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_fof")


def test_null_arguments_rejected():
    L = capi.lib()
    out = (ctypes.c_uint32 * 4)()
    st = L.nbkd_fof(None, 0.1, ctypes.cast(out, ctypes.c_void_p), None, None, 0, None)
    assert st == capi.NBKD_EINVAL
    assert b"NULL" in L.nbkd_last_error()
    assert list(out) == [0, 0, 0, 0]


def test_type_stubs_declare_fof_labels():
    for rel in ("nbodyhpc_amd/kdtree/_impl.pyi", "nbodyhpc/kdtree/_impl.pyi"):
        txt = open(os.path.join(ROOT, rel)).read()
        assert "def fof_labels(self, b: float)" in txt, rel
