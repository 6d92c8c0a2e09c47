"""CPU tests of the radius histogram's boundary (nbkd_query_ball_hist): the
symbol is declared, bound and exported, its argument checks run before any
device call, and the two type stubs agree."""
import ctypes
import os

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_exported():
    assert "nbkd_query_ball_hist" in capi.header_symbols()
    assert "nbkd_query_ball_hist" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_query_ball_hist")
    txt = open(capi.HEADER).read()
    assert "#define NBKD_MAX_RADII 32" in txt


def test_null_arguments_rejected():
    L = capi.lib()
    st = L.nbkd_query_ball_hist(None, None, 0, None, 0, None, None, 0, None)
    assert st == capi.NBKD_EINVAL
    assert b"NULL" in L.nbkd_last_error()


def test_type_stubs_declare_query_ball_hist_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def query_ball_hist(" in a
    assert a == b
