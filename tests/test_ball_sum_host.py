"""CPU tests of the kernel-sum boundary (nbkd_query_ball_sum): the symbol is
declared, bound and exported, every argument check runs before any device call
and leaves the outputs alone, the two type stubs agree, and the Python wrappers
(kernel_sum / sph_density / interpolate) reject bad arguments without a device."""
import ctypes
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_exported():
    assert "nbkd_query_ball_sum" in capi.header_symbols()
    assert "nbkd_query_ball_sum" in capi._PROTOS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "nbkd_query_ball_sum")
    txt = open(capi.HEADER).read()
    for line in ("#define NBKD_KERNEL_TOPHAT   0", "#define NBKD_KERNEL_CUBIC    1",
                 "#define NBKD_KERNEL_WENDLAND 2", "#define NBKD_MAX_VALUES 4"):
        assert line in txt
    assert "equal under ==" in txt  # the determinism statement
    assert (capi.KERNEL_TOPHAT, capi.KERNEL_CUBIC, capi.KERNEL_WENDLAND) == (0, 1, 2)
    assert capi.NBKD_MAX_VALUES == 4


class Args:
    """A well-formed call on a stand-in tree handle.  The argument checks (and
    m == 0) return before the handle is looked at, so no device is needed; the
    outputs hold a sentinel."""

    def __init__(self):
        self.tree = ctypes.create_string_buffer(1 << 16)
        self.q = np.zeros((4, 3), np.float32)
        self.h = np.ones(4, np.float32)
        self.v = np.ones((8, 4), np.float32)
        self.s = np.full((4, 4), 77.0, np.float32)
        self.c = np.full(4, 77, np.uint32)

    def call(self, **kw):
        a = dict(tree=ctypes.addressof(self.tree), q=self.q.ctypes.data, m=4,
                 h=self.h.ctypes.data, values=self.v.ctypes.data, nv=4, kernel=1,
                 out_sum=self.s.ctypes.data, out_count=self.c.ctypes.data)
        a.update(kw)
        L = capi.lib()
        st = L.nbkd_query_ball_sum(a["tree"], a["q"], a["m"], a["h"], a["values"], a["nv"],
                                   a["kernel"], a["out_sum"], a["out_count"], 0, None)
        return st, L.nbkd_last_error()

    def untouched(self):
        return bool(np.all(self.s == 77.0) and np.all(self.c == 77))


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"NULL"),
    (dict(q=None), b"NULL"),
    (dict(h=None), b"NULL"),
    (dict(out_sum=None, out_count=None), b"both NULL"),
    (dict(nv=0), b"channels"),
    (dict(nv=5), b"channels"),
    (dict(nv=-1), b"channels"),
    (dict(values=None, nv=2), b"nv == 1"),
    (dict(kernel=3), b"unknown kernel"),
    (dict(kernel=-1), b"unknown kernel"),
    (dict(m=1 << 32), b"2^32"),
])
def test_invalid_arguments_rejected_before_any_device_call(kw, word):
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


def test_type_stubs_declare_ball_sum_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def ball_sum(" in a
    assert a == b


def wrapper(n=10):
    """A KDTree whose native part was never constructed: the wrappers check
    their arguments before they reach it."""
    from nbodyhpc_amd.kdtree import KDTree
    t = KDTree.__new__(KDTree)
    t._n_input = n
    return t


Q = np.zeros((3, 3), np.float32)


@pytest.mark.parametrize("h", [-1.0, float("nan"), float("inf"), [0.1, -0.1, 0.1],
                               [0.1, float("nan"), 0.1]])
def test_kernel_sum_rejects_bad_radii(h):
    with pytest.raises(ValueError, match="finite"):
        wrapper().kernel_sum(Q, h)
    with pytest.raises(ValueError, match="finite"):
        wrapper().sph_density(Q, h=h)
    with pytest.raises(ValueError, match="finite"):
        wrapper().interpolate(Q, h, np.zeros(10))


def test_kernel_sum_rejects_bad_values_and_kernels():
    t = wrapper()
    with pytest.raises(ValueError, match="values"):
        t.kernel_sum(Q, 0.1, values=np.zeros(9))
    with pytest.raises(ValueError, match="values"):
        t.kernel_sum(Q, 0.1, values=np.zeros((11, 2)))
    with pytest.raises(ValueError, match="channels"):
        t.kernel_sum(Q, 0.1, values=np.zeros((10, 5)))
    with pytest.raises(ValueError, match="values"):
        t.kernel_sum(Q, 0.1, values=np.zeros((10, 2, 2)))
    with pytest.raises(ValueError, match="broadcast"):
        t.kernel_sum(Q, [0.1, 0.2])
    for name in ("gauss", "Cubic", 1, None):
        with pytest.raises(ValueError, match="unknown kernel"):
            t.kernel_sum(Q, 0.1, kernel=name)
        with pytest.raises(ValueError, match="unknown kernel"):
            t.sph_density(Q, kernel=name)
        with pytest.raises(ValueError, match="unknown kernel"):
            t.interpolate(Q, 0.1, np.zeros(10), kernel=name)


def test_sph_density_and_interpolate_reject_bad_shapes():
    t = wrapper()
    with pytest.raises(ValueError, match="mass"):
        t.sph_density(Q, mass=np.ones(9))
    with pytest.raises(ValueError, match="mass"):
        t.sph_density(Q, mass=np.ones((10, 2)))
    with pytest.raises(ValueError, match="field"):
        t.interpolate(Q, 0.1, np.zeros(9))
    with pytest.raises(ValueError, match="channels"):
        t.interpolate(Q, 0.1, np.zeros((10, 4)))
    with pytest.raises(ValueError, match="mass"):
        t.interpolate(Q, 0.1, np.zeros(10), mass=np.ones(3))
