"""CPU tests of the periodic gravity boundary (nbkd_gravity_ewald,
nbkd_ewald_table): the symbols are declared, bound and exported, every argument
check that needs no live tree runs before the handle is looked at and leaves
the outputs alone, the two type stubs agree, the Python wrappers reject bad
arguments without a device, and the correction table holds the float64 Ewald
sums of nbkd.h and interpolates them as closely as a float64 table does."""
import ctypes
import functools
import os

import numpy as np
import pytest

from nbodyhpc_amd import capi

from . import ewald_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24


def test_symbols_declared_bound_and_exported():
    for name in ("nbkd_gravity_ewald", "nbkd_ewald_table"):
        assert name in capi.header_symbols()
        assert name in capi._PROTOS
        assert hasattr(ctypes.CDLL(capi.LIB_PATH), name)
    assert hasattr(capi.Tree, "gravity_ewald") and hasattr(capi.Tree, "gravity_ewald_device")
    assert hasattr(capi, "ewald_table")
    txt = open(capi.HEADER).read()
    assert "#define NBKD_EWALD_N 64" in txt and capi.NBKD_EWALD_N == 64
    doc = txt[:txt.index("nbkd_status nbkd_gravity_ewald(")]
    doc = doc[doc.rindex("/*"):]
    for phrase in ("nearest image", "NBKD_EWALD_N", "d2 == 0 adds nothing", "erfc(a|x-n|)",
                   "i_a = min((int)t_a, 63)", "a + f*(b - a)", "-2.8372975",
                   "no floating-point atomics", "equal under ==", "nbkd_gravity"):
        assert phrase in doc, phrase
    # the old call points here and still says what it rejects
    old = txt[:txt.index("nbkd_status nbkd_gravity(")]
    old = old[old.rindex("/*"):]
    assert "nbkd_gravity_ewald" in old and "Ewald" in old


class Args:
    """A well-formed call on a stand-in tree handle (zeroed: not periodic).  The
    argument checks (and m == 0) return before the handle is looked at, so no
    device is needed; the outputs hold a sentinel."""

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
        st = L.nbkd_gravity_ewald(a["tree"], a["q"], a["m"], a["mass"], a["theta"], a["eps"],
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


def test_a_tree_that_is_not_periodic_is_rejected_before_any_device_call():
    """the stand-in handle is all zeros: a tree with periodic == 0"""
    a = Args()
    st, msg = a.call()
    assert st == capi.NBKD_EINVAL
    assert b"periodic" in msg and b"nbkd_gravity " in msg, msg
    assert a.untouched()


def test_no_queries_is_ok():
    a = Args()
    st, _ = a.call(m=0)
    assert st == capi.NBKD_OK
    assert a.untouched()


def test_table_export_checks_its_capacity():
    need = 65 ** 3 * 4
    buf = np.full(need, 77.0, np.float32)
    L = capi.lib()
    assert L.nbkd_ewald_table(buf.ctypes.data, need - 1) == capi.NBKD_EINVAL
    assert b"nbkd_ewald_table" in L.nbkd_last_error()
    assert L.nbkd_ewald_table(None, need) == capi.NBKD_EINVAL
    assert np.all(buf == 77.0)
    assert L.nbkd_ewald_table(buf.ctypes.data, need) == capi.NBKD_OK
    assert np.array_equal(buf.reshape(65, 65, 65, 4), table())


def test_type_stubs_declare_gravity_ewald_and_agree():
    a = open(os.path.join(ROOT, "nbodyhpc_amd", "kdtree", "_impl.pyi"), "rb").read()
    b = open(os.path.join(ROOT, "nbodyhpc", "kdtree", "_impl.pyi"), "rb").read()
    assert b"def gravity_ewald(" in a
    assert a == b
    from nbodyhpc_amd.kdtree import _impl
    assert hasattr(_impl.KDTree, "gravity_ewald")


def wrapper(n=10):
    """A KDTree whose native part was never constructed: the wrappers check
    their arguments before they reach it."""
    from nbodyhpc_amd.kdtree import KDTree
    t = KDTree.__new__(KDTree)
    t._n_input = n
    return t


Q = np.zeros((3, 3), np.float32)


@pytest.mark.parametrize("mass", [np.ones(9), np.ones((10, 2)), np.ones((10, 1)), 1.0])
def test_wrapper_rejects_mass_of_the_wrong_shape(mass):
    with pytest.raises(ValueError, match="mass must be"):
        wrapper().gravity_ewald(Q, mass=mass)
    with pytest.raises(ValueError, match="mass must be"):
        wrapper().potential_ewald(Q, mass=mass)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_wrapper_rejects_bad_masses(bad):
    m = np.ones(10)
    m[3] = bad
    with pytest.raises(ValueError, match="finite and >= 0"):
        wrapper().gravity_ewald(Q, mass=m)
    with pytest.raises(ValueError, match="finite and >= 0"):
        wrapper().potential_ewald(Q, mass=m)


@pytest.mark.parametrize("theta", [-0.1, 1.0, 1.5, float("nan"), float("inf"), 1.0 - 1e-12])
def test_wrapper_rejects_theta_outside_the_unit_interval(theta):
    with pytest.raises(ValueError, match="theta"):
        wrapper().gravity_ewald(Q, theta=theta)
    with pytest.raises(ValueError, match="theta"):
        wrapper().potential_ewald(Q, theta=theta)


@pytest.mark.parametrize("eps", [-1e-3, float("nan"), float("inf"), 1e39])
def test_wrapper_rejects_bad_softening(eps):
    with pytest.raises(ValueError, match="softening"):
        wrapper().gravity_ewald(Q, softening=eps)
    with pytest.raises(ValueError, match="softening"):
        wrapper().potential_ewald(Q, softening=eps)


def test_wrapper_needs_an_output():
    with pytest.raises(ValueError, match="at least one"):
        wrapper().gravity_ewald(Q, potential=False, acceleration=False)


# ---------------------------------------------------------------- the table
@functools.lru_cache(maxsize=None)
def table():
    t = capi.ewald_table()
    assert t.shape == (65, 65, 65, 4) and t.dtype == np.float32
    t.setflags(write=False)
    return t


def test_table_values():
    """2000 seeded nodes and the eight corners against the float64 sums:
    |T - ref| <= 2^-24 |ref| + 2e-9 (the stated 2e-9, then one rounding)."""
    T = table()
    assert T[0, 0, 0].tolist() == [float(np.float32(eo.C0)), 0.0, 0.0, 0.0]
    idx = np.random.default_rng(701).integers(0, 65, (2000, 3))
    corners = np.array([[a, b, c] for a in (0, 64) for b in (0, 64) for c in (0, 64)])
    idx = np.concatenate([idx, corners])
    cphi, ca = eo.corrections(idx / 128.0)
    ref = np.concatenate([cphi[:, None], ca], axis=1)
    got = T[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.float64)
    err = np.abs(got - ref)
    bound = U24 * np.abs(ref) + 2e-9
    print(f"worst table error over its bound: {np.max(err / bound):.3f}; "
          f"C_phi(0) from the sums: {cphi[-8]:.8f}")
    assert np.all(err <= bound), np.argwhere(err > bound)[:3]
    assert abs(cphi[-8] - eo.C0) < 5e-8  # (the oracle's own limit at the origin)
    # component a is odd in axis a: nothing on the plane x_a = 0 (x_a = 1/2 is
    # not zero: there C_a = -x_a/|x|^3, the nearest image's sign ambiguity)
    assert np.all(np.abs(T[0, :, :, 1]) <= 2e-9)
    assert np.all(np.abs(T[:, 0, :, 2]) <= 2e-9)
    assert np.all(np.abs(T[:, :, 0, 3]) <= 2e-9)
    assert np.all(np.isfinite(T))


# E_phi and E_a of a float64 numpy table rounded to float32, measured when the
# call was specified ("Interpolation error")
E_PHI_F64, E_A_F64 = 1.18e-4, 5.5e-4


def test_interpolation_error():
    """The maximum absolute error, in box units, of the trilinear interpolation
    of the exported table against the float64 sums over 20 000 seeded offsets in
    [-1/2, 1/2]^3: no more than 1.25 times that of a float64 table rounded to
    float32 (the two tables differ by rounding only)."""
    x = (np.random.default_rng(702).random((20000, 3)) - 0.5).astype(np.float32)
    got, _ = eo.interpolate(table(), x, 1.0)
    cphi, ca = eo.corrections(x.astype(np.float64))
    e_phi = float(np.max(np.abs(got[:, 0] - cphi)))
    e_a = float(np.max(np.abs(got[:, 1:] - ca)))
    print(f"E_phi = {e_phi:.3e}, E_a = {e_a:.3e}")
    assert e_phi <= 1.25 * E_PHI_F64
    assert e_a <= 1.25 * E_A_F64


def test_first_table_build_is_quick():
    """a fresh process computes the table in at most 2 s of wall time"""
    import subprocess
    import sys
    code = ("import time, ctypes, numpy as np\n"
            "from nbodyhpc_amd import capi\n"
            "L = capi.lib()\n"
            "t0 = time.perf_counter(); T = capi.ewald_table(); print(time.perf_counter() - t0)\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                         check=True).stdout
    dt = float(out.strip().splitlines()[-1])
    print(f"table build: {dt:.3f} s")
    assert dt <= 2.0
