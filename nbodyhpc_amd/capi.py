"""ctypes binding of the C ABI (include/nbkd.h) — the binding a ctypes caller
of the reference's hot path would add.  Loads the in-tree
nbodyhpc_amd/lib/libnbkd.so and raises if it is missing: there is no fallback.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
# NBKD_LIB: an alternative build of the library (A/B experiments)
LIB_PATH = os.environ.get("NBKD_LIB") or os.path.join(PKG, "lib", "libnbkd.so")
HEADER = os.path.join(os.path.dirname(PKG), "include", "nbkd.h")

NBKD_OK, NBKD_EINVAL, NBKD_EBOX, NBKD_ETOOMANY, NBKD_ENOMEM, NBKD_EDEVICE, NBKD_EINTR = range(7)
NBKD_INPUT_DEVICE = 0x1
NBKD_OUTPUT_DEVICE = 0x2
NBKD_ACCUMULATE = 0x4
NBKD_SQUARED = 0x8
NBKD_SORTED = 0x10
# nbkd_query_ball_sum kernels and channel limit
KERNEL_TOPHAT, KERNEL_CUBIC, KERNEL_WENDLAND = 0, 1, 2
NBKD_MAX_VALUES = 4
NBKD_MAX_RADII = 32
# nbkd_query_ball_hist2 modes and the second axis' bin limit
NBKD_HIST2_RPPI, NBKD_HIST2_SMU = 0, 1
NBKD_MAX_LOS_BINS = 64
NBKD_EWALD_N = 64

NODE_DTYPE = np.dtype([("dim", "<i4"), ("split", "<f4"), ("left", "<u4"), ("right", "<u4")])


class NbkdError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


_c_p = ctypes.c_void_p
_u64 = ctypes.c_uint64
_i32 = ctypes.c_int32
_u32 = ctypes.c_uint32

_PROTOS = {
    "nbkd_build": (_i32, [_c_p, _u64, _i32, _i32, ctypes.c_float, _i32, _u32, _c_p,
                          ctypes.POINTER(_c_p)]),
    "nbkd_set_kth_out": (_i32, [_c_p, _c_p, _u64]),
    "nbkd_build_ext": (_i32, [_c_p, _u64, _i32, _i32, ctypes.c_float, _c_p, _i32, _u32, _c_p,
                              ctypes.POINTER(_c_p)]),
    "nbkd_query_knn": (_i32, [_c_p, _c_p, _u64, _i32, _c_p, _c_p, _u32, _c_p]),
    "nbkd_query_kth": (_i32, [_c_p, _c_p, _u64, _i32, _c_p, _u32, _c_p]),
    "nbkd_query_ball_count": (_i32, [_c_p, _c_p, _u64, ctypes.c_float, _c_p, _u32, _c_p]),
    "nbkd_query_ball_hist": (_i32, [_c_p, _c_p, _u64, _c_p, _i32, _c_p, _c_p, _u32, _c_p]),
    "nbkd_query_ball_hist2": (_i32, [_c_p, _c_p, _u64, _i32, _i32, _c_p, _i32, _c_p, _i32, _c_p,
                                     _u32, _c_p]),
    "nbkd_query_ball_hist2_obs": (_i32, [_c_p, _c_p, _u64, _i32, _c_p, _c_p, _i32, _c_p, _i32,
                                         _c_p, _u32, _c_p]),
    "nbkd_query_ball_sum": (_i32, [_c_p, _c_p, _u64, _c_p, _c_p, _i32, _i32, _c_p, _c_p, _u32,
                                   _c_p]),
    "nbkd_query_ball_profile": (_i32, [_c_p, _c_p, _u64, _c_p, _c_p, _i32, _c_p, _i32, _c_p, _u32,
                                       _c_p]),
    "nbkd_gravity": (_i32, [_c_p, _c_p, _u64, _c_p, ctypes.c_float, ctypes.c_float, _c_p, _c_p,
                            _u32, _c_p]),
    "nbkd_gravity_ewald": (_i32, [_c_p, _c_p, _u64, _c_p, ctypes.c_float, ctypes.c_float, _c_p,
                                  _c_p, _u32, _c_p]),
    "nbkd_ewald_table": (_i32, [_c_p, _u64]),
    "nbkd_query_ball_csr": (_i32, [_c_p, _c_p, _u64, ctypes.c_float, _c_p, _c_p, _u64, _u32,
                                   _c_p]),
    "nbkd_fof": (_i32, [_c_p, ctypes.c_float, _c_p, _c_p, ctypes.POINTER(_u64), _u32, _c_p]),
    "nbkd_group_catalog": (_i32, [_c_p, _c_p, _c_p, _c_p, _i32, _u32, _u64, _u64,
                                  ctypes.POINTER(_u64), ctypes.POINTER(_u64), _c_p, _c_p, _c_p,
                                  _c_p, _c_p, _c_p, _u32, _c_p]),
    "nbkd_group_potential": (_i32, [_c_p, _c_p, _c_p, _u64, _u64, _c_p, ctypes.c_float, _u32,
                                    _c_p, _c_p, _u32, _c_p]),
    "nbkd_tree_info": (_i32, [_c_p, ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                              ctypes.POINTER(_i32), ctypes.POINTER(ctypes.c_float),
                              ctypes.POINTER(_i32)]),
    "nbkd_export": (_i32, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nbkd_free": (None, [_c_p]),
    "nbkd_last_error": (ctypes.c_char_p, []),
    "nbkd_device_count": (_i32, [ctypes.POINTER(_i32)]),
    "nbkd_timing_enable": (_i32, [_i32]),
    "nbkd_timing_reset": (_i32, []),
    "nbkd_timing_read": (_i32, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                ctypes.POINTER(_u64)]),
    "nbkd_stats_enable": (_i32, [_i32]),
    "nbkd_stats_read": (_i32, [ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "nbkd_stats_read_all": (_i32, [ctypes.POINTER(_u64), _i32]),
    "nbkd_set_ids": (_i32, [_c_p, _c_p, _u32, _c_p]),
    "nbkd_slab_select": (_i32, [_c_p, _c_p, _u64, ctypes.c_float, ctypes.c_float, _c_p, _c_p,
                                _u64, ctypes.POINTER(_u64), _i32, _c_p]),
    "nbkd_slab_violations": (_i32, [_c_p, _c_p, _u64, _i32, ctypes.c_float, ctypes.c_float,
                                    ctypes.c_float, ctypes.POINTER(_u64), _i32, _c_p]),
    "nbkd_slab_forward": (_i32, [_c_p, _c_p, _u64, _i32, ctypes.c_float, ctypes.c_float, _c_p,
                                 _c_p, _u64, ctypes.POINTER(_u64), _i32, _c_p]),
    "nbkd_slab_forward_async": (_i32, [_c_p, _c_p, _u64, _i32, ctypes.c_float, ctypes.c_float,
                                       _c_p, _c_p, _u64, _c_p, _i32, _c_p]),
    "nbkd_rows_gather": (_i32, [_c_p, _u64, _c_p, _u64, _c_p, _i32, _c_p]),
    "nbkd_rows_scatter": (_i32, [_c_p, _u64, _c_p, _u64, _c_p, _i32, _c_p]),
    "nbkd_set_tuning": (_i32, [ctypes.c_char_p, ctypes.c_double]),
    "nbkd_set_interrupt": (_i32, [_c_p, _c_p]),
    "nbkd_get_tuning": (_i32, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]),
    "nbkd_collect_wide_addr": (_i32, [_u64]),
    "nbkd_collect_instance": (_i32, [_i32, _u64, _u64]),
    "nbkd_collect_stage_offsets": (_i32, [_u64, _u64]),
    "nbkd_comm_probe": (_i32, []),
    "nbkd_comm_unique_id": (_i32, [_c_p]),
    "nbkd_comm_init": (_i32, [_c_p, _i32, _i32, _i32, ctypes.POINTER(_c_p)]),
    "nbkd_comm_exchange": (_i32, [_c_p, _i32, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "nbkd_comm_free": (None, [_c_p]),
    "nbkd_deposit": (_i32, [_c_p, _c_p, _c_p, _u64, _i32, _i32, _i32, ctypes.c_float, _c_p, _i32,
                            _i32, _i32, _i32, _c_p, _i32, _u32, _c_p]),
}
COMM_ID_BYTES = 128


def header_symbols() -> list[str]:
    """Function names declared in include/nbkd.h."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbkd_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `python -m nbodyhpc_amd.build`")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(st):
    if st != NBKD_OK:
        raise NbkdError(st, lib().nbkd_last_error().decode())


def device_count() -> int:
    c = _i32(0)
    _check(lib().nbkd_device_count(ctypes.byref(c)))
    return c.value


def _host_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Tree:
    """Owning handle over an nbkd_tree*.  Inputs are numpy arrays (host) or raw
    device pointers (int) with `device_ptrs=True`."""

    def __init__(self, points=None, leafsize=128, boxsize=None, device=-1, *, n=None,
                 dev_ptr=None, stream=None, extent=None):
        L = lib()
        h = _c_p()
        flags = 0
        if dev_ptr is not None:
            ptr, count, flags = dev_ptr, n, NBKD_INPUT_DEVICE
        else:
            pts = _host_f32(points)
            if pts.ndim != 2 or pts.shape[1] != 3:
                raise RuntimeError("positions must be a 2D array of shape (N, 3)")
            ptr, count = pts.ctypes.data, pts.shape[0]
            self._keep = pts
        periodic = boxsize is not None
        # extent (ex, ey, ez): nbkd_build_ext, split axes by the points' extent
        # (slab trees); None: the reference's depth % 3
        ext = None if extent is None else (ctypes.c_float * 3)(*[float(e) for e in extent])
        ext = None if ext is None else ctypes.cast(ext, ctypes.c_void_p)
        st = L.nbkd_build_ext(ptr, count, int(leafsize), 1 if periodic else 0,
                              float(boxsize) if periodic else 0.0, ext, int(device), flags,
                              stream, ctypes.byref(h))
        _check(st)
        self.h = h
        self._keep = None
        self.npoints = int(count)  # the caller's point count (self.n is the padded one)
        n8, nn, per, box, dev = _u64(), _u64(), _i32(), ctypes.c_float(), _i32()
        _check(L.nbkd_tree_info(h, ctypes.byref(n8), ctypes.byref(nn), ctypes.byref(per),
                                ctypes.byref(box), ctypes.byref(dev)))
        self.n, self.size = n8.value, nn.value
        self.periodic, self.boxsize, self.device = bool(per.value), box.value, dev.value

    def close(self):
        if getattr(self, "h", None):
            lib().nbkd_free(self.h)
            self.h = None

    __del__ = close

    def export(self):
        nodes = np.empty(self.size, NODE_DTYPE)
        x, y, z = (np.empty(self.n, np.float32) for _ in range(3))
        idx = np.empty(self.n, np.uint32)
        _check(lib().nbkd_export(self.h, nodes.ctypes.data, x.ctypes.data, y.ctypes.data,
                                 z.ctypes.data, idx.ctypes.data))
        return nodes, x, y, z, idx

    def query(self, q, k, squared=False):
        """(m, k) distances and ids; squared=True: d2 instead of sqrtf(d2)."""
        q = _host_f32(q).reshape(-1, 3)
        m = q.shape[0]
        d = np.empty((m, k), np.float32)
        i = np.empty((m, k), np.uint32)
        _check(lib().nbkd_query_knn(self.h, q.ctypes.data, m, int(k), d.ctypes.data,
                                    i.ctypes.data, NBKD_SQUARED if squared else 0, None))
        return d, i

    def query_device(self, q_ptr, m, k, d_ptr, i_ptr, stream=None, input_device=True,
                     squared=False):
        flags = (NBKD_OUTPUT_DEVICE | (NBKD_INPUT_DEVICE if input_device else 0)
                 | (NBKD_SQUARED if squared else 0))
        _check(lib().nbkd_query_knn(self.h, q_ptr, int(m), int(k), d_ptr, i_ptr, flags, stream))

    def query_kth(self, q, k):
        """Distance to the k-th neighbour (column k-1 of query()), float32 (m,)."""
        q = _host_f32(q)
        out = np.empty(q.shape[0], np.float32)
        _check(lib().nbkd_query_kth(self.h, q.ctypes.data, q.shape[0], int(k), out.ctypes.data, 0,
                                    None))
        return out

    def query_kth_device(self, q_ptr, m, k, d_ptr, stream=None, input_device=True):
        flags = NBKD_OUTPUT_DEVICE | (NBKD_INPUT_DEVICE if input_device else 0)
        _check(lib().nbkd_query_kth(self.h, q_ptr, int(m), int(k), d_ptr, flags, stream))

    def set_kth_out(self, dev_ptr=None, capacity=0):
        """nbkd_set_kth_out: self queries with device rows also write each row's
        k-th distance to dev_ptr[row] (None detaches)."""
        _check(lib().nbkd_set_kth_out(self.h, dev_ptr, int(capacity) if dev_ptr else 0))

    def set_ids(self, ids=None, *, dev_ptr=None, stream=None):
        """Map the tree's point ids through `ids` (host array or device pointer)."""
        if dev_ptr is not None:
            _check(lib().nbkd_set_ids(self.h, dev_ptr, NBKD_INPUT_DEVICE, stream))
        else:
            a = np.ascontiguousarray(ids, dtype=np.uint32)
            _check(lib().nbkd_set_ids(self.h, a.ctypes.data, 0, stream))

    def ball_count(self, q, r):
        q = _host_f32(q)
        out = np.empty(q.shape[0], np.uint32)
        _check(lib().nbkd_query_ball_count(self.h, q.ctypes.data, q.shape[0], float(r),
                                           out.ctypes.data, 0, None))
        return out

    def ball_count_device(self, q_ptr, m, r, out_ptr, stream=None):
        _check(lib().nbkd_query_ball_count(self.h, q_ptr, int(m), float(r), out_ptr,
                                           NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE, stream))

    def ball_hist(self, q, radii, counts=True, total=True):
        """nbkd_query_ball_hist of host queries: (cumulative counts (m, nr) uint32
        or None, column sums (nr,) uint64 or None) for the ascending radii."""
        q = _host_f32(q).reshape(-1, 3)
        r = _host_f32(radii).reshape(-1)
        m, nr = q.shape[0], r.shape[0]
        c = np.empty((m, nr), np.uint32) if counts else None
        t = np.empty(nr, np.uint64) if total else None
        _check(lib().nbkd_query_ball_hist(self.h, q.ctypes.data, m, r.ctypes.data, nr,
                                          c.ctypes.data if counts else None,
                                          t.ctypes.data if total else None, 0, None))
        return c, t

    def ball_hist_device(self, q_ptr, m, radii, out_ptr, total=True, stream=None):
        """Device queries, device counts ((m, nr) uint32; out_ptr None: totals
        only); returns the (nr,) uint64 totals (the call then waits for them)
        or None (the call returns once enqueued)."""
        r = _host_f32(radii).reshape(-1)
        t = np.empty(r.shape[0], np.uint64) if total else None
        _check(lib().nbkd_query_ball_hist(self.h, q_ptr, int(m), r.ctypes.data, r.shape[0],
                                          out_ptr, t.ctypes.data if total else None,
                                          NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE, stream))
        return t

    def ball_hist2(self, q, edges1, edges2, mode, los=2):
        """nbkd_query_ball_hist2 of host queries: the (n1, n2) uint64 pair counts,
        (rp, pi) bins for NBKD_HIST2_RPPI, (s, mu) bins for NBKD_HIST2_SMU."""
        q = _host_f32(q).reshape(-1, 3)
        e1 = _host_f32(edges1).reshape(-1)
        e2 = _host_f32(edges2).reshape(-1)
        t = np.empty((e1.shape[0], e2.shape[0]), np.uint64)
        _check(lib().nbkd_query_ball_hist2(self.h, q.ctypes.data, q.shape[0], int(mode), int(los),
                                           e1.ctypes.data, e1.shape[0], e2.ctypes.data,
                                           e2.shape[0], t.ctypes.data, 0, None))
        return t

    def ball_hist2_device(self, q_ptr, m, edges1, edges2, mode, los=2, stream=None):
        """Device queries; returns the (n1, n2) uint64 pair counts (the call
        waits for them)."""
        e1 = _host_f32(edges1).reshape(-1)
        e2 = _host_f32(edges2).reshape(-1)
        t = np.empty((e1.shape[0], e2.shape[0]), np.uint64)
        _check(lib().nbkd_query_ball_hist2(self.h, q_ptr, int(m), int(mode), int(los),
                                           e1.ctypes.data, e1.shape[0], e2.ctypes.data,
                                           e2.shape[0], t.ctypes.data, NBKD_INPUT_DEVICE, stream))
        return t

    def ball_hist2_obs(self, q, edges1, edges2, mode, observer):
        """nbkd_query_ball_hist2_obs of host queries: the (n1, n2) uint64 pair
        counts with each pair's line of sight from ``observer`` (3 floats)
        through the pair's midpoint."""
        q = _host_f32(q).reshape(-1, 3)
        e1 = _host_f32(edges1).reshape(-1)
        e2 = _host_f32(edges2).reshape(-1)
        o = _host_f32(observer).reshape(3)
        t = np.empty((e1.shape[0], e2.shape[0]), np.uint64)
        _check(lib().nbkd_query_ball_hist2_obs(self.h, q.ctypes.data, q.shape[0], int(mode),
                                               o.ctypes.data, e1.ctypes.data, e1.shape[0],
                                               e2.ctypes.data, e2.shape[0], t.ctypes.data, 0,
                                               None))
        return t

    def ball_hist2_obs_device(self, q_ptr, m, edges1, edges2, mode, observer, stream=None):
        """Device queries; returns the (n1, n2) uint64 pair counts (the call
        waits for them)."""
        e1 = _host_f32(edges1).reshape(-1)
        e2 = _host_f32(edges2).reshape(-1)
        o = _host_f32(observer).reshape(3)
        t = np.empty((e1.shape[0], e2.shape[0]), np.uint64)
        _check(lib().nbkd_query_ball_hist2_obs(self.h, q_ptr, int(m), int(mode), o.ctypes.data,
                                               e1.ctypes.data, e1.shape[0], e2.ctypes.data,
                                               e2.shape[0], t.ctypes.data, NBKD_INPUT_DEVICE,
                                               stream))
        return t

    def ball_sum(self, q, h, values=None, kernel=1, count=False):
        """nbkd_query_ball_sum of host arrays: the raw float32 sums, (m,) without
        values or for 1-D values, else (m, nv); with count=True the pair (sums,
        counts (m,) uint32).  h: one radius per query; values: (n,) or (n, nv)
        by input row; kernel: KERNEL_TOPHAT / KERNEL_CUBIC / KERNEL_WENDLAND."""
        q = _host_f32(q).reshape(-1, 3)
        m = q.shape[0]
        hh = _host_f32(h).reshape(-1)
        if hh.shape[0] != m:
            raise ValueError("h must hold one radius per query")
        v, nv = None, 1
        if values is not None:
            v = _host_f32(values)
            if v.ndim not in (1, 2) or v.shape[0] != self.npoints:
                raise ValueError("values must be (n,) or (n, nv) with n the tree's point count")
            nv = 1 if v.ndim == 1 else v.shape[1]
        flat = v is None or v.ndim == 1
        s = np.empty(m if flat else (m, nv), np.float32)
        c = np.empty(m, np.uint32) if count else None
        _check(lib().nbkd_query_ball_sum(self.h, q.ctypes.data, m, hh.ctypes.data,
                                         None if v is None else v.ctypes.data, int(nv),
                                         int(kernel), s.ctypes.data,
                                         c.ctypes.data if count else None, 0, None))
        return (s, c) if count else s

    def ball_sum_device(self, q_ptr, m, h_ptr, values_ptr, nv, kernel, sum_ptr, count_ptr=None,
                        stream=None):
        """Device queries, radii, values ((n, nv) or None) and outputs ((m, nv)
        float32 sums and / or (m,) uint32 counts); returns once enqueued."""
        _check(lib().nbkd_query_ball_sum(self.h, q_ptr, int(m), h_ptr, values_ptr, int(nv),
                                         int(kernel), sum_ptr, count_ptr,
                                         NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE, stream))

    def ball_profile(self, q, radii, values=None, scale=None):
        """nbkd_query_ball_profile of host arrays: the raw float32 per-bin sums,
        (m, nr) without values or for 1-D values, else (m, nr, nv).  radii:
        ascending, shared by the queries; scale: one factor per query or None
        (edges radii[k] * scale[i]); values: (n,) or (n, nv) by input row."""
        q = _host_f32(q).reshape(-1, 3)
        m = q.shape[0]
        r = _host_f32(radii).reshape(-1)
        nr = r.shape[0]
        sc = None
        if scale is not None:
            sc = _host_f32(scale).reshape(-1)
            if sc.shape[0] != m:
                raise ValueError("scale must hold one factor per query")
        v, nv = None, 1
        if values is not None:
            v = _host_f32(values)
            if v.ndim not in (1, 2) or v.shape[0] != self.npoints:
                raise ValueError("values must be (n,) or (n, nv) with n the tree's point count")
            nv = 1 if v.ndim == 1 else v.shape[1]
        flat = v is None or v.ndim == 1
        s = np.empty((m, nr) if flat else (m, nr, nv), np.float32)
        _check(lib().nbkd_query_ball_profile(self.h, q.ctypes.data, m,
                                             None if sc is None else sc.ctypes.data,
                                             r.ctypes.data, nr,
                                             None if v is None else v.ctypes.data, int(nv),
                                             s.ctypes.data, 0, None))
        return s

    def ball_profile_device(self, q_ptr, m, radii, scale_ptr, values_ptr, nv, sum_ptr,
                            stream=None):
        """Device queries, scales ((m,) or None), values ((n, nv) or None) and
        sums ((m, nr, nv) float32); the radii are host memory.  Returns once
        enqueued."""
        r = _host_f32(radii).reshape(-1)
        _check(lib().nbkd_query_ball_profile(self.h, q_ptr, int(m), scale_ptr, r.ctypes.data,
                                             r.shape[0], values_ptr, int(nv), sum_ptr,
                                             NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE, stream))

    def gravity(self, q, mass=None, theta=0.5, eps=0.0, phi=True, acc=True):
        """nbkd_gravity of host arrays, G = 1: (phi (m,) float32 or None, acc
        (m, 3) float32 or None).  mass: (n,) by input row, or None (mass 1);
        theta: the opening angle in [0, 1), 0 = the direct sum; eps: the
        Plummer softening."""
        q = _host_f32(q).reshape(-1, 3)
        m = q.shape[0]
        w = None
        if mass is not None:
            w = _host_f32(mass)
            if w.shape != (self.npoints,):
                raise ValueError("mass must be (n,) with n the tree's point count")
        p = np.empty(m, np.float32) if phi else None
        a = np.empty((m, 3), np.float32) if acc else None
        _check(lib().nbkd_gravity(self.h, q.ctypes.data, m, None if w is None else w.ctypes.data,
                                  float(theta), float(eps), p.ctypes.data if phi else None,
                                  a.ctypes.data if acc else None, 0, None))
        return p, a

    def gravity_device(self, q_ptr, m, mass_ptr, theta, eps, phi_ptr, acc_ptr=None, stream=None):
        """Device queries, masses ((n,) or None) and outputs ((m,) float32
        potentials and / or (m, 3) float32 accelerations); returns once enqueued."""
        _check(lib().nbkd_gravity(self.h, q_ptr, int(m), mass_ptr, float(theta), float(eps),
                                  phi_ptr, acc_ptr, NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE,
                                  stream))

    def gravity_ewald(self, q, mass=None, theta=0.5, eps=0.0, phi=True, acc=True):
        """nbkd_gravity_ewald of host arrays on a periodic tree, G = 1: (phi
        (m,) float32 or None, acc (m, 3) float32 or None), the arguments of
        gravity.  A query outside [0, L]^3 gets NaNs."""
        q = _host_f32(q).reshape(-1, 3)
        m = q.shape[0]
        w = None
        if mass is not None:
            w = _host_f32(mass)
            if w.shape != (self.npoints,):
                raise ValueError("mass must be (n,) with n the tree's point count")
        p = np.empty(m, np.float32) if phi else None
        a = np.empty((m, 3), np.float32) if acc else None
        _check(lib().nbkd_gravity_ewald(self.h, q.ctypes.data, m,
                                        None if w is None else w.ctypes.data, float(theta),
                                        float(eps), p.ctypes.data if phi else None,
                                        a.ctypes.data if acc else None, 0, None))
        return p, a

    def gravity_ewald_device(self, q_ptr, m, mass_ptr, theta, eps, phi_ptr, acc_ptr=None,
                             stream=None):
        """Device queries, masses ((n,) or None) and outputs ((m,) float32
        potentials and / or (m, 3) float32 accelerations); returns once enqueued."""
        _check(lib().nbkd_gravity_ewald(self.h, q_ptr, int(m), mass_ptr, float(theta), float(eps),
                                        phi_ptr, acc_ptr, NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE,
                                        stream))

    def fof(self, b, sizes=True):
        """nbkd_fof into host arrays: (labels (n,) uint32 = the smallest input
        row of each point's group, sizes (n,) uint32 or None, ngroups)."""
        n = self.npoints
        lab = np.empty(n, np.uint32)
        siz = np.empty(n, np.uint32) if sizes else None
        ng = _u64()
        _check(lib().nbkd_fof(self.h, float(b), lab.ctypes.data,
                              siz.ctypes.data if sizes else None, ctypes.byref(ng), 0, None))
        return lab, siz, ng.value

    def fof_device(self, b, labels_ptr, sizes_ptr=None, stream=None):
        """nbkd_fof into device arrays ((n,) uint32 each); returns once enqueued."""
        _check(lib().nbkd_fof(self.h, float(b), labels_ptr, sizes_ptr, None,
                              NBKD_OUTPUT_DEVICE, stream))

    def group_catalog(self, labels, min_members=1, weight=None, values=None, members=True):
        """nbkd_group_catalog of host arrays, sized with one call and filled
        with a second: (head (G,) uint32, size (G,) uint32, offsets (G + 1,)
        uint64 or None, members (K,) uint32 or None, moments (G, 5 + 2 nv)
        float64, dmax (G,) float32).  labels: (n,) canonical (the output of
        fof); weight: (n,) or None; values: (n,) or (n, nv) or None."""
        n = self.npoints
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        if lab.shape != (n,):
            raise ValueError("labels must be (n,) with n the tree's point count")
        w = None
        if weight is not None:
            w = _host_f32(weight)
            if w.shape != (n,):
                raise ValueError("weight must be (n,) with n the tree's point count")
        v, nv = None, 0
        if values is not None:
            v = _host_f32(values)
            if v.ndim not in (1, 2) or v.shape[0] != n:
                raise ValueError("values must be (n,) or (n, nv) with n the tree's point count")
            v = np.ascontiguousarray(v.reshape(n, -1))
            nv = v.shape[1]
        wp = None if w is None else w.ctypes.data
        vp = None if v is None else v.ctypes.data
        ng, nm = _u64(), _u64()
        _check(lib().nbkd_group_catalog(self.h, lab.ctypes.data, wp, vp, nv, int(min_members), 0,
                                        0, ctypes.byref(ng), ctypes.byref(nm), None, None, None,
                                        None, None, None, 0, None))
        G, K = ng.value, nm.value
        head, size = np.empty(G, np.uint32), np.empty(G, np.uint32)
        off = np.zeros(G + 1, np.uint64) if members else None
        mem = np.empty(K, np.uint32) if members else None
        mom = np.empty((G, 5 + 2 * nv), np.float64)
        dmax = np.empty(G, np.float32)
        if G:
            _check(lib().nbkd_group_catalog(self.h, lab.ctypes.data, wp, vp, nv,
                                            int(min_members), G, K, ctypes.byref(ng),
                                            ctypes.byref(nm), head.ctypes.data, size.ctypes.data,
                                            off.ctypes.data if members else None,
                                            mem.ctypes.data if members else None,
                                            mom.ctypes.data, dmax.ctypes.data, 0, None))
        return head, size, off, mem, mom, dmax

    def group_catalog_device(self, labels_ptr, weight_ptr, values_ptr, nv, min_members,
                             group_capacity, member_capacity, head_ptr=None, size_ptr=None,
                             offsets_ptr=None, members_ptr=None, moments_ptr=None, dmax_ptr=None,
                             stream=None):
        """nbkd_group_catalog with device inputs and device outputs (raw
        pointers, any output may be None); returns (G, K).  Nothing but the
        counts is written when G > group_capacity or K > member_capacity."""
        ng, nm = _u64(), _u64()
        _check(lib().nbkd_group_catalog(self.h, labels_ptr, weight_ptr, values_ptr, int(nv),
                                        int(min_members), int(group_capacity),
                                        int(member_capacity), ctypes.byref(ng), ctypes.byref(nm),
                                        head_ptr, size_ptr, offsets_ptr, members_ptr,
                                        moments_ptr, dmax_ptr,
                                        NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE, stream))
        return ng.value, nm.value

    def group_potential(self, offsets, members, mass=None, eps=0.0, max_members=0, phi=True,
                        minpos=True):
        """nbkd_group_potential of host arrays, G = 1: (phi (K,) float32 or
        None, minpos (ngroups,) uint32 or None).  offsets (ngroups + 1,) and
        members (K,): the rows of each group (any grouping); mass: (n,) by
        input row, or None (mass 1); max_members: larger groups are skipped
        (NaN, 0xFFFFFFFF), 0 = no limit."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        mem = np.ascontiguousarray(members, dtype=np.uint32)
        if off.ndim != 1 or off.shape[0] < 1 or mem.ndim != 1:
            raise ValueError("offsets must be (ngroups + 1,) and members (K,)")
        w = None
        if mass is not None:
            w = _host_f32(mass)
            if w.shape != (self.npoints,):
                raise ValueError("mass must be (n,) with n the tree's point count")
        G, K = off.shape[0] - 1, mem.shape[0]
        p = np.empty(K, np.float32) if phi else None
        mp = np.empty(G, np.uint32) if minpos else None
        # (K == 0: no array to point at; the library reads no member)
        mptr = mem.ctypes.data if K else np.zeros(1, np.uint32).ctypes.data
        _check(lib().nbkd_group_potential(self.h, off.ctypes.data, mptr, G, K,
                                          None if w is None else w.ctypes.data, float(eps),
                                          int(max_members), p.ctypes.data if phi else None,
                                          mp.ctypes.data if minpos else None, 0, None))
        return p, mp

    def group_potential_device(self, offsets_ptr, members_ptr, ngroups, nmembers, mass_ptr, eps,
                               max_members, phi_ptr, minpos_ptr=None, stream=None):
        """Device offsets, members, masses ((n,) or None) and outputs ((K,)
        float32 potentials and / or (ngroups,) uint32 entries); the call waits
        (the violation count of the list is read on the host)."""
        _check(lib().nbkd_group_potential(self.h, offsets_ptr, members_ptr, int(ngroups),
                                          int(nmembers), mass_ptr, float(eps), int(max_members),
                                          phi_ptr, minpos_ptr,
                                          NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE, stream))

    def ball_csr(self, q, r, sorted=False):
        """CSR radius query of host queries: (offsets (m + 1,) uint64, ids);
        sorted=True: each row ascending (NBKD_SORTED, sorted on the device)."""
        q = _host_f32(q)
        m = q.shape[0]
        fl = NBKD_SORTED if sorted else 0
        off = np.empty(m + 1, np.uint64)
        _check(lib().nbkd_query_ball_csr(self.h, q.ctypes.data, m, float(r), off.ctypes.data,
                                         None, 0, fl, None))
        idx = np.empty(int(off[-1]), np.uint32)
        _check(lib().nbkd_query_ball_csr(self.h, q.ctypes.data, m, float(r), off.ctypes.data,
                                         idx.ctypes.data if idx.size else None, idx.size, fl,
                                         None))
        return off, idx

    def ball_csr_device(self, q_ptr, m, r, off, idx_ptr, capacity, sorted=False, stream=None):
        """Device queries and device ids (offsets in host memory `off`,
        (m + 1,) uint64); idx_ptr None: the counts pass only."""
        fl = NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE | (NBKD_SORTED if sorted else 0)
        _check(lib().nbkd_query_ball_csr(self.h, q_ptr, int(m), float(r), off.ctypes.data,
                                         idx_ptr, int(capacity), fl, stream))
        return off


def deposit(xyz, weight, radius, grid, ppu, period=(-1.0, -1.0, -1.0), subsample=4, mode=0,
            device=-1, out=None, window=None):
    """Host arrays in, float32 grid (gx, gy, nz) in Fortran order out (nbkd_deposit).
    `window` = (x0, wx): only columns [x0, x0 + wx) of the gx-wide grid, shape
    (wx, gy, nz).  `out` (that shape, Fortran-contiguous float32): accumulate into it."""
    p, w, r = _host_f32(xyz), _host_f32(weight), _host_f32(radius)
    gx, gy, nz = (int(v) for v in grid)
    x0, wx = (0, gx) if window is None else (int(window[0]), int(window[1]))
    per = np.ascontiguousarray(period, np.float32)
    flags = 0
    if out is None:
        out = np.empty((wx, gy, nz), np.float32, order="F")
    else:
        if out.dtype != np.float32 or out.shape != (wx, gy, nz) or not out.flags.f_contiguous:
            raise ValueError("out must be a Fortran-ordered float32 array of the grid's shape")
        flags |= NBKD_ACCUMULATE
    _check(lib().nbkd_deposit(p.ctypes.data, w.ctypes.data, r.ctypes.data, p.shape[0], gx, gy, nz,
                              float(ppu), per.ctypes.data, int(subsample), int(mode), x0, wx,
                              out.ctypes.data, int(device), flags, None))
    return out


def deposit_device(xyz_ptr, weight_ptr, radius_ptr, n, grid, ppu, out_ptr,
                   period=(-1.0, -1.0, -1.0), subsample=4, mode=0, device=-1, accumulate=False,
                   stream=None, window=None):
    """Device pointers in and out; returns once the deposit is enqueued."""
    gx, gy, nz = (int(v) for v in grid)
    x0, wx = (0, gx) if window is None else (int(window[0]), int(window[1]))
    per = np.ascontiguousarray(period, np.float32)
    flags = NBKD_INPUT_DEVICE | NBKD_OUTPUT_DEVICE | (NBKD_ACCUMULATE if accumulate else 0)
    _check(lib().nbkd_deposit(xyz_ptr, weight_ptr, radius_ptr, int(n), gx, gy, nz, float(ppu),
                              per.ctypes.data, int(subsample), int(mode), x0, wx, out_ptr,
                              int(device), flags, stream))


def ewald_table():
    """nbkd_ewald_table: the correction table of nbkd_gravity_ewald, float32
    (65, 65, 65, 4): [i, j, k] = (C_phi, C_ax, C_ay, C_az) at the offset
    (i, j, k) / 128 in units of the box.  Needs no device."""
    nn = NBKD_EWALD_N + 1
    out = np.empty((nn, nn, nn, 4), np.float32)
    _check(lib().nbkd_ewald_table(out.ctypes.data, out.size))
    return out


def set_tuning(name, value):
    """nbkd_set_tuning: "knn_seed_margin" (default 3.5), "candidate_bytes" (0 = auto)."""
    _check(lib().nbkd_set_tuning(name.encode(), float(value)))


def get_tuning(name):
    v = ctypes.c_double()
    _check(lib().nbkd_get_tuning(name.encode(), ctypes.byref(v)))
    return v.value


def collect_wide_addr(nodes):
    """nbkd_collect_wide_addr: whether a tree of `nodes` nodes takes the collect
    kernel's wide-address instance (the "collect_wide_addr" knob forces it)."""
    return bool(lib().nbkd_collect_wide_addr(int(nodes)))


def collect_instance(leafsize, points, nodes):
    """nbkd_collect_instance: (one_chunk, narrow) -- whether a tree of `points`
    points and `nodes` nodes built with `leafsize` takes the collect kernel's
    one-chunk instance (leaf size <= 64; the "collect_one_chunk" knob turns it
    off), and whether its loads take 32-bit byte offsets."""
    v = lib().nbkd_collect_instance(int(leafsize), int(points), int(nodes))
    return bool(v & 1), bool(v & 2)


def collect_stage_offsets(points, nodes):
    """nbkd_collect_stage_offsets: which of the one-chunk instance's staging
    offsets fit 32 bits, as (points, group boxes, leaf boxes)."""
    v = lib().nbkd_collect_stage_offsets(int(points), int(nodes))
    return bool(v & 1), bool(v & 2), bool(v & 4)


def timing_enable(on=True):
    _check(lib().nbkd_timing_enable(1 if on else 0))


def timing_reset():
    _check(lib().nbkd_timing_reset())


def timing_read(name):
    ms, cnt = ctypes.c_double(), _u64()
    _check(lib().nbkd_timing_read(name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
    return ms.value, cnt.value


def stats_enable(on=True):
    _check(lib().nbkd_stats_enable(1 if on else 0))


def stats_read():
    a, b = _u64(), _u64()
    _check(lib().nbkd_stats_read(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


# work counters of the last kNN call (collect kernel, knn_collect.hip): nodes
# entered x packet lanes, (query, point) distance evaluations, dense point steps,
# sparse (lane-compacted) iterations, leaf points staged, packets (waves),
# candidates appended, leaves scanned, queries sent to the exact kernel,
# queries retried with a larger seed ball; then the collect kernel's phase
# clocks (shader cycles summed over waves): tree walk, leaf staging wait, leaf
# need test, dense scan, sparse scan, bound update; lanes needing a staged
# chunk, summed over chunks
STATS_NAMES = ("node_visits", "pair_evals", "leaves_reached", "sparse_iters", "points_staged",
               "packets", "candidates", "leaves_scanned", "fallback_queries", "retry_queries",
               "clk_walk", "clk_wait", "clk_leaf_test", "clk_dense", "clk_sparse", "clk_tighten",
               "chunk_lanes")


# the same slots after a radius count with stats enabled (ball.hip STATS instance)
BALL_STATS_NAMES = ("node_visits", "points_evaluated", "leaves_needed", "transposed_steps",
                    "points_staged", "packets", "full_lane_leaves", "partial_lane_leaves",
                    "lane_loop_chunks", "unused9", "clk_walk", "clk_leaf_test", "clk_wait",
                    "clk_transposed", "clk_lane_loop", "unused15", "unused16")


def ball_stats_read_all():
    arr = (_u64 * len(BALL_STATS_NAMES))()
    _check(lib().nbkd_stats_read_all(arr, len(BALL_STATS_NAMES)))
    return dict(zip(BALL_STATS_NAMES, [int(v) for v in arr]))


def stats_read_all():
    arr = (_u64 * len(STATS_NAMES))()
    _check(lib().nbkd_stats_read_all(arr, len(STATS_NAMES)))
    return dict(zip(STATS_NAMES, [int(v) for v in arr]))


# ------------------------------------------------------------------ slabs / RCCL
def slab_select(xyz_ptr, ids_ptr, n, lo, hi, out_xyz_ptr=None, out_ids_ptr=None, capacity=0,
                device=0, stream=None):
    """Device-side stable selection of points with lo <= x < hi; returns the count."""
    c = _u64()
    _check(lib().nbkd_slab_select(xyz_ptr, ids_ptr, int(n), float(lo), float(hi), out_xyz_ptr,
                                  out_ids_ptr, int(capacity), ctypes.byref(c), int(device), stream))
    return c.value


def slab_violations(q_ptr, dist_ptr, m, k, lo, hi, h, device=0, stream=None):
    c = _u64()
    _check(lib().nbkd_slab_violations(q_ptr, dist_ptr, int(m), int(k), float(lo), float(hi),
                                      float(h), ctypes.byref(c), int(device), stream))
    return c.value


def slab_forward_async(q_ptr, dist_ptr, m, k, cl, ch, count_ptr, list_ptr=None, sides_ptr=None,
                       capacity=0, device=0, stream=None):
    """nbkd_slab_forward_async: the same test, its total in the device word
    count_ptr when the stream gets there (nothing is waited for)."""
    _check(lib().nbkd_slab_forward_async(q_ptr, dist_ptr, int(m), int(k), float(cl), float(ch),
                                         list_ptr, sides_ptr, int(capacity), count_ptr,
                                         int(device), stream))


def slab_forward(q_ptr, dist_ptr, m, k, cl, ch, list_ptr=None, sides_ptr=None, capacity=0,
                 device=0, stream=None):
    """nbkd_slab_forward: total count of own queries whose k-th distance reaches
    past cl (left) or ch (right); up to `capacity` (index, side bits) entries."""
    c = _u64()
    _check(lib().nbkd_slab_forward(q_ptr, dist_ptr, int(m), int(k), float(cl), float(ch), list_ptr,
                                   sides_ptr, int(capacity), ctypes.byref(c), int(device), stream))
    return c.value


def rows_gather(src_ptr, row_bytes, idx_ptr, n, dst_ptr, device=0, stream=None):
    _check(lib().nbkd_rows_gather(src_ptr, int(row_bytes), idx_ptr, int(n), dst_ptr, int(device),
                                  stream))


def rows_scatter(src_ptr, row_bytes, idx_ptr, n, dst_ptr, device=0, stream=None):
    _check(lib().nbkd_rows_scatter(src_ptr, int(row_bytes), idx_ptr, int(n), dst_ptr, int(device),
                                   stream))


def comm_probe() -> None:
    """Raises unless RCCL loads (no bootstrap listener is started)."""
    _check(lib().nbkd_comm_probe())


def comm_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(lib().nbkd_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """RCCL communicator over librccl (dlopen'ed by libnbkd)."""

    def __init__(self, uid: bytes, rank: int, world: int, device: int):
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        h = _c_p()
        _check(lib().nbkd_comm_init(buf, int(rank), int(world), int(device), ctypes.byref(h)))
        self.h = h

    def exchange(self, pairs, stream=None):
        """pairs: list of (send_ptr, send_bytes, send_peer, recv_ptr, recv_bytes, recv_peer)."""
        n = len(pairs)
        sp = (_c_p * n)(*[p[0] for p in pairs])
        sb = (_u64 * n)(*[int(p[1]) for p in pairs])
        speer = (_i32 * n)(*[int(p[2]) for p in pairs])
        rp = (_c_p * n)(*[p[3] for p in pairs])
        rb = (_u64 * n)(*[int(p[4]) for p in pairs])
        rpeer = (_i32 * n)(*[int(p[5]) for p in pairs])
        _check(lib().nbkd_comm_exchange(self.h, n, sp, sb, speer, rp, rb, rpeer, stream))

    def close(self):
        if getattr(self, "h", None):
            lib().nbkd_comm_free(self.h)
            self.h = None

    __del__ = close
