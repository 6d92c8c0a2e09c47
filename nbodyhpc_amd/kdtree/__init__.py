"""MI355X-native drop-in for ``nbodyhpc.kdtree``.

Mirrors the reference wrapper kdtree/src/python/nbodyhpc/kdtree/__init__.py:11-56
(defaults leafsize=128, max_threads=-1; unknown keyword arguments warn;
N-D query arrays are flattened) on top of the pybind11 module ``_impl``
(mirror of kdtree/src/cpp/pybind.cpp), which drives the HIP kernels through
the C ABI in include/nbkd.h.  There is no CPU fallback: without the built
extension or without a GPU the constructor raises.

Additions (no reference counterpart): ``query_ball`` (scipy-style radius
query, count or index lists), ``count_neighbors`` / ``pair_counts`` (counts at
many radii in one tree walk), ``fof`` / ``fof_labels`` (friends-of-friends
groups of the tree's points), ``density`` (local number density from the k-th
neighbour distance or from a radius count), a ``device`` keyword, and
persistence: ``points()``, ``save`` / ``load`` (.npz,
no pickle inside) and pickling.  A restored tree is rebuilt on the GPU from
the saved points (the build is deterministic: same node table; ~55 ms at 1e8),
so neither the file nor the pickle carries device state.
Deviation: the reference's N-D reshape-back (``reshape(shape[:-1], k)``,
__init__.py:53-54) raises TypeError; here the result has shape
``shape[:-1] + (k,)``.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional, Tuple

import numpy as np

try:
    from ._impl import KDTree as cKDTree
    from ._impl import device_count
except ImportError as e:  # fail loudly: no CPU path exists
    raise ImportError(
        "nbodyhpc_amd.kdtree._impl is not built; run `python -m nbodyhpc_amd.build` "
        f"(hipcc for gfx950 + pybind11). Original error: {e}") from e

__all__ = ["KDTree", "cKDTree", "device_count"]


def _flatten(points):
    points = np.asarray(points)
    if points.ndim != 2:
        shape = points.shape
        return points.reshape((-1, shape[-1])), shape
    return points, None


class KDTree(cKDTree):
    """Spatial KD-tree, with optional periodic boundary conditions (GPU build and queries)."""

    def __init__(self, points: np.ndarray, leafsize: int = 128, max_threads: int = -1,
                 boxsize: Optional[float] = None, device: int = -1, **kwargs):
        """Build a new KDTree.

        Parameters
        ----------
        points : (N, 3) array of points (cast to float32).
        leafsize : maximum number of points in a leaf (the reference clamps to >= 16).
        max_threads : accepted for compatibility; the build runs on the GPU.
        boxsize : periodic box size L (every coordinate must be in [0, L]), or None.
        device : HIP device ordinal (-1: the current device).
        """
        super().__init__(points, leafsize, max_threads, boxsize, device)
        self._leafsize = int(leafsize)
        self._n_input = int(np.shape(points)[0])

        if len(kwargs) > 0:
            warnings.warn("Unrecognized keyword arguments: {}".format(kwargs))

    def query(self, points: np.ndarray, k: int = 1, workers: int = 1,
              **kwargs) -> Tuple[np.ndarray, np.ndarray]:
        if len(kwargs) > 0:
            warnings.warn("Unrecognized keyword arguments: {}".format(kwargs))

        points, shape = _flatten(points)
        distances, indices = super().query(points, k, workers)

        if shape is not None:
            distances = distances.reshape(tuple(shape[:-1]) + (k,))
            indices = indices.reshape(tuple(shape[:-1]) + (k,))

        return distances, indices

    def query_ball(self, points: np.ndarray, r: float, return_length: bool = False,
                   return_sorted: bool = True, workers: int = 1, return_csr: bool = False,
                   **kwargs):
        """Points within distance r (d2 <= r*r in float32, the kNN metric).

        return_length=True -> uint32 counts, shape points.shape[:-1].
        return_csr=True -> (offsets uint64 (M + 1,), indices uint32): row i is
        indices[offsets[i]:offsets[i + 1]] (each row sorted on the device
        unless return_sorted=False); no per-row Python work, any M (the call
        streams in batches).
        Otherwise an object array of uint32 index arrays (sorted ascending
        unless return_sorted=False), like scipy's query_ball_point.
        """
        if len(kwargs) > 0:
            warnings.warn("Unrecognized keyword arguments: {}".format(kwargs))
        points, shape = _flatten(points)
        out_shape = tuple(shape[:-1]) if shape is not None else (np.asarray(points).shape[0],)
        if return_length:
            return super().query_ball_count(points, float(r)).reshape(out_shape)
        # rows sorted on the device (NBKD_SORTED), both passes streamed in batches
        off, idx = super().query_ball_csr(points, float(r), bool(return_sorted))
        if return_csr:
            return off, idx
        # scipy's object-array form: one array view per row (the rows
        # themselves are already sorted)
        m = len(off) - 1
        rows = np.empty(m, dtype=object)
        for i, row in enumerate(np.split(idx, off[1:-1].astype(np.int64)) if m else ()):
            rows[i] = row
        return rows.reshape(out_shape)

    def count_neighbors(self, points: np.ndarray, r, cumulative: bool = True,
                        per_point: bool = False):
        """Neighbour counts at many radii in one tree walk (scipy's
        ``count_neighbors(other, r)`` with an array ``r``).

        r : a scalar or a 1-D ascending array of up to 32 radii (each finite
            and >= 0; equal neighbours allowed).  The count at radius r[j] is
            the number of tree points with d2 <= r[j]*r[j] in float32, the
            value ``query_ball(points, r[j], return_length=True)`` gives.
        per_point=False -> uint64 totals over all queries, shape (nr,) (a
            scalar r: a Python int).
        per_point=True -> uint32 counts, shape points.shape[:-1] + (nr,) (a
            scalar r: points.shape[:-1]).
        cumulative=False -> first differences along the radius axis: counts
            per bin (r[j-1], r[j]], the first bin kept as it is.
        """
        scalar = np.ndim(r) == 0
        radii = np.atleast_1d(np.asarray(r, dtype=np.float32))
        if radii.ndim != 1:
            raise ValueError("r must be a scalar or a 1-D array of radii")
        if radii.size == 0:
            raise ValueError("r is empty: at least one radius is needed")
        if radii.size > 32:
            raise ValueError(f"r holds {radii.size} radii: at most 32 per call")
        if not np.all(np.isfinite(radii)) or np.any(radii < 0):
            raise ValueError("every radius must be finite and >= 0")
        if np.any(radii[1:] < radii[:-1]):
            raise ValueError("r must be ascending (non-decreasing)")
        points, shape = _flatten(points)
        out_shape = tuple(shape[:-1]) if shape is not None else (np.asarray(points).shape[0],)
        total, counts = super().query_ball_hist(points, radii, bool(per_point))
        res = counts.reshape(out_shape + (radii.size,)) if per_point else total
        if not cumulative:
            res = np.diff(res, axis=-1, prepend=res.dtype.type(0))
        if scalar:
            return res[..., 0] if per_point else int(res[0])
        return res

    def pair_counts(self, r):
        """Auto pair counts DD(<= r) of the tree's own points, cumulative in r:
        unordered pairs i < j with d2 <= r*r, self pairs removed.  Coincident
        distinct particles (d2 = 0) still count as pairs.  ``r`` as in
        ``count_neighbors``; returns uint64 (nr,) (a scalar r: a Python int)."""
        n = self._n_input
        total = self.count_neighbors(self.points(), r)
        if np.ndim(r) == 0:
            return (total - n) // 2
        return (total - np.uint64(n)) // np.uint64(2)

    def fof(self, linking_length: float, min_members: int = 1, return_sizes: bool = False):
        """Friends-of-friends groups of the tree's own points: two points are
        friends when d2 <= linking_length**2 in float32 (the ``query_ball``
        predicate, periodic on a periodic tree), groups are the connected
        components.

        Returns ``group``, int64 (N,): groups are numbered 0..G-1 by descending
        size, ties by the smaller first member (input row); points of groups
        with fewer than ``min_members`` members get -1.  With
        return_sizes=True also ``sizes``, int64 (G,), the member counts in
        that numbering.  ``fof_labels(b)`` gives the raw (labels, sizes) pair:
        the smallest input row of each point's group and the member count at
        each label.
        """
        labels, sizes = super().fof_labels(float(linking_length))
        heads = np.flatnonzero(sizes >= max(int(min_members), 1))  # ascending labels
        order = np.argsort(-sizes[heads].astype(np.int64), kind="stable")
        heads = heads[order]
        number = np.full(labels.shape[0], -1, np.int64)
        number[heads] = np.arange(heads.shape[0], dtype=np.int64)
        group = number[labels]
        if return_sizes:
            return group, sizes[heads].astype(np.int64)
        return group

    def kth_distance(self, points: np.ndarray, k: int):
        """Distance to the k-th nearest neighbour of each point: column k-1 of
        query(points, k)[0], without materialising the (M, k) rows.  Scaled,
        these are the per-point smoothing radii the rasterizer takes."""
        points, shape = _flatten(points)
        out_shape = tuple(shape[:-1]) if shape is not None else (np.asarray(points).shape[0],)
        return super().query_kth(points, int(k)).reshape(out_shape)

    def density(self, points: np.ndarray, k: Optional[int] = None, r: Optional[float] = None):
        """Local number density at each query point.

        k given: k / (4/3 pi r_k^3) with r_k the k-th neighbour distance.
        r given: count(d <= r) / (4/3 pi r^3).
        """
        if (k is None) == (r is None):
            raise ValueError("give exactly one of k or r")
        if k is not None:
            rk = self.kth_distance(points, k).astype(np.float64)
            return k / (4.0 / 3.0 * math.pi * rk ** 3)
        c = self.query_ball(points, r, return_length=True).astype(np.float64)
        return c / (4.0 / 3.0 * math.pi * float(r) ** 3)

    # ---------------------------------------------------------------- persistence
    def points(self) -> np.ndarray:
        """The (N, 3) float32 points the tree holds, in input order (read back
        from the device copy: the permuted SoA and its index array)."""
        _, x, y, z, idx = self.export()
        n = self._n_input
        out = np.empty((len(idx), 3), np.float32)
        out[idx, 0], out[idx, 1], out[idx, 2] = x, y, z
        return out[:n]

    def _state(self):
        return {"points": self.points(), "leafsize": self._leafsize,
                "boxsize": float(self.boxsize) if self.periodic else None}

    def __reduce__(self):
        st = self._state()
        return (_restore, (st["points"], st["leafsize"], st["boxsize"]))

    def save(self, path) -> None:
        """Write the tree's points and parameters to an .npz file."""
        st = self._state()
        np.savez(path, format_version=np.int64(1), points=st["points"],
                 leafsize=np.int64(st["leafsize"]),
                 boxsize=np.float64(-1.0 if st["boxsize"] is None else st["boxsize"]))

    @classmethod
    def load(cls, path, device: int = -1) -> "KDTree":
        """Rebuild a tree written by ``save`` (on ``device``)."""
        with np.load(path, allow_pickle=False) as f:
            if int(f["format_version"]) != 1:
                raise ValueError(f"unsupported KDTree file version {int(f['format_version'])}")
            box = float(f["boxsize"])
            return cls(f["points"], int(f["leafsize"]), boxsize=None if box < 0 else box,
                       device=device)


def _restore(points, leafsize, boxsize):
    return KDTree(points, leafsize, boxsize=boxsize)
