"""MI355X-native drop-in for ``nbodyhpc.kdtree``.

Mirrors the reference wrapper kdtree/src/python/nbodyhpc/kdtree/__init__.py:11-56
(defaults leafsize=128, max_threads=-1; unknown keyword arguments warn;
N-D query arrays are flattened) on top of the pybind11 module ``_impl``
(mirror of kdtree/src/cpp/pybind.cpp), which drives the HIP kernels through
the C ABI in include/nbkd.h.  There is no CPU fallback: without the built
extension or without a GPU the constructor raises.

Additions (no reference counterpart): ``query_ball`` (scipy-style radius
query, count or index lists), ``count_neighbors`` / ``pair_counts`` (counts at
many radii in one tree walk), ``count_pairs_rppi`` / ``count_pairs_smu`` /
``pair_counts_rppi`` / ``pair_counts_smu`` / ``xi_rppi`` / ``xi_smu``
(anisotropic pair counts about a line of sight in one tree walk, wp(rp) and
the multipoles from them; with ``observer=`` the line of sight of each pair
runs from the observer through the pair's midpoint, for light cones and survey
mocks), ``landy_szalay`` / ``xi_rppi_ls`` / ``xi_smu_ls`` (the same from DD, DR
and RR against a random catalogue), ``fof`` / ``fof_labels`` (friends-of-friends
groups of the tree's points), ``fof_catalog`` (members, mass, centre, extent
and value moments per group, reduced on the GPU), ``density`` (local number density from the k-th
neighbour distance or from a radius count), ``kernel_sum`` / ``sph_density`` /
``interpolate`` (kernel-weighted sums over each query's own ball: the gather
form of SPH), ``profile`` / ``so_mass`` (weighted radial profiles in one tree
walk, spherical-overdensity masses and radii read off them),
``gravity`` / ``potential`` (Barnes-Hut potentials and
accelerations from the tree's points as masses), ``gravity_ewald`` /
``potential_ewald`` (the same on a periodic tree: an Ewald sum over all
images), ``group_potential`` /
``unbind`` (each group member's potential from its own group, the most-bound
member, iterative unbinding), a ``device`` keyword, and
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

__all__ = ["KDTree", "cKDTree", "device_count", "landy_szalay"]

# kernel name -> (NBKD_KERNEL_* code, 3-D normalisation sigma of K(d / h) / h^3
# with support radius h)
_KERNELS = {"tophat": (0, 3.0 / (4.0 * math.pi)), "cubic": (1, 8.0 / math.pi),
            "wendland": (2, 21.0 / (2.0 * math.pi))}
_MAX_VALUES = 4  # NBKD_MAX_VALUES
_MAX_RADII = 32  # NBKD_MAX_RADII
_MAX_LOS_BINS = 64  # NBKD_MAX_LOS_BINS
_HIST2_RPPI, _HIST2_SMU = 0, 1  # NBKD_HIST2_*


def _flatten(points):
    points = np.asarray(points)
    if points.ndim != 2:
        shape = points.shape
        return points.reshape((-1, shape[-1])), shape
    return points, None


def _obs_kw(observer):
    """the ``observer`` keyword of the count methods, left out when None"""
    return {} if observer is None else {"observer": observer}


def _multipoles(xi, u, ells):
    """{ell: (2 ell + 1) sum_l xi P_ell(mu_mid) dmu} of xi (ns, nmu) on the mu
    edges u (nmu + 1,), float64"""
    dmu = u[1:] - u[:-1]
    mid = 0.5 * (u[1:] + u[:-1])
    poles = {}
    for ell in ells:
        c = np.zeros(int(ell) + 1)
        c[int(ell)] = 1.0
        leg = np.polynomial.legendre.legval(mid, c)
        poles[int(ell)] = (2 * int(ell) + 1) * (xi * (leg * dmu)[None, :]).sum(axis=1)
    return poles


def _geometric(lo, hi, n):
    """n float32 edges from lo to hi in equal ratios, ascending (the two ends
    exact: the float32 values of lo and hi)"""
    g = np.exp(np.linspace(math.log(lo), math.log(hi), n)).astype(np.float32)
    g[0], g[-1] = np.float32(lo), np.float32(hi)
    return np.maximum.accumulate(g)


def landy_szalay(dd, dr, rr, nd, nr):
    """The Landy-Szalay estimator per bin, in float64:
    ``(DD / (nd (nd - 1)) - 2 DR / (nd nr) + RR / (nr (nr - 1))) / (RR / (nr (nr - 1)))``,
    NaN where ``rr == 0``.

    dd, rr : ordered pair counts of the nd data points and of the nr random
        points among themselves, self pairs removed (both orders of a pair
        counted, as ``count_pairs_rppi`` / ``count_pairs_smu`` count them).
    dr : the counts of the data as queries against the randoms' tree.
    """
    dd = np.asarray(dd, dtype=np.float64)
    dr = np.asarray(dr, dtype=np.float64)
    rr = np.asarray(rr, dtype=np.float64)
    nd, nr = float(nd), float(nr)
    with np.errstate(divide="ignore", invalid="ignore"):
        rrn = rr / (nr * (nr - 1.0))
        xi = (dd / (nd * (nd - 1.0)) - 2.0 * dr / (nd * nr) + rrn) / rrn
    return np.where(rr == 0, np.nan, xi)


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

        The threshold is min(fl(r*r), FLT_MAX): a negative r acts as |r|,
        r = NaN matches nothing, and r = inf (or any r whose square overflows)
        returns every point at a finite distance, never a padding point.  A
        query with a NaN coordinate, or so far away that every d2 overflows,
        gets an empty row (count 0).

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
            value ``query_ball(points, r[j], return_length=True)`` gives
            (threshold min(fl(r[j]*r[j]), FLT_MAX): a square that overflows
            counts every point at a finite distance; a query with a NaN
            coordinate or with every d2 = inf counts nothing).
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

    @staticmethod
    def _edges(e, name, nmax, mu=False):
        """the float32 edges of one axis of the anisotropic counts, checked"""
        e = np.asarray(e, dtype=np.float32)
        if e.ndim != 1:
            raise ValueError(f"{name} must be a 1-D array of edges")
        if e.size == 0:
            raise ValueError(f"{name} is empty: at least one edge is needed")
        if e.size > nmax:
            raise ValueError(f"{name} holds {e.size} edges: at most {nmax} per call")
        if not np.all(np.isfinite(e)) or np.any(e < 0):
            raise ValueError(f"every edge of {name} must be finite and >= 0")
        if mu and np.any(e > 1):
            raise ValueError(f"every edge of {name} must be <= 1")
        if np.any(e[1:] < e[:-1]):
            raise ValueError(f"{name} must be ascending (non-decreasing)")
        return np.ascontiguousarray(e)

    def _observer(self, observer, los):
        """the float32 observer of the pairwise line of sight, checked"""
        if los != 2:
            raise ValueError("give los or observer, not both")
        if self.periodic:
            raise ValueError("observer needs a non-periodic tree: pairwise lines of sight are "
                             "not defined on a periodic one (los takes an axis there)")
        try:
            o = np.asarray(observer, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("observer must be 3 finite coordinates") from None
        with np.errstate(over="ignore"):
            o32 = o.astype(np.float32)
        if o.shape != (3,) or not np.all(np.isfinite(o32)):
            raise ValueError(f"observer must be 3 finite coordinates, got {observer!r}")
        return np.ascontiguousarray(o32)

    def _count_pairs2(self, points, e1, e2, mode, los, names, observer=None):
        e1 = self._edges(e1, names[0], _MAX_RADII)
        e2 = self._edges(e2, names[1], _MAX_LOS_BINS, mu=mode == _HIST2_SMU)
        if los not in (0, 1, 2):
            raise ValueError("los must be 0, 1 or 2 (the axis of the line of sight)")
        if observer is not None:
            o = self._observer(observer, los)
            points, _ = _flatten(points)
            return super().query_ball_hist2_obs(points, e1, e2, mode, o)
        points, _ = _flatten(points)
        return super().query_ball_hist2(points, e1, e2, mode, int(los))

    def count_pairs_rppi(self, points: np.ndarray, rp, pi, los: int = 2, observer=None):
        """Pair counts of ``points`` against the tree's points in (rp, pi) bins,
        one tree walk: uint64 (len(rp), len(pi)).  rp (up to 32) and pi (up to
        64) are ascending edges, each finite and >= 0; ``los`` is the axis of the
        line of sight.  With a = the per-axis squared separations (float32,
        minimum image on a periodic tree), pi2 = a[los], rp2 = the sum of the
        other two, a pair falls into bin (#{k: rp2 > rp[k]^2}, #{l: pi2 >
        pi[l]^2}) and is dropped when either index runs past the last edge: bins
        are differential on both axes, bin 0 reaches from 0 to the first edge.
        Cross counts D1D2, DR and RR come from passing the other catalogue.

        observer : None, or 3 finite coordinates (non-periodic trees only, and
            instead of ``los``): the line of sight of each pair then runs from
            the observer through the pair's midpoint.  With s = p - q and l =
            (p - o) + (q - o), pi2 = min((s . l)^2 / |l|^2, s2) (0 where l = 0)
            and rp2 = s2 - pi2, all in float32 (include/nbkd.h,
            nbkd_query_ball_hist2_obs)."""
        return self._count_pairs2(points, rp, pi, _HIST2_RPPI, los, ("rp", "pi"), observer)

    def count_pairs_smu(self, points: np.ndarray, s, mu, los: int = 2, observer=None):
        """Pair counts of ``points`` against the tree's points in (s, mu) bins,
        one tree walk: uint64 (len(s), len(mu)).  s (up to 32 edges) bins the
        tree's own distance (s2 = d2 of ``count_neighbors``), mu (up to 64 edges
        in [0, 1]) bins |pi| / s through pi2 <= fl(mu[l]^2 * s2).  With a last mu
        edge of 1 every pair within s[-1] is counted, and the sum over mu equals
        ``count_neighbors(points, s, cumulative=False)``.  ``observer`` as in
        ``count_pairs_rppi``: pi2 is then taken along the line from the observer
        through the pair's midpoint."""
        return self._count_pairs2(points, s, mu, _HIST2_SMU, los, ("s", "mu"), observer)

    def _auto2(self, counts):
        """ordered counts of the tree's own points -> unordered pairs: the n
        self pairs leave bin (0, 0), every bin is halved"""
        counts = counts.copy()
        counts[0, 0] -= np.uint64(self._n_input)
        return counts // np.uint64(2)

    def pair_counts_rppi(self, rp, pi, los: int = 2, observer=None):
        """Auto pair counts DD(rp, pi) of the tree's own points: unordered pairs
        i < j per bin (``count_pairs_rppi``'s bins), self pairs removed."""
        return self._auto2(self.count_pairs_rppi(self.points(), rp, pi, los, **_obs_kw(observer)))

    def pair_counts_smu(self, s, mu, los: int = 2, observer=None):
        """Auto pair counts DD(s, mu) of the tree's own points: unordered pairs
        i < j per bin (``count_pairs_smu``'s bins), self pairs removed."""
        return self._auto2(self.count_pairs_smu(self.points(), s, mu, los, **_obs_kw(observer)))

    def _xi_args(self, edges, name, nsec, nsec_name):
        if not self.periodic:
            raise ValueError("the natural estimator with analytic RR needs a periodic tree")
        return self._xi_edges(edges, name, nsec, nsec_name)

    def _xi_edges(self, edges, name, nsec, nsec_name):
        e = self._edges(edges, name, _MAX_RADII)
        if e.size < 2:
            raise ValueError(f"{name} needs at least two edges (one bin)")
        if np.any(e[1:] <= e[:-1]):
            raise ValueError(f"{name} must be strictly ascending")
        if int(nsec) != nsec or not 1 <= nsec <= _MAX_LOS_BINS:
            raise ValueError(f"{nsec_name} must be an integer in [1, {_MAX_LOS_BINS}]")
        return e, int(nsec)

    def xi_rppi(self, rp_edges, pi_max: float, npi: int, los: int = 2):
        """xi(rp, pi) and wp(rp) of the tree's own points on a periodic tree:
        the natural estimator DD / RR - 1 with analytic RR, in float64.

        rp_edges : n strictly ascending edges (n - 1 bins; what lies inside the
            first edge, the self pairs among it, is dropped); rp_edges[-1] <= L/2.
        pi_max, npi : npi equal bins of |pi| up to pi_max <= L/2 (edges
            pi_max (l + 1) / npi, rounded to float32).
        Returns (xi (n - 1, npi), wp (n - 1,)), wp = 2 sum_l xi dpi.  RR per
        ordered pair is N (N / L^3) pi (rp_hi^2 - rp_lo^2) 2 (pi_hi - pi_lo), with
        the float32 edges the counts used."""
        e, npi = self._xi_args(rp_edges, "rp_edges", npi, "npi")
        L = float(self.boxsize)
        if not (math.isfinite(pi_max) and pi_max > 0):
            raise ValueError("pi_max must be finite and > 0")
        if float(e[-1]) > 0.5 * L or pi_max > 0.5 * L:
            raise ValueError("rp_edges[-1] and pi_max must not exceed half the box")
        pe = (float(pi_max) * (np.arange(npi, dtype=np.float64) + 1.0) / npi).astype(np.float32)
        dd = self.count_pairs_rppi(self.points(), e, pe, los)[1:].astype(np.float64)
        n = float(self._n_input)
        r = e.astype(np.float64)
        p = np.concatenate([[0.0], pe.astype(np.float64)])
        vol = math.pi * (r[1:] ** 2 - r[:-1] ** 2)[:, None] * 2.0 * (p[1:] - p[:-1])[None, :]
        xi = dd / (n * (n / L ** 3) * vol) - 1.0
        wp = 2.0 * (xi * (p[1:] - p[:-1])[None, :]).sum(axis=1)
        return xi, wp

    def xi_smu(self, s_edges, nmu: int, ells=(0, 2, 4), los: int = 2):
        """xi(s, mu) and its multipoles of the tree's own points on a periodic
        tree: the natural estimator DD / RR - 1 with analytic RR, in float64.

        s_edges : n strictly ascending edges (n - 1 bins; what lies inside the
            first edge is dropped); s_edges[-1] <= L/2.
        nmu : equal bins of mu in [0, 1] (edges (l + 1) / nmu, rounded to float32).
        Returns (xi (n - 1, nmu), multipoles {ell: (n - 1,)}), xi_ell(s) =
        (2 ell + 1) sum_l xi P_ell(mu_mid) dmu.  RR per ordered pair is
        N (N / L^3) (4 pi / 3) (s_hi^3 - s_lo^3) (mu_hi - mu_lo)."""
        e, nmu = self._xi_args(s_edges, "s_edges", nmu, "nmu")
        L = float(self.boxsize)
        if float(e[-1]) > 0.5 * L:
            raise ValueError("s_edges[-1] must not exceed half the box")
        me = ((np.arange(nmu, dtype=np.float64) + 1.0) / nmu).astype(np.float32)
        dd = self.count_pairs_smu(self.points(), e, me, los)[1:].astype(np.float64)
        n = float(self._n_input)
        r = e.astype(np.float64)
        u = np.concatenate([[0.0], me.astype(np.float64)])
        dmu = u[1:] - u[:-1]
        vol = (4.0 * math.pi / 3.0) * (r[1:] ** 3 - r[:-1] ** 3)[:, None] * dmu[None, :]
        xi = dd / (n * (n / L ** 3) * vol) - 1.0
        return xi, _multipoles(xi, u, ells)

    def _ls_randoms(self, randoms):
        if not isinstance(randoms, KDTree):
            raise ValueError("randoms must be a KDTree of the random catalogue")
        if bool(randoms.periodic) != bool(self.periodic) or (
                self.periodic and float(randoms.boxsize) != float(self.boxsize)):
            raise ValueError("randoms must have the tree's periodicity and box size")

    def _ls_counts(self, randoms, count, e1, e2, los, observer):
        """(DD, DR, RR) of ``count`` ("count_pairs_rppi" / "count_pairs_smu"),
        ordered, without the first row (what lies inside the first edge, the
        self pairs among it)"""
        kw = _obs_kw(observer)
        data = self.points()
        dd = getattr(self, count)(data, e1, e2, los, **kw)[1:]
        dr = getattr(randoms, count)(data, e1, e2, los, **kw)[1:]
        rr = getattr(randoms, count)(randoms.points(), e1, e2, los, **kw)[1:]
        return dd, dr, rr

    def xi_rppi_ls(self, randoms, rp_edges, pi_max: float, npi: int, los: int = 2,
                   observer=None):
        """xi(rp, pi) and wp(rp) of the tree's points by the Landy-Szalay
        estimator against a random catalogue, in float64: ``landy_szalay`` of
        DD, DR and RR, three tree walks.

        randoms : the KDTree of the random catalogue (same periodicity and box).
        rp_edges, pi_max, npi : the bins of ``xi_rppi`` (what lies inside the
            first rp edge is dropped; pi edges pi_max (l + 1) / npi rounded to
            float32; on a periodic tree neither may pass half the box).
        los, observer : as in ``count_pairs_rppi``; with an observer (a
            non-periodic tree) each pair's line of sight runs through its
            midpoint, the geometry of a light cone or a survey mock.
        Returns (xi (n - 1, npi), wp (n - 1,)), wp = 2 sum_l xi dpi; NaN where
        RR is 0."""
        self._ls_randoms(randoms)
        e, npi = self._xi_edges(rp_edges, "rp_edges", npi, "npi")
        if not (math.isfinite(pi_max) and pi_max > 0):
            raise ValueError("pi_max must be finite and > 0")
        if self.periodic and (float(e[-1]) > 0.5 * float(self.boxsize)
                              or pi_max > 0.5 * float(self.boxsize)):
            raise ValueError("rp_edges[-1] and pi_max must not exceed half the box")
        pe = (float(pi_max) * (np.arange(npi, dtype=np.float64) + 1.0) / npi).astype(np.float32)
        dd, dr, rr = self._ls_counts(randoms, "count_pairs_rppi", e, pe, los, observer)
        xi = landy_szalay(dd, dr, rr, self._n_input, randoms._n_input)
        p = np.concatenate([[0.0], pe.astype(np.float64)])
        wp = 2.0 * (xi * (p[1:] - p[:-1])[None, :]).sum(axis=1)
        return xi, wp

    def xi_smu_ls(self, randoms, s_edges, nmu: int, ells=(0, 2, 4), los: int = 2,
                  observer=None):
        """xi(s, mu) and its multipoles of the tree's points by the
        Landy-Szalay estimator against a random catalogue, in float64.

        randoms, los, observer : as in ``xi_rppi_ls``.
        s_edges, nmu, ells : the bins and multipoles of ``xi_smu`` (mu edges
            (l + 1) / nmu rounded to float32; xi_ell(s) = (2 ell + 1) sum_l xi
            P_ell(mu_mid) dmu).
        Returns (xi (n - 1, nmu), multipoles {ell: (n - 1,)}); NaN where RR is
        0."""
        self._ls_randoms(randoms)
        e, nmu = self._xi_edges(s_edges, "s_edges", nmu, "nmu")
        if self.periodic and float(e[-1]) > 0.5 * float(self.boxsize):
            raise ValueError("s_edges[-1] must not exceed half the box")
        me = ((np.arange(nmu, dtype=np.float64) + 1.0) / nmu).astype(np.float32)
        dd, dr, rr = self._ls_counts(randoms, "count_pairs_smu", e, me, los, observer)
        xi = landy_szalay(dd, dr, rr, self._n_input, randoms._n_input)
        u = np.concatenate([[0.0], me.astype(np.float64)])
        return xi, _multipoles(xi, u, ells)

    def fof(self, linking_length: float, min_members: int = 1, return_sizes: bool = False):
        """Friends-of-friends groups of the tree's own points: two points are
        friends when d2 <= linking_length**2 in float32 (the ``query_ball``
        predicate, periodic on a periodic tree), groups are the connected
        components.  The linking length must be finite and >= 0; one whose
        square overflows in float32 (threshold min(fl(b*b), FLT_MAX)) links
        every point into one group.

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

    def fof_catalog(self, linking_length: Optional[float], min_members: int = 20, mass=None,
                    values=None, members: bool = False, labels=None):
        """The group catalogue of the friends-of-friends groups (or of any
        canonical labelling given as ``labels``: labels[i] = the smallest
        input row of i's group; ``linking_length`` may then be None), reduced
        on the GPU in float64 with a fixed summation order.

        mass : (N,) weights or None (unit masses).
        values : (N,) or (N, nv <= 4) per-particle channels (velocities, ...).

        Groups with at least ``min_members`` members are numbered exactly as
        ``fof(linking_length, min_members)`` numbers them: descending size,
        ties by the smaller head.  Returns a dict of arrays over the groups:
        ``head`` (smallest member row), ``size``, ``mass`` (sum of weights),
        ``center`` float64 (G, 3) (wrapped into [0, L) on a periodic tree, L
        the tree's float32 box, and still below L after a cast to float32, so
        that it is a legal query of this tree: a coordinate within half a
        float32 step below L is returned as 0, the same place; offsets are
        unwrapped relative to the head), ``rms_radius``, ``mean``
        and ``dispersion`` (G, nv) of the value channels, ``spans_box`` (bool:
        a member lies L/2 or more from the head along an axis, so the
        unwrapped centre is not trustworthy; all False on a non-periodic
        tree), and with members=True ``offsets`` (G + 1,) and ``members``:
        members[offsets[g]:offsets[g + 1]] = the rows of group g, ascending.
        """
        n = self._n_input
        if labels is None and linking_length is None:
            raise ValueError("give labels or a linking_length")
        w = None
        if mass is not None:
            w = np.asarray(mass, dtype=np.float32)
            if w.shape != (n,):
                raise ValueError(f"mass must be (N,) with N = {n} the tree's point count")
        v, nv = None, 0
        if values is not None:
            v = np.asarray(values, dtype=np.float32)
            if v.ndim not in (1, 2) or v.shape[0] != n:
                raise ValueError(f"values must be (N,) or (N, nv) with N = {n} the tree's point "
                                 f"count, got {v.shape}")
            v = np.ascontiguousarray(v.reshape(n, -1))
            nv = v.shape[1]
            if not 1 <= nv <= _MAX_VALUES:
                raise ValueError(f"values holds {nv} channels: 1 to {_MAX_VALUES} per call")
        if labels is not None:
            lab = np.asarray(labels)
            if lab.shape != (n,):
                raise ValueError(f"labels must be (N,) with N = {n} the tree's point count")
            lab = np.ascontiguousarray(lab, dtype=np.uint32)
        else:
            lab, _ = super().fof_labels(float(linking_length))
        head, size, off, mem, mom, dmax = super().group_moments(
            lab, max(int(min_members), 1), w, v, bool(members))
        # fof()'s numbering: descending size, ties by the smaller head (the
        # device's order is ascending heads, the sort is stable)
        order = np.argsort(-size.astype(np.int64), kind="stable")
        head, size, mom, dmax = head[order], size[order], mom[order], dmax[order]
        with np.errstate(divide="ignore", invalid="ignore"):
            m0 = mom[:, 0]
            dbar = mom[:, 1:4] / m0[:, None]
            center = self.points()[head].astype(np.float64) + dbar
            rms = np.sqrt(np.maximum(mom[:, 4] / m0 - np.sum(dbar * dbar, axis=1), 0.0))
            mean = mom[:, 5:5 + nv] / m0[:, None]
            disp = np.sqrt(np.maximum(mom[:, 5 + nv:5 + 2 * nv] / m0[:, None] - mean * mean, 0.0))
        if self.periodic:
            L = float(self.boxsize)
            center = center % L
            # a tiny negative wraps to L in float64, and a centre within half a
            # float32 step below L becomes L once cast: both are the place 0
            center[center.astype(np.float32) >= np.float32(L)] = 0.0
            spans = dmax >= np.float32(0.5) * np.float32(self.boxsize)
        else:
            spans = np.zeros(head.shape[0], bool)
        cat = {"head": head, "size": size, "mass": m0.copy(), "center": center,
               "rms_radius": rms, "mean": mean, "dispersion": disp, "spans_box": spans}
        if members:
            cnt = np.diff(off.astype(np.int64))[order]
            new_off = np.zeros(head.shape[0] + 1, np.int64)
            np.cumsum(cnt, out=new_off[1:])
            # gather each group's rows into its new place
            src = np.repeat(off[:-1].astype(np.int64)[order] - new_off[:-1], cnt)
            cat["offsets"] = new_off.astype(np.uint64)
            cat["members"] = mem[src + np.arange(mem.shape[0], dtype=np.int64)]
        return cat

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

    # ---------------------------------------------------------------- kernel sums
    def _sum_args(self, points, h, values, kernel):
        """Checked arguments of a kernel sum: (flat float32 points, output
        shape, float32 radii (M,), float32 values (N, nv) or None, whether
        values was 1-D or absent, kernel code).  Runs before any device call."""
        if kernel not in _KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}: one of {sorted(_KERNELS)}")
        points, shape = _flatten(points)
        m = np.asarray(points).shape[0]
        out_shape = tuple(shape[:-1]) if shape is not None else (m,)
        hh = np.asarray(h, dtype=np.float64)
        if not np.all(np.isfinite(hh)) or np.any(hh < 0):
            raise ValueError("every radius h must be finite and >= 0")
        try:
            hh = np.broadcast_to(hh, out_shape).reshape(-1)
        except ValueError:
            raise ValueError(f"h of shape {np.shape(h)} does not broadcast to the queries "
                             f"{out_shape}") from None
        vals, flat = None, True
        if values is not None:
            vals = np.asarray(values, dtype=np.float32)
            if vals.ndim not in (1, 2) or vals.shape[0] != self._n_input:
                raise ValueError(f"values must be (N,) or (N, nv) with N = {self._n_input} "
                                 f"the tree's point count, got {vals.shape}")
            flat = vals.ndim == 1
            if not flat and not 1 <= vals.shape[1] <= _MAX_VALUES:
                raise ValueError(f"values holds {vals.shape[1]} channels: 1 to {_MAX_VALUES} "
                                 "per call")
            vals = np.ascontiguousarray(vals.reshape(self._n_input, -1))
        return (points, out_shape, np.ascontiguousarray(hh, dtype=np.float32), vals, flat,
                _KERNELS[kernel][0])

    def kernel_sum(self, points: np.ndarray, h, values=None, kernel: str = "cubic",
                   return_count: bool = False):
        """Kernel-weighted sums over each query's own ball, summed on the GPU:
        ``sum_j values[j] * K(d_ij / h_i)`` over the tree points with
        d2 <= h_i*h_i in float32 (the ``query_ball`` predicate at r = h_i).

        h : a scalar or an array broadcast to the queries, finite and >= 0.
        values : None (weight 1), (N,) or (N, nv <= 4), indexed like the
            tree's input points.
        kernel : "tophat" (K = 1), "cubic" (the M4 spline
            1 - 6u^2 + 6u^3 | 2(1 - u)^3) or "wendland" ((1 - u)^4 (1 + 4u)).

        Returns the raw (un-normalised) sums as float64, shape
        points.shape[:-1] (+ (nv,) for 2-D values); with return_count=True
        also the uint32 neighbour counts.  The device sums in float32, one
        accumulator per (query, channel) in a fixed order: identical calls
        give identical arrays.
        """
        points, out_shape, hh, vals, flat, code = self._sum_args(points, h, values, kernel)
        sums, counts = super().ball_sum(points, hh, vals, code, bool(return_count))
        sums = sums.astype(np.float64).reshape(out_shape if flat else out_shape + (sums.shape[1],))
        if return_count:
            return sums, counts.reshape(out_shape)
        return sums

    def sph_density(self, points: Optional[np.ndarray] = None, k: int = 32, mass=None,
                    kernel: str = "cubic", h=None):
        """SPH (gather) density ``sigma / h_i^3 * sum_j m_j K(d_ij / h_i)``
        with sigma = 3/(4 pi), 8/pi, 21/(2 pi) for "tophat", "cubic" and
        "wendland".  points=None: at the tree's own points.  h: the smoothing
        lengths, or None for the k-th neighbour distance.  mass: (N,) or None
        (unit masses: a number density).  float64; inf or NaN where h is 0."""
        if kernel not in _KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}: one of {sorted(_KERNELS)}")
        if mass is not None and (np.ndim(mass) != 1 or np.shape(mass)[0] != self._n_input):
            raise ValueError(f"mass must be (N,) with N = {self._n_input} the tree's point count")
        if h is not None:
            hh = np.asarray(h, dtype=np.float64)
            if not np.all(np.isfinite(hh)) or np.any(hh < 0):
                raise ValueError("every radius h must be finite and >= 0")
        if points is None:
            points = self.points()
        if h is None:
            h = self.kth_distance(points, int(k))
        s = self.kernel_sum(points, h, mass, kernel)
        h64 = np.broadcast_to(np.asarray(h, dtype=np.float32).astype(np.float64), s.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _KERNELS[kernel][1] * s / h64 ** 3

    def interpolate(self, points: np.ndarray, h, field, mass=None, kernel: str = "cubic"):
        """SPH interpolation of a per-particle field at arbitrary points:
        ``sum_j m_j A_j K / sum_j m_j K`` over each query's ball of radius
        h_i, in one device call (channels m*A_1..m*A_c, m).  field: (N,) or
        (N, c <= 3); mass: (N,) or None (unit masses).  float64, shape
        points.shape[:-1] (+ (c,)); NaN where the ball is empty."""
        if kernel not in _KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}: one of {sorted(_KERNELS)}")
        f = np.asarray(field, dtype=np.float64)
        if f.ndim not in (1, 2) or f.shape[0] != self._n_input:
            raise ValueError(f"field must be (N,) or (N, c) with N = {self._n_input} the tree's "
                             f"point count, got {f.shape}")
        if f.ndim == 2 and not 1 <= f.shape[1] <= _MAX_VALUES - 1:
            raise ValueError(f"field holds {f.shape[1]} channels: 1 to {_MAX_VALUES - 1} per call")
        if mass is None:
            w = np.ones(self._n_input, np.float64)
        else:
            w = np.asarray(mass, dtype=np.float64)
            if w.ndim != 1 or w.shape[0] != self._n_input:
                raise ValueError(f"mass must be (N,) with N = {self._n_input} the tree's point "
                                 "count")
        vals = np.concatenate([f.reshape(self._n_input, -1) * w[:, None], w[:, None]], axis=1)
        s = self.kernel_sum(points, h, vals.astype(np.float32), kernel)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = s[..., :-1] / s[..., -1:]
        return out[..., 0] if f.ndim == 1 else out

    # ---------------------------------------------------------------- radial profiles
    def _profile_args(self, points, radii, values, scale):
        """Checked arguments of a profile: (flat float32 points, output shape,
        float32 radii (nr,), float32 values (N, nv) or None, whether values was
        1-D or absent, float32 scale (M,) or None).  Runs before any device
        call."""
        r = np.asarray(radii, dtype=np.float32)
        if r.ndim != 1:
            raise ValueError("radii must be a 1-D array")
        if r.size == 0:
            raise ValueError("radii is empty: at least one radius is needed")
        if r.size > _MAX_RADII:
            raise ValueError(f"radii holds {r.size} radii: at most {_MAX_RADII} per call")
        if not np.all(np.isfinite(r)) or np.any(r < 0):
            raise ValueError("every radius must be finite and >= 0")
        if np.any(r[1:] < r[:-1]):
            raise ValueError("radii must be ascending (non-decreasing)")
        points, shape = _flatten(points)
        m = np.asarray(points).shape[0]
        out_shape = tuple(shape[:-1]) if shape is not None else (m,)
        sc = None
        if scale is not None:
            sc = np.asarray(scale, dtype=np.float64)
            if not np.all(np.isfinite(sc)) or np.any(sc < 0):
                raise ValueError("every scale must be finite and >= 0")
            try:
                sc = np.broadcast_to(sc, out_shape).reshape(-1)
            except ValueError:
                raise ValueError(f"scale of shape {np.shape(scale)} does not broadcast to the "
                                 f"queries {out_shape}") from None
            sc = np.ascontiguousarray(sc, dtype=np.float32)
        vals, flat = None, True
        if values is not None:
            vals = np.asarray(values, dtype=np.float32)
            if vals.ndim not in (1, 2) or vals.shape[0] != self._n_input:
                raise ValueError(f"values must be (N,) or (N, nv) with N = {self._n_input} "
                                 f"the tree's point count, got {vals.shape}")
            flat = vals.ndim == 1
            if not flat and not 1 <= vals.shape[1] <= _MAX_VALUES:
                raise ValueError(f"values holds {vals.shape[1]} channels: 1 to {_MAX_VALUES} "
                                 "per call")
            vals = np.ascontiguousarray(vals.reshape(self._n_input, -1))
        return points, out_shape, np.ascontiguousarray(r), vals, flat, sc

    def profile(self, points: np.ndarray, radii, values=None, scale=None,
                cumulative: bool = False):
        """Weighted radial profiles around each query in one tree walk: the
        sum of ``values`` over the tree points in each of the nr shells.

        radii : 1-D ascending array of up to 32 shell edges (each finite and
            >= 0; equal neighbours give an empty bin).
        scale : None, or a scalar or array broadcast to the queries, finite and
            >= 0: query i's edges are ``radii[k] * scale[i]`` (formed in
            float32), so profiles come in units of each halo's own radius.
        values : None (weight 1: counts), (N,) or (N, nv <= 4), indexed like the
            tree's input points.

        A point falls into bin b = the number of edges k with
        ``not d2 <= fl(e_k * e_k)`` in float32 (the ``query_ball`` predicate):
        bin 0 is the ball of the first edge, bin k the shell (e_{k-1}, e_k],
        points beyond the last edge are dropped.  Returns the raw per-bin sums,
        float32, shape points.shape[:-1] + (nr,) (+ (nv,) for 2-D values); with
        cumulative=True their float64 running sum over the bins, the enclosed
        sums M(<= e_k).  The device sums in float32, one accumulator per (query,
        bin, channel) in a fixed order: identical calls give identical arrays.

        After ``fof_catalog`` / ``group_potential`` the centres are the
        catalogue's ``center`` rows or the most-bound members
        (``points()[most_bound]``), and ``scale`` a radius per halo (for
        instance ``so_mass(...)["radius"]``) for stacked profiles.
        """
        points, out_shape, r, vals, flat, sc = self._profile_args(points, radii, values, scale)
        sums = super().ball_profile(points, r, vals, sc)
        sums = sums.reshape(out_shape + ((r.size,) if flat else (r.size, sums.shape[2])))
        if cumulative:
            return np.cumsum(sums.astype(np.float64), axis=len(out_shape))
        return sums

    def so_mass(self, centres: np.ndarray, overdensity, r_max: float, mass=None,
                r_min: Optional[float] = None, nbins: int = 32, refine: int = 1):
        """Spherical-overdensity masses and radii (M200c / R200c and the like)
        around each centre, from ``profile``.

        overdensity : the threshold mean density (mass per volume in the
            tree's units, for instance 200 times the critical density), a
            scalar or one value per centre.
        r_max, r_min : the search range; r_min defaults to r_max / 1000.
        mass : (N,) particle masses or None (unit masses).
        nbins : edges per pass (2 to 32); refine : further passes.

        The first pass takes ``nbins`` geometric edges e_k from r_min to r_max,
        M_k = the float64 running sum of the bins and the enclosed mean density
        rho_k = M_k / (4/3 pi e_k^3) (float64, from the float32 edges).  k* is
        the smallest k with rho_k < overdensity: status 1 if k* == 0 (already
        below at r_min), status 2 if there is none (no crossing within r_max),
        otherwise the crossing lies in the bracket [e_{k*-1}, e_{k*}].  Each
        further pass profiles the bracket alone, in units of its lower edge
        (``scale`` = r_lo: bin 0 recounts M(<= r_lo)), with ``nbins`` geometric
        edges from 1 to the previous edge ratio times (1 + 2^-20), and narrows
        the bracket the same way; a pass that does not bracket a crossing
        leaves the earlier bracket.

        Returns a dict of arrays over the centres: ``radius`` (the log-log
        interpolation of the mean density inside the bracket), ``mass`` =
        overdensity * 4/3 pi radius^3, the bracket ``r_lo``, ``r_hi`` (float32
        edges) with the enclosed masses ``m_lo``, ``m_hi`` (float64), and
        ``status`` (0: found).  radius and mass are NaN where status != 0.
        Works on periodic and non-periodic trees (keep r_max below half the
        box).

        After ``fof_catalog`` the centres are ``cat["center"]``; after
        ``group_potential`` / ``unbind`` the most-bound members,
        ``points()[most_bound]``.
        """
        nbins, refine = int(nbins), int(refine)
        if not 2 <= nbins <= _MAX_RADII:
            raise ValueError(f"nbins must be in [2, {_MAX_RADII}], got {nbins}")
        if refine < 0:
            raise ValueError(f"refine must be >= 0, got {refine}")
        r_max = float(r_max)
        r_min = r_max / 1000.0 if r_min is None else float(r_min)
        if not (math.isfinite(r_max) and math.isfinite(r_min) and 0.0 < r_min < r_max):
            raise ValueError("r_min and r_max must be finite with 0 < r_min < r_max")
        centres, shape = _flatten(centres)
        centres = np.asarray(centres)
        if centres.ndim != 2 or centres.shape[1] != 3:
            raise ValueError("centres must be an array of shape (..., 3)")
        m = centres.shape[0]
        out_shape = tuple(shape[:-1]) if shape is not None else (m,)
        delta = np.asarray(overdensity, dtype=np.float64)
        if not np.all(np.isfinite(delta)) or np.any(delta <= 0):
            raise ValueError("overdensity must be finite and > 0")
        try:
            delta = np.broadcast_to(delta, out_shape).reshape(-1)
        except ValueError:
            raise ValueError(f"overdensity of shape {np.shape(overdensity)} does not broadcast "
                             f"to the centres {out_shape}") from None
        if mass is not None and (np.ndim(mass) != 1 or np.shape(mass)[0] != self._n_input):
            raise ValueError(f"mass must be (N,) with N = {self._n_input} the tree's point count")
        vol = 4.0 / 3.0 * math.pi

        def crossing(edges, cum, thresh):
            """per row the smallest k with rho_k < thresh, or -1"""
            with np.errstate(divide="ignore", invalid="ignore"):
                rho = cum / (vol * edges.astype(np.float64) ** 3)
            below = rho < thresh[:, None]
            return np.where(below.any(axis=1), below.argmax(axis=1), -1)

        # pass 1: shared edges
        grid = _geometric(r_min, r_max, nbins)
        cum = np.asarray(self.profile(centres, grid, mass, None, True), np.float64).reshape(m, nbins)
        k = crossing(np.broadcast_to(grid, (m, nbins)), cum, delta)
        status = np.where(k == 0, 1, np.where(k < 0, 2, 0)).astype(np.int32)
        good = np.flatnonzero(status == 0)
        r_lo = np.full(m, np.nan, np.float32)
        r_hi = np.full(m, np.nan, np.float32)
        m_lo = np.full(m, np.nan)
        m_hi = np.full(m, np.nan)
        r_lo[good], r_hi[good] = grid[k[good] - 1], grid[k[good]]
        m_lo[good], m_hi[good] = cum[good, k[good] - 1], cum[good, k[good]]
        ratio = float(np.max(grid[1:].astype(np.float64) / grid[:-1].astype(np.float64)))
        for _ in range(refine):
            if good.size == 0:
                break
            grid = _geometric(1.0, ratio * (1.0 + 2.0 ** -20), nbins)
            s = r_lo[good]
            cum = np.asarray(self.profile(centres[good], grid, mass, s, True),
                             np.float64).reshape(good.size, nbins)
            edges = grid[None, :] * s[:, None]  # float32 products, the device's edges
            k = crossing(edges, cum, delta[good])
            hit = np.flatnonzero(k > 0)
            g = good[hit]
            r_lo[g], r_hi[g] = edges[hit, k[hit] - 1], edges[hit, k[hit]]
            m_lo[g], m_hi[g] = cum[hit, k[hit] - 1], cum[hit, k[hit]]
            ratio = float(np.max(grid[1:].astype(np.float64) / grid[:-1].astype(np.float64)))
        # log-log interpolation of the mean density inside the bracket
        lo64, hi64 = r_lo.astype(np.float64), r_hi.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho_lo, rho_hi = m_lo / (vol * lo64 ** 3), m_hi / (vol * hi64 ** 3)
            f = np.log(rho_lo / delta) / np.log(rho_lo / rho_hi)
            radius = np.clip(lo64 * (hi64 / lo64) ** f, lo64, hi64)
        radius = np.where(status == 0, radius, np.nan)
        res = {"radius": radius, "mass": delta * vol * radius ** 3, "r_lo": r_lo, "r_hi": r_hi,
               "m_lo": m_lo, "m_hi": m_hi, "status": status}
        return {name: a.reshape(out_shape) for name, a in res.items()}

    # ---------------------------------------------------------------- gravity
    def _gravity_args(self, mass, softening, theta, potential, acceleration):
        """Checked arguments of ``gravity`` / ``gravity_ewald``: (float32 masses
        (N,) or None, theta, eps).  Runs before any device call."""
        w = None
        if mass is not None:
            w = np.asarray(mass, dtype=np.float32)
            if w.shape != (self._n_input,):
                raise ValueError(f"mass must be (N,) with N = {self._n_input} the tree's point "
                                 f"count, got {w.shape}")
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("every mass must be finite and >= 0")
            w = np.ascontiguousarray(w)
        th = float(theta)
        if not 0.0 <= th < 1.0 or not np.float32(th) < np.float32(1.0):
            raise ValueError(f"theta must be in [0, 1), got {theta!r}")
        eps = float(softening)
        with np.errstate(over="ignore"):
            eps_ok = math.isfinite(eps) and eps >= 0.0 and bool(np.isfinite(np.float32(eps)))
        if not eps_ok:
            raise ValueError(f"softening must be finite and >= 0, got {softening!r}")
        if not (potential or acceleration):
            raise ValueError("at least one of potential and acceleration is needed")
        return w, th, eps

    def gravity(self, points: Optional[np.ndarray] = None, mass=None, softening: float = 0.0,
                theta: float = 0.5, G: float = 1.0, potential: bool = True,
                acceleration: bool = True):
        """Gravitational potential and acceleration at each query point from
        the tree's points as masses, by a Barnes-Hut walk on the GPU:
        ``phi_i = -G sum_j m_j / sqrt(d_ij^2 + softening^2)`` and
        ``acc_i = G sum_j m_j (p_j - q_i) / (d_ij^2 + softening^2)^(3/2)``.

        points : (..., 3) query points, or None: the tree's own points.
        mass : (N,) masses indexed like the tree's input points, finite and
            >= 0, or None (unit masses).
        softening : the Plummer softening length, finite and >= 0.  A point at
            the query's own position adds nothing, whatever the softening.
        theta : the opening angle in [0, 1).  A node whose box diagonal is at
            most theta times the distance to its centre of mass counts as one
            mass there; 0 is the direct sum over all points.
        G : scales both results (the device sums with G = 1).

        Returns ``(phi, acc)``: float64 arrays of shape points.shape[:-1] and
        points.shape[:-1] + (3,); the one switched off by ``potential=False``
        or ``acceleration=False`` is None.  The device sums in float32, one
        accumulator per query and component in an order fixed by the tree and
        the query: identical calls give identical arrays, whatever else is
        asked in the same call.  Periodic trees are not supported here (no Ewald
        sum): ``gravity_ewald`` is the call for them."""
        w, th, eps = self._gravity_args(mass, softening, theta, potential, acceleration)
        if self.periodic:
            raise ValueError("gravity needs a non-periodic tree: Ewald sums are not provided")
        if points is None:
            points = self.points()
        points, shape = _flatten(points)
        out_shape = tuple(shape[:-1]) if shape is not None else (np.asarray(points).shape[0],)
        phi, acc = super().gravity(points, w, th, eps, bool(potential), bool(acceleration))
        if phi is not None:
            phi = (float(G) * phi.astype(np.float64)).reshape(out_shape)
        if acc is not None:
            acc = (float(G) * acc.astype(np.float64)).reshape(out_shape + (3,))
        return phi, acc

    def potential(self, points: Optional[np.ndarray] = None, mass=None, softening: float = 0.0,
                  theta: float = 0.5, G: float = 1.0):
        """The potential alone: ``gravity(..., acceleration=False)[0]``."""
        return self.gravity(points, mass, softening, theta, G, True, False)[0]

    def gravity_ewald(self, points: Optional[np.ndarray] = None, mass=None,
                      softening: float = 0.0, theta: float = 0.5, G: float = 1.0,
                      potential: bool = True, acceleration: bool = True):
        """``gravity`` on a periodic tree: the potential and acceleration from
        the tree's points and all their periodic images (an Ewald sum, zero
        mean potential over the box), by the same Barnes-Hut walk with every
        offset taken to its nearest image and a tabulated correction added to
        each term.

        The arguments and results are those of ``gravity``.  Points outside
        the box are wrapped into [0, L) in float64 first.  The softening acts
        on the nearest image's Newtonian term only.  A point at the query's
        own position adds nothing, so the constant ``-2.8372975 G m / L`` of a
        particle's own images is not part of its potential.  The tabulated
        correction is interpolated: per unit mass it errs by up to about
        1.2e-4 / L in the potential and 5.6e-4 / L^2 in an acceleration
        component.  A non-periodic tree raises ValueError (use ``gravity``)."""
        w, th, eps = self._gravity_args(mass, softening, theta, potential, acceleration)
        if not self.periodic:
            raise ValueError("gravity_ewald needs a periodic tree: gravity sums a non-periodic "
                             "one")
        if points is None:
            points = self.points()
        points, shape = _flatten(points)
        out_shape = tuple(shape[:-1]) if shape is not None else (np.asarray(points).shape[0],)
        L = float(self.boxsize)
        p64 = np.asarray(points, dtype=np.float64)
        p64 = p64 - L * np.floor(p64 / L)
        p32 = p64.astype(np.float32)
        # (a value just below L can round up to L, which is the same place as 0)
        p32[p32 >= np.float32(L)] = 0.0
        phi, acc = super().gravity_ewald(np.ascontiguousarray(p32), w, th, eps, bool(potential),
                                         bool(acceleration))
        if phi is not None:
            phi = (float(G) * phi.astype(np.float64)).reshape(out_shape)
        if acc is not None:
            acc = (float(G) * acc.astype(np.float64)).reshape(out_shape + (3,))
        return phi, acc

    def potential_ewald(self, points: Optional[np.ndarray] = None, mass=None,
                        softening: float = 0.0, theta: float = 0.5, G: float = 1.0):
        """The potential alone: ``gravity_ewald(..., acceleration=False)[0]``."""
        return self.gravity_ewald(points, mass, softening, theta, G, True, False)[0]

    # ---------------------------------------------------------------- group potentials
    def _group_args(self, offsets, members, mass, softening, theta, max_direct):
        """Checked arguments of ``group_potential`` / ``unbind``: (offsets
        uint64 (G + 1,), members uint32 (K,), float32 masses (N,) or None,
        eps, theta, max_direct).  Runs before any device call."""
        n = self._n_input
        off = np.asarray(offsets)
        if off.ndim != 1 or off.shape[0] < 1 or off.dtype.kind not in "iu":
            raise ValueError("offsets must be a 1-D integer array of ngroups + 1 entries, got "
                             f"shape {off.shape}, dtype {off.dtype}")
        mem = np.asarray(members)
        if mem.ndim != 1 or (mem.size and mem.dtype.kind not in "iu"):
            raise ValueError(f"members must be a 1-D integer array of rows, got shape {mem.shape}, "
                             f"dtype {mem.dtype}")
        off64 = off.astype(np.int64)
        if off64[0] != 0 or off64[-1] != mem.shape[0] or np.any(off64[1:] < off64[:-1]):
            raise ValueError("offsets must start at 0, never decrease and end at len(members) = "
                             f"{mem.shape[0]}")
        if mem.size and (int(mem.min()) < 0 or int(mem.max()) >= n):
            raise ValueError(f"members must be rows in [0, N) with N = {n} the tree's point count")
        w = None
        if mass is not None:
            w = np.asarray(mass, dtype=np.float32)
            if w.shape != (n,):
                raise ValueError(f"mass must be (N,) with N = {n} the tree's point count, got "
                                 f"{w.shape}")
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("every mass must be finite and >= 0")
            w = np.ascontiguousarray(w)
        eps = float(softening)
        with np.errstate(over="ignore"):
            eps_ok = math.isfinite(eps) and eps >= 0.0 and bool(np.isfinite(np.float32(eps)))
        if not eps_ok:
            raise ValueError(f"softening must be finite and >= 0, got {softening!r}")
        th = float(theta)
        if not 0.0 <= th < 1.0 or not np.float32(th) < np.float32(1.0):
            raise ValueError(f"theta must be in [0, 1), got {theta!r}")
        if max_direct is not None:
            if int(max_direct) != max_direct or not 1 <= int(max_direct) < 2 ** 32:
                raise ValueError(f"max_direct must be None or an integer in [1, 2^32), got "
                                 f"{max_direct!r}")
            max_direct = int(max_direct)
        return (np.ascontiguousarray(off64.astype(np.uint64)),
                np.ascontiguousarray(mem, dtype=np.uint32), w, eps, th, max_direct)

    def _unwrapped(self, rows, pts):
        """float32 positions of ``rows`` relative to the first of them; on a
        periodic tree each axis takes the image nearest to it (the catalogue's
        rule: of d, d - L, d + L the smallest magnitude, ties to the earlier)."""
        d = pts[rows] - pts[rows[0]]
        if self.periodic:
            L = np.float32(self.boxsize)
            for alt in (d - L, d + L):
                closer = np.abs(alt) < np.abs(d)
                d = np.where(closer, alt, d)
        return np.ascontiguousarray(d, dtype=np.float32)

    def _group_phi(self, off, mem, w, eps, th, G, max_direct, pts=None):
        """(phi float64 (K,), most_bound int64 (G,), the cached points)."""
        phi32, minpos = super().group_potential(off, mem, w, eps, max_direct or 0)
        phi = float(G) * phi32.astype(np.float64)
        most = np.full(minpos.shape[0], -1, np.int64)
        has = minpos != np.uint32(0xFFFFFFFF)
        most[has] = mem[minpos[has]]
        if max_direct is not None:
            o = off.astype(np.int64)
            for g in np.flatnonzero(np.diff(o) > max_direct):
                if pts is None:
                    pts = self.points()
                rows = mem[o[g]:o[g + 1]]
                tmp = KDTree(self._unwrapped(rows, pts), self._leafsize)
                pg = tmp.potential(None, None if w is None else w[rows], eps, th, G)
                phi[o[g]:o[g + 1]] = pg
                most[g] = rows[int(np.argmin(pg))]
        return phi, most, pts

    def group_potential(self, offsets, members, mass=None, softening: float = 0.0,
                        G: float = 1.0, max_direct: Optional[int] = 200_000, theta: float = 0.5):
        """The potential of every member from its own group only, and each
        group's most-bound member: ``phi_e = -G sum_f m_j / sqrt(d_ij^2 +
        softening^2)`` over the entries f of e's group (i = members[e],
        j = members[f]), a direct sum on the GPU in one call for all groups.

        offsets, members : ``members[offsets[g]:offsets[g + 1]]`` = the rows of
            group g, as ``fof_catalog(..., members=True)`` returns them.  Any
            grouping is accepted: rows may be missing or repeat, groups may be
            empty, so a trimmed list (``unbind``) goes straight back in.
        mass : (N,) masses indexed like the tree's input points, finite and
            >= 0, or None (unit masses).
        softening : the Plummer softening length.  The entry itself, a repeated
            row and a coincident point add nothing, whatever the softening.
        max_direct : groups with more entries are not summed directly (the work
            is the square of the size): each is unwrapped relative to its first
            member, put into a temporary non-periodic tree and answered by
            ``potential(theta=theta)``.  Their values are approximate (the
            Barnes-Hut error of ``theta``; float32 accumulation), and their
            most-bound member is the argmin of those values.  None sums every
            group directly.  The default bounds one group's direct sum to about
            50 ms (4e10 terms at the 8e11 terms per second DESIGN.md records).

        On a periodic tree distances are minimum-image ones: the isolated
        potential of the group, meaningful for groups that do not span the box
        (``spans_box`` False).  The device forms each term in float32 and sums
        a member's terms in float64 in list order: identical calls give
        identical arrays, independent of the tree's leaf size.

        Returns ``(phi, most_bound)``: float64 (K,) aligned with ``members``,
        and int64 (G,), the row of the smallest entry with the lowest
        potential, -1 for an empty group."""
        off, mem, w, eps, th, md = self._group_args(offsets, members, mass, softening, theta,
                                                    max_direct)
        phi, most, _ = self._group_phi(off, mem, w, eps, th, G, md)
        return phi, most

    def unbind(self, offsets, members, velocities, mass=None, softening: float = 0.0,
               G: float = 1.0, max_iter: int = 20, min_members: int = 1,
               max_direct: Optional[int] = 200_000, theta: float = 0.5):
        """Iterative unbinding of a list of groups.  Each iteration computes,
        per group, the mass-weighted mean velocity of the current members (in
        float64) and ``E = |v - vbar|^2 / 2 + phi`` with ``phi`` from
        ``group_potential`` (same arguments); every member with E >= 0 is
        dropped (order kept), and a group left with fewer than ``min_members``
        members is emptied.  It stops when an iteration drops nothing, or after
        ``max_iter`` iterations.

        velocities : (N, 3) indexed like the tree's input points.

        Returns a dict: ``offsets`` uint64 (G + 1,) (the same G: an emptied
        group has equal offsets) and ``members`` uint32, the bound members;
        ``phi`` and ``energy`` float64, of that final state and aligned with
        ``members``; ``most_bound`` int64 (G,) (-1 for an empty group);
        ``iterations``, the number of iterations run (the last one, which
        dropped nothing, included)."""
        off, mem, w, eps, th, md = self._group_args(offsets, members, mass, softening, theta,
                                                    max_direct)
        n = self._n_input
        vel = np.asarray(velocities, dtype=np.float64)
        if vel.shape != (n, 3):
            raise ValueError(f"velocities must be (N, 3) with N = {n} the tree's point count, got "
                             f"{vel.shape}")
        if int(max_iter) < 0:
            raise ValueError(f"max_iter must be >= 0, got {max_iter!r}")
        min_members = max(int(min_members), 1)
        w64 = np.ones(n, np.float64) if w is None else w.astype(np.float64)
        ngroups = off.shape[0] - 1
        pts, iterations = None, 0
        while True:
            phi, most, pts = self._group_phi(off, mem, w, eps, th, G, md, pts)
            o = off.astype(np.int64)
            cnt = np.diff(o)
            full = np.flatnonzero(cnt > 0)
            starts = o[:-1][full]  # strictly ascending: reduceat sums exactly these groups
            gid = np.repeat(np.arange(ngroups), cnt)
            mm, vv = w64[mem], vel[mem]
            vbar = np.zeros((ngroups, 3))
            if full.size:
                msum = np.add.reduceat(mm, starts)
                with np.errstate(divide="ignore", invalid="ignore"):
                    vb = np.add.reduceat(mm[:, None] * vv, starts, axis=0) / msum[:, None]
                plain = np.add.reduceat(vv, starts, axis=0) / cnt[full][:, None]
                vbar[full] = np.where(msum[:, None] > 0, vb, plain)  # (massless group: plain mean)
            dv = vv - vbar[gid]
            energy = 0.5 * np.sum(dv * dv, axis=1) + phi
            if iterations >= int(max_iter):
                break
            iterations += 1
            keep = ~(energy >= 0.0)
            left = np.zeros(ngroups, np.int64)
            if full.size:
                left[full] = np.add.reduceat(keep.astype(np.int64), starts)
            keep &= (left >= min_members)[gid]
            if keep.all():
                break
            left = np.where(left >= min_members, left, 0)
            mem = np.ascontiguousarray(mem[keep])
            off = np.concatenate([[0], np.cumsum(left)]).astype(np.uint64)
        return {"offsets": off, "members": mem, "phi": phi, "energy": energy,
                "most_bound": most, "iterations": iterations}

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
