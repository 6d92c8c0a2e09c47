"""The collect kernel's scan loop (knn_collect.hip grp_packet: the pair list,
the scan steps, the bound histogram and its tighten) on the smallest shapes at
which it can go wrong.  Every case goes through the C ABI on a tree of at most
5e4 points and is compared twice:

  - with the oracle by tests.parity.assert_knn_equal (distances bit for bit);
  - with arrays recorded once on the GPU from the library of the commit before
    the scan loop was rewritten (tests/golden/collect_scan_parent.npz, written
    by tests/golden/gen_collect_scan.py): the same distances, the same ids and
    the same six work counters.  The ids pin the order inside exact-distance
    ties, which the oracle comparison leaves free, so a column that fills in
    another order shows; the counters catch a bound that tightened differently.

The cases (tests/collect_scan_cases.py):
  steps-*    single-leaf trees of 8 and 64 points with 1..65 queries: the one
             scanned leaf's pair list runs from one entry to several scan
             steps, odd and even step counts, the last packet one valid lane
  full-*     64 (63) queries inside one 64-point leaf whose seed balls cover
             all of it: the full 512-entry pair list, and 504 entries with
             the last packet slot unused (both whole scan steps: the padding
             pairs run in the steps-* cases, 1 pair + 7 padding in
             steps-n8-m1)
  shape-*    every leaf shape of the three instances: leaf sizes 8, 32, 64
             (one chunk) and 128 (half-leaves), open and periodic (queries
             within a seed radius of the faces: the periodic scan)
  units-*    a periodic box of side 205 000
  overflow   100 coincident points around a query at k = 8 (column of 48): the
             clamp overwrites the last slot, the exact path answers the row
  byte-edge  255 coincident points in one histogram bucket of one k = 128
             query: 255 candidates in its 256-slot column, no re-walk
"""
import functools
import os

import numpy as np
import pytest

from tests import collect_scan_cases as cs
from tests.parity import assert_knn_equal
from tests.test_gpu_collect_walk import COUNTERS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "collect_scan_parent.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture
def knobs(gpu):
    saved = {n: gpu.get_tuning(n) for n in ("knn_seed_margin", "candidate_bytes")}
    yield gpu.set_tuning
    for n, v in saved.items():
        gpu.set_tuning(n, v)


def run_case(gpu, set_tuning, pts, q, k, leaf, box, tune):
    """Rows from the plain instance, then rows and the six work counters from
    the instrumented one; both must agree."""
    for n, v in tune.items():
        set_tuning(n, v)
    t = gpu.Tree(pts, leafsize=leaf, boxsize=box)
    try:
        d, i = t.query(q, k)
        gpu.stats_enable(True)
        try:
            ds, is_ = t.query(q, k)
            st = gpu.stats_read_all()
        finally:
            gpu.stats_enable(False)
    finally:
        t.close()
    assert np.array_equal(d.view(np.uint32), ds.view(np.uint32)) and np.array_equal(i, is_)
    return d, i, np.array([st[n] for n in COUNTERS], np.int64)


_ORACLE = {}


def oracle_rows(oracle, group, pts, q, box, kmax):
    """The oracle's rows of a group's queries, computed once at the group's
    largest k; a case's rows are their first k columns (sorted distances)."""
    if group not in _ORACLE:
        _ORACLE[group] = oracle.tree(pts, 32, box).query(q, kmax, workers=8)
    return _ORACLE[group]


@pytest.mark.parametrize("name", cs.names())
def test_scan_case(gpu, oracle, knobs, name):
    pts, q, k, leaf, box, tune, group = cs.case(name)
    assert len(pts) <= 50_000
    d, i, c = run_case(gpu, knobs, pts, q, k, leaf, box, tune)
    g = _golden()
    kmax = g[group + "__d"].shape[1]
    dr, ir = oracle_rows(oracle, group, pts, q, box, kmax)
    assert_knn_equal(d, i, dr[:, :k], ir[:, :k], pts, q, box)
    want_d = g[group + "__d"][:, :k]
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), "distances differ from the parent's"
    assert np.array_equal(i, g[name + "__i"]), "ids (tie order) differ from the parent's"
    assert dict(zip(COUNTERS, c.tolist())) == dict(zip(COUNTERS, g[name + "__c"].tolist()))
