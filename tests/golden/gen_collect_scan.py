"""Recorder of tests/golden/collect_scan_parent.npz: every case of
tests/collect_scan_cases.py through the C ABI of the library that NBKD_LIB
names (the build of the commit before the scan loop was rewritten), on a GPU.

  NBKD_LIB=<parent build>/libnbkd.so python tests/golden/gen_collect_scan.py [out.npz]

Per case <name>__i (ids) and <name>__c (the six work counters of
tests.test_gpu_collect_walk.COUNTERS); per group of cases that share points,
queries and box <group>__d, the sorted distances at the group's largest k, of
which each case's distances must be the first k columns (checked here)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nbodyhpc_amd import capi  # noqa: E402
from tests import collect_scan_cases as cs  # noqa: E402
from tests.test_gpu_collect_scan import run_case  # noqa: E402
from tests.test_gpu_collect_walk import COUNTERS  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden",
                                                              "collect_scan_parent.npz")
    saved = {n: capi.get_tuning(n) for n in ("knn_seed_margin", "candidate_bytes")}
    arrays, dist = {}, {}
    for name in cs.names():
        pts, q, k, leaf, box, tune, group = cs.case(name)
        d, i, c = run_case(capi, capi.set_tuning, pts, q, k, leaf, box, tune)
        for n, v in saved.items():
            capi.set_tuning(n, v)
        arrays[name + "__i"] = i
        arrays[name + "__c"] = c
        if group not in dist or dist[group].shape[1] < k:
            dist[group], d = d, dist.get(group, d)
        kk = d.shape[1]
        assert np.array_equal(dist[group][:, :kk].view(np.uint32), d.view(np.uint32)), name
        print(name, dict(zip(COUNTERS, c.tolist())), flush=True)
    for group, d in dist.items():
        arrays[group + "__d"] = d
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes", "lib", os.environ.get("NBKD_LIB", "production"))


if __name__ == "__main__":
    main()
