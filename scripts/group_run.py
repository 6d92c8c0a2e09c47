"""Group catalogue (nbkd_group_catalog) next to the group finder that feeds it:
uniform periodic points at each --n, leafsize 64, device inputs and outputs.
Per linking length --f (in mean spacings: 0.2 barely links, 0.9 is past
percolation, one group holding most points) and per --min-members, after a
warm-up of everything, HIP events time
  (a) one fof call (labels and sizes),
  (b) one group_catalog call (every output; weights and three value channels),
each `--steps` times (the median is reported); the library's event timers give
the per-phase split (fof_hook / fof_flatten / fof_label, group_sort /
group_moments / group_combine).  Each catalogue is checked once on the host:
sizes against the fof sizes, the offsets against their cumulative sum, the
members of the largest group against the labels, its weight sum against numpy
within size * 2^-52 * sum |w|, and a second call against the first with ==.

One process; writes the numbers to --out (default profiles/group.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402
from scripts.fof_run import kernel_ms, setup, timed  # noqa: E402

NV = 3
FOF_SCOPES = ("fof_hook", "fof_flatten", "fof_label")
GROUP_SCOPES = ("group_sort", "group_moments", "group_combine")


def run(n, leaf, steps, f, min_members):
    d, s, t = setup("uniform", n, leaf)
    b = f * n ** (-1.0 / 3.0)
    rng = np.random.default_rng(1)
    w = (0.5 + rng.random(n, dtype=np.float32)).astype(np.float32)
    v = rng.standard_normal((n, NV), dtype=np.float32)
    dw, dv = hip.DeviceArray.from_numpy(w), hip.DeviceArray.from_numpy(v)
    lab = hip.DeviceArray((n,), np.uint32)
    siz = hip.DeviceArray((n,), np.uint32)

    def fof():
        t.fof_device(b, lab.ptr, siz.ptr, stream=s.handle)

    fof()
    s.synchronize()
    hl, hs = lab.numpy(), siz.numpy()
    res = {"n": n, "leafsize": leaf, "b": b, "b_in_spacings": f, "steps": steps, "nv": NV,
           "ngroups": int(np.count_nonzero(hs)), "largest_group": int(hs.max())}
    res["fof_call"] = timed(s, steps, fof)
    res["fof_kernels"] = kernel_ms(FOF_SCOPES, s, steps, fof)
    for mm in min_members:
        G, K = t.group_catalog_device(lab.ptr, dw.ptr, dv.ptr, NV, mm, 0, 0, stream=s.handle)
        nt = 5 + 2 * NV
        outs = [hip.DeviceArray((max(G, 1),), np.uint32), hip.DeviceArray((max(G, 1),), np.uint32),
                hip.DeviceArray((G + 1,), np.uint64), hip.DeviceArray((max(K, 1),), np.uint32),
                hip.DeviceArray((max(G, 1), nt), np.float64),
                hip.DeviceArray((max(G, 1),), np.float32)]

        def catalog():
            return t.group_catalog_device(lab.ptr, dw.ptr, dv.ptr, NV, mm, G, K,
                                          *[o.ptr for o in outs], stream=s.handle)

        def sizing():
            return t.group_catalog_device(lab.ptr, dw.ptr, dv.ptr, NV, mm, 0, 0, stream=s.handle)

        assert catalog() == (G, K)
        first = [o.numpy() for o in outs]
        head, size, off, mem, mom = (first[0][:G], first[1][:G], first[2], first[3][:K],
                                     first[4][:G])
        # host checks
        keep = np.flatnonzero(hs >= mm)
        assert np.array_equal(head, keep) and np.array_equal(size, hs[keep])
        assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), size)
        if G:
            g = int(np.argmax(size))
            rows = np.flatnonzero(hl == head[g])
            assert np.array_equal(mem[int(off[g]):int(off[g + 1])], rows)
            ws = w[rows].astype(np.float64)
            assert abs(mom[g, 0] - ws.sum()) <= len(rows) * 2.0 ** -52 * np.abs(ws).sum()
        assert catalog() == (G, K)
        assert all(np.array_equal(a, o.numpy()) for a, o in zip(first, outs))
        del first, head, size, off, mem, mom
        r = {"min_members": mm, "groups_kept": G, "rows_kept": K,
             "catalog_call": timed(s, steps, catalog), "sizing_call": timed(s, steps, sizing),
             "catalog_kernels": kernel_ms(GROUP_SCOPES, s, steps, catalog)}
        r["catalog_over_fof_call"] = r["catalog_call"]["median_ms"] / res["fof_call"]["median_ms"]
        res.setdefault("catalogs", []).append(r)
        kk = r["catalog_kernels"]
        print(f"n={n:.0e} b={f} min_members={mm}: fof {res['fof_call']['median_ms']:.2f} ms (hook "
              f"{res['fof_kernels']['fof_hook']['ms_per_call']:.2f}); catalog "
              f"{r['catalog_call']['median_ms']:.2f} ms (sort {kk['group_sort']['ms_per_call']:.2f},"
              f" moments {kk['group_moments']['ms_per_call']:.2f}, combine "
              f"{kk['group_combine']['ms_per_call']:.2f}), sizing call "
              f"{r['sizing_call']['median_ms']:.2f} ms; {G} groups, {K} rows, largest "
              f"{res['largest_group']}", flush=True)
        for o in outs:
            o.free()
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e7, 1e8])
    ap.add_argument("--f", type=float, nargs="+", default=[0.2, 0.9])
    ap.add_argument("--min-members", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    out = {"runs": [run(int(n), a.leaf, a.steps, f, a.min_members) for n in a.n for f in a.f]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
