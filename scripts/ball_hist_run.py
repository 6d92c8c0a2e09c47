"""The radius histogram against the calls it replaces: uniform periodic points,
leafsize 64, the tree's own points as device queries, 16 log-spaced radii from
0.001 L to 0.01 L.  After a warm-up pass of everything, HIP events time
  (a) one ball_hist call, totals only,
  (b) one ball_count at the largest radius,
  (c) the 16 ball_count calls that (a) replaces,
each `--steps` times (the median is reported), and (a)'s totals are checked
against the column sums of (c).  One process, no environment switches; writes
the numbers to --out (default profiles/ball_hist.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402


def timed(stream, steps, fn):
    """median / min / max of `steps` event-timed runs of fn() on the stream, ms"""
    ms = []
    for _ in range(steps):
        e0, e1 = hip.Event(), hip.Event()
        e0.record(stream)
        fn()
        e1.record(stream)
        ms.append(e0.elapsed_ms(e1))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def run(n, radii, leaf, steps):
    pts = synth.uniform(n)
    d = hip.DeviceArray.from_numpy(pts)
    del pts
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0, stream=s.handle)
    cnt = hip.DeviceArray((n,), np.uint32)

    def hist():
        return t.ball_hist_device(d.ptr, n, radii, None, stream=s.handle)

    def count(r):
        t.ball_count_device(d.ptr, n, float(r), cnt.ptr, s.handle)

    # warm-up (the workspace grows here), and the check: (a)'s totals are the
    # column sums of the 16 single-radius counts
    tot = hist()
    sums = []
    for r in radii:
        count(r)
        s.synchronize()
        sums.append(int(cnt.numpy().sum(dtype=np.uint64)))
    if [int(v) for v in tot] != sums:
        raise RuntimeError(f"n={n}: ball_hist totals {list(tot)} != ball_count sums {sums}")
    a = timed(s, steps, hist)
    b = timed(s, steps, lambda: count(radii[-1]))
    c = timed(s, steps, lambda: [count(r) for r in radii])
    s.synchronize()
    res = {"n": n, "leafsize": leaf, "steps": steps, "totals": sums,
           "a_ball_hist_totals": a, "b_ball_count_rmax": b, "c_ball_count_x16": c,
           "a_over_b": a["median_ms"] / b["median_ms"],
           "a_over_c": a["median_ms"] / c["median_ms"]}
    print(f"n={n:.0e}: (a) ball_hist {a['median_ms']:.2f} ms, (b) ball_count(r_max) "
          f"{b['median_ms']:.2f} ms, (c) 16 x ball_count {c['median_ms']:.2f} ms; "
          f"a/b {res['a_over_b']:.2f}, a/c {res['a_over_c']:.3f}; totals match", flush=True)
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="+", default=[1e7, 1e8])
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_hist.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    radii = np.logspace(-3.0, -2.0, 16).astype(np.float32)
    out = {"radii": [float(r) for r in radii], "runs": [run(int(n), radii, a.leaf, a.steps)
                                                        for n in a.n]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ok = all(r["a_over_c"] < 1.0 for r in out["runs"])
    print("ball_hist below 16 x ball_count at every size" if ok
          else "FAIL: ball_hist is not below 16 x ball_count", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
