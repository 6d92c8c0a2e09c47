"""Observer-frame pair counts (nbkd_query_ball_hist2_obs) against the fixed-axis
ones (nbkd_query_ball_hist2, los = 2) at the same edges on the same tree in the
same process: what the per-pair line of sight (a division per pair) and the lost
cylinder pruning (the walk follows the bounding ball) cost.  Non-periodic
trees of uniform points at --n and of the log-normal set at --lognormal,
leafsize 64, the tree's own points as device queries, the observer at
--distance box lengths from the centre of the box along -z.  Per input, the
configurations of scripts/ball_hist2_run.py:
  (a) SMU, 16 geometric s edges 0.0005 L .. 0.01 L, nmu = 1,
  (b) the same s edges, nmu = 16,
  (c) RPPI, 16 x 16, the same edges as rp, pi_max = rp_max = 0.01 L,
  (d) RPPI, 16 x 40, pi_max = 0.04 L (the elongated cylinder),
each once with the observer and once along the axis, and ball_hist at the same
s edges (totals only).  One process, interleaved rounds (every operation once
per round), a warm-up round, then --steps rounds: HIP events time the calls, the
library's event timers the kernels; medians, min and max are reported.

Asserted here: the observer-frame (a), and (b) summed over mu, equal the
differenced ball_hist totals (pi2 <= s2 by the clamp), as the fixed-axis ones do.

Writes --out (default profiles/ball_hist2_obs.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402

N1 = 16
S_MIN, S_MAX, PI_LONG = 0.0005, 0.01, 0.04
KEYS = ("a_smu_nmu1", "b_smu_nmu16", "c_rppi_16x16", "d_rppi_16x40")


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def run(kind, n, leaf, steps, distance):
    pts = synth.uniform(n) if kind == "uniform" else synth.lognormal(n)
    d = hip.DeviceArray.from_numpy(pts)
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, stream=s.handle)
    observer = np.array([0.5, 0.5, 0.5 - distance], np.float32)
    edges = np.geomspace(S_MIN, S_MAX, N1).astype(np.float32)
    e2 = {"a_smu_nmu1": (np.array([1.0], np.float32), capi.NBKD_HIST2_SMU),
          "b_smu_nmu16": (((np.arange(16) + 1.0) / 16).astype(np.float32), capi.NBKD_HIST2_SMU),
          "c_rppi_16x16": ((S_MAX * (np.arange(16) + 1.0) / 16).astype(np.float32),
                           capi.NBKD_HIST2_RPPI),
          "d_rppi_16x40": ((PI_LONG * (np.arange(40) + 1.0) / 40).astype(np.float32),
                           capi.NBKD_HIST2_RPPI)}
    got = {}

    def obs(k):
        def fn():
            got["obs_" + k] = t.ball_hist2_obs_device(d.ptr, n, edges, e2[k][0], e2[k][1],
                                                      observer, stream=s.handle)
        return fn

    def axis(k):
        def fn():
            got["axis_" + k] = t.ball_hist2_device(d.ptr, n, edges, e2[k][0], e2[k][1], 2,
                                                   stream=s.handle)
        return fn

    def hist():
        got["ball_hist"] = t.ball_hist_device(d.ptr, n, edges, None, stream=s.handle)

    ops = {}
    for k in KEYS:  # the pair of one configuration runs back to back
        ops["obs_" + k] = ("ball_hist2_obs", obs(k))
        ops["axis_" + k] = ("ball_hist2", axis(k))
    ops["ball_hist"] = ("ball_hist", hist)
    call = {k: [] for k in ops}
    kern = {k: [] for k in ops}
    capi.timing_enable(True)
    try:
        for rnd in range(steps + 1):  # round 0 warms up (the workspace grows there)
            for k, (scope, fn) in ops.items():
                capi.timing_reset()
                e0, e1 = hip.Event(), hip.Event()
                e0.record(s.handle)
                fn()
                e1.record(s.handle)
                s.synchronize()
                if rnd == 0:
                    print(f"{kind} n={n:.0e}: warmed up {k}", flush=True)
                    continue
                call[k].append(e0.elapsed_ms(e1))
                kern[k].append(capi.timing_read(scope)[0])
    finally:
        capi.timing_enable(False)
    want = np.diff(got["ball_hist"].astype(np.int64), prepend=0).astype(np.uint64)
    for frame in ("obs_", "axis_"):
        if not np.array_equal(got[frame + "a_smu_nmu1"][:, 0], want):
            raise RuntimeError(f"{kind} n={n}: {frame}(a) differs from the differenced ball_hist "
                               "totals")
        if not np.array_equal(got[frame + "b_smu_nmu16"].sum(axis=1), want):
            raise RuntimeError(f"{kind} n={n}: {frame}(b) summed over mu differs from the "
                               "differenced ball_hist totals")
    res = {"input": kind, "n": n, "leafsize": leaf, "steps": steps, "periodic": False,
           "observer": [float(x) for x in observer], "s_edges": [float(e) for e in edges],
           "pairs_within_s_max": int(got["ball_hist"][-1])}
    for k in ops:
        res[k] = {"call": stats(call[k]), "kernel": stats(kern[k]), "kernel_scope": ops[k][0]}
        if k != "ball_hist":
            res[k]["pairs_counted"] = int(got[k].sum())
    res["obs_over_axis"] = {}
    for k in KEYS:
        o, a = res["obs_" + k]["kernel"], res["axis_" + k]["kernel"]
        # the range of the ratio: the extremes of the two kernels against each other
        res["obs_over_axis"][k] = {"median": o["median_ms"] / a["median_ms"],
                                   "min": o["min_ms"] / a["max_ms"],
                                   "max": o["max_ms"] / a["min_ms"]}
    ball = lambda rp, pi: (rp * rp + pi * pi) ** 1.5  # noqa: E731
    oc, od = res["obs_c_rppi_16x16"]["kernel"], res["obs_d_rppi_16x40"]["kernel"]
    ac, ad = res["axis_c_rppi_16x16"]["kernel"], res["axis_d_rppi_16x40"]["kernel"]
    res["d_over_c"] = {"obs_kernel": od["median_ms"] / oc["median_ms"],
                       "axis_kernel": ad["median_ms"] / ac["median_ms"],
                       "bounding_ball_volume": ball(S_MAX, PI_LONG) / ball(S_MAX, S_MAX),
                       "cylinder_volume": PI_LONG / S_MAX}
    print(f"{kind} n={n:.0e} ({res['pairs_within_s_max'] / n:.1f} pairs per query within s_max): "
          "kernel ms observer / axis "
          + " ".join(f"({k[0]}) {res['obs_' + k]['kernel']['median_ms']:.2f} / "
                     f"{res['axis_' + k]['kernel']['median_ms']:.2f} = "
                     f"{res['obs_over_axis'][k]['median']:.2f}" for k in KEYS)
          + f"; ball_hist {res['ball_hist']['kernel']['median_ms']:.2f}; (d)/(c) observer "
          f"{res['d_over_c']['obs_kernel']:.2f}, axis {res['d_over_c']['axis_kernel']:.2f} at "
          f"{res['d_over_c']['bounding_ball_volume']:.1f} times the bounding ball", flush=True)
    t.close()
    d.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e7])
    ap.add_argument("--lognormal", type=float, default=1e7, help="0: skip")
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--distance", type=float, default=3.0,
                    help="the observer's distance from the box centre, in box lengths")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_hist2_obs.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    runs = [run("uniform", int(n), a.leaf, a.steps, a.distance) for n in a.n]
    if a.lognormal:
        runs.append(run("lognormal", int(a.lognormal), a.leaf, a.steps, a.distance))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"runs": runs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
