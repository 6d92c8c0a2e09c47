"""Barnes-Hut gravity on a periodic tree (nbkd_gravity_ewald) beside
nbkd_gravity on a non-periodic tree over the same points: uniform points at
each --n and the log-normal set at --lognormal, leafsize 64, the tree's own
points as device queries, device outputs, unit masses, box 1.  Per input and
opening angle theta (--thetas; theta = 0, the direct sum, only up to
--direct-max points):
  both calls (HIP events) and both walk kernels (the library's event timers) in
  one process: a warm-up round, then --steps rounds with the two calls
  interleaved, medians; their ratio is the cost of periodicity;
  the mean number of monopole and point terms per query of the periodic walk,
  from a host model of the walk nbkd.h defines on --model-rows own points;
  the rms and the maximum relative acceleration error |a - a0| / |a0| on a
  fixed sample of --sample rows against the library's own theta = 0, and against
  a float64 direct Ewald sum on the host (nbkd.h's formulas, no table) for as
  many of the first --exact-rows of them as --exact-pairs (rows x points) allows:
  the host sum costs about 300 erfc / exp / cos per pair.

Writes --out (default profiles/gravity_ewald.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nbodyhpc_amd import capi, hip, synth  # noqa: E402
from gravity_run import Model, rel_err, stats  # noqa: E402
from tests import ewald_oracle as eo  # noqa: E402


def wrap(d):
    """the nearest image in a unit box (float32, nbkd.h's rule)"""
    one = np.float32(1.0)
    dm, dp = d - one, d + one
    r = np.where(np.abs(dm) < np.abs(d), dm, d)
    return np.where(np.abs(dp) < np.abs(r), dp, r)


class PeriodicModel(Model):
    def terms(self, q, theta):
        """(monopole terms, point terms) per query, offsets wrapped"""
        th2 = np.float32(theta) * np.float32(theta)
        mono, pts = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
        stack = [(0, np.arange(len(q)))]
        left, right, dim = self.nodes["left"], self.nodes["right"], self.nodes["dim"]
        while stack:
            i, rows = stack.pop()
            if th2 > 0:
                d = wrap(self.c[i][None, :] - q[rows])
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                ok = self.s2[i] <= th2 * d2
                mono[rows[ok]] += 1
                rows = rows[~ok]
                if rows.size == 0:
                    continue
            if dim[i] < 0:
                pts[rows] += self.count[i]
            else:
                stack.append((int(right[i]), rows))
                stack.append((int(left[i]), rows))
        return mono, pts


def ewald64(pts, q):
    """float64 direct Ewald accelerations at q (unit masses, unit box); the
    real-space images with |n_i| <= 2: the next ones are at r >= 2.5, where
    erfc(2 r) < 2e-12"""
    near = eo.IMAGES[np.abs(eo.IMAGES).max(axis=1) <= 2]
    out = np.zeros((len(q), 3))
    for j in range(len(q)):
        for a in range(0, len(pts), 50_000):
            d = pts[a:a + 50_000].astype(np.float64) - q[j].astype(np.float64)[None, :]
            d -= np.round(d)
            d2 = (d * d).sum(axis=1)
            on = d2 > 0
            d, d2 = d[on], d2[on]
            _, ca = eo.corrections(d, near)
            out[j] += (d * (d2 ** -1.5)[:, None] + ca).sum(axis=0)
    return out


def run(kind, n, leaf, steps, thetas, direct_max, nsample, nmodel, nexact, exact_pairs):
    pts = synth.uniform(n) if kind == "uniform" else synth.lognormal(n)
    pts[pts >= np.float32(1.0)] = 0.0
    d = hip.DeviceArray.from_numpy(pts)
    s = hip.Stream()
    per = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0, stream=s.handle)
    flat = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, stream=s.handle)
    rng = np.random.default_rng(30)
    rows = np.sort(rng.choice(n, min(nsample, n), replace=False))
    mrows = rows[:: max(1, len(rows) // nmodel)][:nmodel]
    sample = np.ascontiguousarray(pts[rows])
    nexact = int(min(nexact, exact_pairs // n))
    a64 = ewald64(pts, sample[:nexact]) if nexact else None
    del pts
    model = PeriodicModel(per, n)
    phi = hip.DeviceArray((n,), np.float32)
    acc = hip.DeviceArray((n, 3), np.float32)
    ds = hip.DeviceArray.from_numpy(sample)
    a0d = hip.DeviceArray((len(rows), 3), np.float32)
    per.gravity_ewald_device(ds.ptr, len(rows), None, 0.0, 0.0, None, a0d.ptr, stream=s.handle)
    s.synchronize()
    a0 = a0d.numpy().astype(np.float64)
    res = {"input": kind, "n": n, "leafsize": leaf, "steps": steps, "nodes": int(per.size),
           "sample_rows": len(rows), "model_rows": len(mrows), "exact_rows": nexact, "rows": []}
    if nexact:
        res["theta0_rel_err_vs_f64_ewald_rms"], res["theta0_rel_err_vs_f64_ewald_max"] = \
            rel_err(a0[:nexact], a64)
    calls = {"ewald": lambda th: per.gravity_ewald_device(d.ptr, n, None, th, 0.0, phi.ptr,
                                                         acc.ptr, stream=s.handle),
             "plain": lambda th: flat.gravity_device(d.ptr, n, None, th, 0.0, phi.ptr, acc.ptr,
                                                     stream=s.handle)}
    scope = {"ewald": "gravity_ewald_walk", "plain": "gravity_walk"}
    capi.timing_enable(True)
    try:
        for theta in thetas:
            if theta == 0.0 and n > direct_max:
                continue
            label = f"{kind} n={n:.0e} theta={theta}"
            call = {k: [] for k in calls}
            walk = {k: [] for k in calls}
            for rnd in range(steps + 1):
                for k in ("plain", "ewald"):  # interleaved; the last call leaves acc
                    capi.timing_reset()
                    e0, e1 = hip.Event(), hip.Event()
                    e0.record(s.handle)
                    calls[k](theta)
                    e1.record(s.handle)
                    s.synchronize()
                    if rnd:
                        call[k].append(e0.elapsed_ms(e1))
                        walk[k].append(capi.timing_read(scope[k])[0])
            a = acc.numpy()[rows].astype(np.float64)
            if not np.all(np.isfinite(a)):
                raise RuntimeError(f"{label}: accelerations that are not finite")
            rms0, max0 = rel_err(a, a0)
            mono, pnt = model.terms(sample[np.searchsorted(rows, mrows)], theta)
            row = {"theta": theta, "call": stats(call["ewald"]), "walk": stats(walk["ewald"]),
                   "gravity_call": stats(call["plain"]), "gravity_walk": stats(walk["plain"]),
                   "walk_ratio": float(np.median(walk["ewald"]) / np.median(walk["plain"])),
                   "mean_monopole_terms": float(mono.mean()),
                   "mean_point_terms": float(pnt.mean()),
                   "acc_rel_err_rms": rms0, "acc_rel_err_max": max0}
            if nexact:
                row["acc_rel_err_vs_f64_ewald_rms"], row["acc_rel_err_vs_f64_ewald_max"] = \
                    rel_err(a[:nexact], a64)
            res["rows"].append(row)
            print(f"{label}: call {row['call']['median_ms']:.2f} ms, walk "
                  f"{row['walk']['median_ms']:.2f}; nbkd_gravity walk "
                  f"{row['gravity_walk']['median_ms']:.2f} (ratio {row['walk_ratio']:.2f}); terms "
                  f"{row['mean_monopole_terms']:.0f} + {row['mean_point_terms']:.0f}; acc error "
                  f"rms {rms0:.2e} max {max0:.2e}"
                  + (f" (against the float64 Ewald sum, {nexact} rows: "
                     f"{row['acc_rel_err_vs_f64_ewald_rms']:.2e}, "
                     f"{row['acc_rel_err_vs_f64_ewald_max']:.2e})" if nexact else ""), flush=True)
    finally:
        capi.timing_enable(False)
    per.close()
    flat.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e5, 1e6, 1e7])
    ap.add_argument("--lognormal", type=float, nargs="*", default=[1e5, 1e6, 1e7])
    ap.add_argument("--thetas", type=float, nargs="*", default=[0.0, 0.3, 0.5, 0.7])
    ap.add_argument("--direct-max", type=float, default=1e5)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--model-rows", type=int, default=32)
    ap.add_argument("--exact-rows", type=int, default=32)
    ap.add_argument("--exact-pairs", type=float, default=3.2e6)
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gravity_ewald.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    args = (a.leaf, a.steps, a.thetas, a.direct_max, a.sample, a.model_rows, a.exact_rows,
            int(a.exact_pairs))
    runs = [run("uniform", int(n), *args) for n in a.n]
    runs += [run("lognormal", int(n), *args) for n in a.lognormal]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"runs": runs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
