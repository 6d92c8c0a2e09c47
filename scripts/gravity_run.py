"""Barnes-Hut potentials and accelerations (nbkd_gravity): non-periodic uniform
points at each --n and the log-normal set at --lognormal, leafsize 64, the
tree's own points as device queries, device outputs, unit masses.  Per input
and opening angle theta (--thetas; theta = 0, the direct sum, only up to
--direct-max points):
  the call (HIP events), the moments pass and the walk kernel (the library's
  event timers): one process, a warm-up round, then --steps rounds, medians;
  the mean number of monopole and point terms per query, from a host model of
  the walk nbkd.h defines on a fixed sample of --model-rows own points;
  the rms and the maximum relative acceleration error |a - a0| / |a0| against
  theta = 0 on a fixed sample of --sample rows, and against a float64 direct
  sum on the host for the first --exact-rows of them (theta = 0 sums up to n
  float32 terms in sequence: at 1e7 points its own rounding is what the first
  figure shows).
Beside each row, the nearest existing kernel: kernel_sum (nbkd_query_ball_sum),
top-hat, unit weights, at the radius whose balls hold the row's mean number of
point terms on average (two corrections of the uniform-density radius).

Writes --out (default profiles/gravity.json)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


class Model:
    """The node moments of an exported tree with unit masses (float64 sums; the
    last bits of the summation order do not matter for counting terms) and the
    walk's term counts for a few queries."""

    def __init__(self, tree, n):
        nodes, x, y, z, perm = tree.export()
        self.nodes = nodes
        xyz = np.stack([x, y, z], 1)
        real = perm < n
        leaf = np.flatnonzero(nodes["dim"] < 0)
        nn = len(nodes)
        M, S = np.zeros(nn), np.zeros((nn, 3))
        lo, hi = np.full((nn, 3), np.inf), np.full((nn, 3), -np.inf)
        # leaves are consecutive ranges of tree positions, in node order
        start = nodes["left"][leaf].astype(np.int64)
        w = real.astype(np.float64)
        M[leaf] = np.add.reduceat(w, start)
        S[leaf] = np.add.reduceat(w[:, None] * xyz.astype(np.float64), start, axis=0)
        lo[leaf] = np.minimum.reduceat(np.where(real[:, None], xyz, np.inf), start, axis=0)
        hi[leaf] = np.maximum.reduceat(np.where(real[:, None], xyz, -np.inf), start, axis=0)
        self.count = np.zeros(nn, np.int64)
        self.count[leaf] = np.add.reduceat(real.astype(np.int64), start)
        left, right, dim = nodes["left"], nodes["right"], nodes["dim"]
        for i in range(nn - 1, -1, -1):  # preorder: children follow their parent
            if dim[i] >= 0:
                l, r = left[i], right[i]
                M[i] = M[l] + M[r]
                S[i] = S[l] + S[r]
                lo[i] = np.minimum(lo[l], lo[r])
                hi[i] = np.maximum(hi[l], hi[r])
        self.c = (S / M[:, None]).astype(np.float32)
        e = (hi - lo).astype(np.float32)
        self.s2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]

    def terms(self, q, theta):
        """(monopole terms, point terms) per query"""
        th2 = np.float32(theta) * np.float32(theta)
        mono, pts = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
        stack = [(0, np.arange(len(q)))]
        left, right, dim = self.nodes["left"], self.nodes["right"], self.nodes["dim"]
        while stack:
            i, rows = stack.pop()
            if th2 > 0:
                d = self.c[i][None, :] - q[rows]
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


def direct64(pts, q):
    """float64 direct-sum accelerations at q (unit masses, no softening)"""
    out = np.zeros((len(q), 3))
    q64 = q.astype(np.float64)
    for a in range(0, len(pts), 100_000):
        d = pts[None, a:a + 100_000, :].astype(np.float64) - q64[:, None, :]
        d2 = (d * d).sum(axis=2)
        with np.errstate(divide="ignore"):
            w = np.where(d2 > 0, d2 ** -1.5, 0.0)
        out += (w[:, :, None] * d).sum(axis=1)
    return out


def rel_err(a, ref):
    rel = np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)
    return float(np.sqrt(np.mean(rel * rel))), float(rel.max())


def timed(fn, scopes, s, steps, label):
    """a warm-up, then `steps` timed calls: (call ms, {scope: kernel ms})"""
    call, kern = [], {k: [] for k in scopes}
    for rnd in range(steps + 1):
        capi.timing_reset()
        e0, e1 = hip.Event(), hip.Event()
        e0.record(s.handle)
        fn()
        e1.record(s.handle)
        s.synchronize()
        if rnd == 0:
            print(f"{label}: warmed up", flush=True)
            continue
        call.append(e0.elapsed_ms(e1))
        for k in scopes:
            kern[k].append(capi.timing_read(k)[0])
    return call, kern


def run(kind, n, leaf, steps, thetas, direct_max, nsample, nmodel, nexact):
    pts = synth.uniform(n) if kind == "uniform" else synth.lognormal(n)
    d = hip.DeviceArray.from_numpy(pts)
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, stream=s.handle)
    rng = np.random.default_rng(30)
    rows = np.sort(rng.choice(n, min(nsample, n), replace=False))
    mrows = rows[:: max(1, len(rows) // nmodel)][:nmodel]
    sample = np.ascontiguousarray(pts[rows])
    a64 = direct64(pts, sample[:nexact])
    del pts
    model = Model(t, n)
    phi = hip.DeviceArray((n,), np.float32)
    acc = hip.DeviceArray((n, 3), np.float32)
    # theta = 0 on the sample rows: the reference accelerations
    ds = hip.DeviceArray.from_numpy(sample)
    a0d = hip.DeviceArray((len(rows), 3), np.float32)
    t.gravity_device(ds.ptr, len(rows), None, 0.0, 0.0, None, a0d.ptr, stream=s.handle)
    s.synchronize()
    a0 = a0d.numpy().astype(np.float64)
    ref_rms, ref_max = rel_err(a0[:nexact], a64)
    hr = hip.DeviceArray((n,), np.float32)
    out1 = hip.DeviceArray((n,), np.float32)
    cnt = hip.DeviceArray((n,), np.uint32)
    res = {"input": kind, "n": n, "leafsize": leaf, "steps": steps, "nodes": int(t.size),
           "sample_rows": len(rows), "model_rows": len(mrows), "exact_rows": len(a64),
           "theta0_sample_rel_err_vs_f64_rms": ref_rms,
           "theta0_sample_rel_err_vs_f64_max": ref_max, "rows": []}
    capi.timing_enable(True)
    try:
        for theta in thetas:
            if theta == 0.0 and n > direct_max:
                continue
            label = f"{kind} n={n:.0e} theta={theta}"
            call, kern = timed(lambda: t.gravity_device(d.ptr, n, None, theta, 0.0, phi.ptr,
                                                        acc.ptr, stream=s.handle),
                               ("gravity_moments", "gravity_walk"), s, steps, label)
            a = acc.numpy()[rows].astype(np.float64)
            rms0, max0 = rel_err(a, a0)
            rms64, max64 = rel_err(a[:nexact], a64)
            if not np.all(np.isfinite(a)) or not np.all(phi.numpy_head(1000) < 0):
                raise RuntimeError(f"{label}: results that are not finite and negative")
            mono, pnt = model.terms(sample[np.searchsorted(rows, mrows)], theta)
            row = {"theta": theta, "call": stats(call), "moments": stats(kern["gravity_moments"]),
                   "walk": stats(kern["gravity_walk"]),
                   "mean_monopole_terms": float(mono.mean()),
                   "mean_point_terms": float(pnt.mean()),
                   "acc_rel_err_rms": rms0, "acc_rel_err_max": max0,
                   "acc_rel_err_vs_f64_rms": rms64, "acc_rel_err_vs_f64_max": max64}
            # kernel_sum, top-hat, at the radius holding as many points on average
            want = min(max(row["mean_point_terms"], 1.0), float(n))
            r = (want / (4.0 / 3.0 * math.pi * n)) ** (1.0 / 3.0)
            for _ in range(3):
                hr_np = np.full(n, r, np.float32)
                hip.memcpy(hr.ptr, hr_np.ctypes.data, hr_np.nbytes, hip.H2D)
                t.ball_sum_device(d.ptr, n, hr.ptr, None, 1, capi.KERNEL_TOPHAT, None, cnt.ptr,
                                  stream=s.handle)
                s.synchronize()
                have = float(cnt.numpy().mean(dtype=np.float64))
                if abs(have - want) <= 0.02 * want:
                    break
                r *= (want / max(have, 1.0)) ** (1.0 / 3.0)
            kc, kk = timed(lambda: t.ball_sum_device(d.ptr, n, hr.ptr, None, 1, capi.KERNEL_TOPHAT,
                                                     out1.ptr, None, stream=s.handle),
                           ("ball_sum",), s, steps, label + " kernel_sum")
            row["kernel_sum_tophat"] = {"r": r, "mean_neighbours": have, "call": stats(kc),
                                        "kernel": stats(kk["ball_sum"])}
            res["rows"].append(row)
            print(f"{label}: call {row['call']['median_ms']:.2f} ms, moments "
                  f"{row['moments']['median_ms']:.3f}, walk {row['walk']['median_ms']:.2f}; terms "
                  f"{row['mean_monopole_terms']:.0f} + {row['mean_point_terms']:.0f}; acc error rms "
                  f"{row['acc_rel_err_rms']:.2e} max {row['acc_rel_err_max']:.2e} (against float64: "
                  f"{rms64:.2e}, {max64:.2e}); kernel_sum "
                  f"top-hat at {have:.0f} neighbours {row['kernel_sum_tophat']['kernel']['median_ms']:.2f} ms",
                  flush=True)
    finally:
        capi.timing_enable(False)
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e5, 1e6, 1e7])
    ap.add_argument("--lognormal", type=float, default=1e6, help="0: skip")
    ap.add_argument("--thetas", type=float, nargs="*", default=[0.0, 0.3, 0.5, 0.7])
    ap.add_argument("--direct-max", type=float, default=1e5)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--model-rows", type=int, default=100)
    ap.add_argument("--exact-rows", type=int, default=32)
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gravity.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    args = (a.leaf, a.steps, a.thetas, a.direct_max, a.sample, a.model_rows, a.exact_rows)
    runs = [run("uniform", int(n), *args) for n in a.n]
    if a.lognormal:
        runs.append(run("lognormal", int(a.lognormal), *args))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"runs": runs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
