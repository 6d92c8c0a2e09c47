"""Kernel-weighted sums (nbkd_query_ball_sum) against the two existing walks at
the same radius: periodic uniform points at each --n (and the log-normal set
at --lognormal), leafsize 64, the tree's own points as queries (device I/O).
Per input, with r the radius that holds 32 points on average and
h_k = query_kth(k = 32):
  (a) ball_sum, top-hat, nv = 1, every h_i = r,
  (b) ball_sum, cubic spline, nv = 1, h_i = h_k,
  (c) the same with nv = 4,
beside ball_count at r and, while the id list stays below --csr-max-ids, the
CSR route at r, whose fill pass (ball_fill) is the only way to the same numbers
without ball_sum, before any summing on the host.  One process, interleaved
rounds (every operation once per round), a warm-up round, then --steps rounds:
HIP events time the calls, the library's event timers the kernels; medians, min
and max are reported.

Acceptance (written down, not asserted in tests): row (a)'s ball_sum kernel
median must not exceed the ball_fill median of the same run by more than
ball_fill's own max - min.

Writes --out (default profiles/ball_sum.json)."""
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


def run(kind, n, leaf, steps, csr_max_ids):
    pts = synth.uniform(n) if kind == "uniform" else synth.lognormal(n)
    d = hip.DeviceArray.from_numpy(pts)
    del pts
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0, stream=s.handle)
    r = (32.0 / (4.0 / 3.0 * math.pi * n)) ** (1.0 / 3.0)
    rng = np.random.default_rng(20)
    hr = hip.DeviceArray.from_numpy(np.full(n, r, np.float32))
    hk = hip.DeviceArray((n,), np.float32)
    t.query_kth_device(d.ptr, n, 32, hk.ptr, stream=s.handle)
    v4 = hip.DeviceArray.from_numpy((0.5 + 1.5 * rng.random((n, 4))).astype(np.float32))
    out1 = hip.DeviceArray((n,), np.float32)
    out4 = hip.DeviceArray((n, 4), np.float32)
    cnt = hip.DeviceArray((n,), np.uint32)
    cnt2 = hip.DeviceArray((n,), np.uint32)
    TOPHAT, CUBIC = capi.KERNEL_TOPHAT, capi.KERNEL_CUBIC
    ops = {
        "a_tophat_nv1_r": ("ball_sum", lambda: t.ball_sum_device(
            d.ptr, n, hr.ptr, None, 1, TOPHAT, out1.ptr, cnt2.ptr, stream=s.handle)),
        "b_cubic_nv1_hk": ("ball_sum", lambda: t.ball_sum_device(
            d.ptr, n, hk.ptr, v4.ptr, 1, CUBIC, out1.ptr, None, stream=s.handle)),
        "c_cubic_nv4_hk": ("ball_sum", lambda: t.ball_sum_device(
            d.ptr, n, hk.ptr, v4.ptr, 4, CUBIC, out4.ptr, None, stream=s.handle)),
        "ball_count_r": ("ball_count", lambda: t.ball_count_device(d.ptr, n, r, cnt.ptr, s.handle)),
    }
    # ((b) reads v4 as an (n, 1) array, its first n floats: any values do)
    ops["ball_count_r"][1]()
    s.synchronize()
    nnz = int(cnt.numpy().sum(dtype=np.uint64))
    res = {"input": kind, "n": n, "leafsize": leaf, "r": r, "steps": steps, "ids_at_r": nnz,
           "mean_neighbours_at_r": nnz / n, "mean_hk": float(hk.numpy().mean(dtype=np.float64))}
    if nnz <= csr_max_ids:
        off = np.empty(n + 1, np.uint64)
        ids = hip.DeviceArray((nnz,), np.uint32)
        ops["csr_r"] = ("ball_fill", lambda: t.ball_csr_device(d.ptr, n, r, off, ids.ptr, nnz,
                                                               stream=s.handle))
    else:
        res["csr_r"] = f"skipped: {nnz} ids exceed --csr-max-ids"
    call = {k: [] for k in ops}
    kern = {k: [] for k in ops}
    gather = []
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
                if k == "c_cubic_nv4_hk":
                    gather.append(capi.timing_read("ball_sum_gather")[0])
    finally:
        capi.timing_enable(False)
    # (a) against the count it claims to equal
    if not np.array_equal(cnt2.numpy(), cnt.numpy()):
        raise RuntimeError(f"{kind} n={n}: ball_sum's count at h = r differs from ball_count")
    if not np.all(np.isfinite(out4.numpy())) or not np.all(out4.numpy_head(1000) > 0):
        raise RuntimeError(f"{kind} n={n}: sums that are not finite and positive")
    for k in ops:
        res[k] = {"call": stats(call[k]), "kernel": stats(kern[k]), "kernel_scope": ops[k][0]}
    res["gather_nv4_kernel"] = stats(gather)
    cm = res["ball_count_r"]["kernel"]["median_ms"]
    for k in ("a_tophat_nv1_r", "b_cubic_nv1_hk", "c_cubic_nv4_hk"):
        res[k]["kernel_over_ball_count"] = res[k]["kernel"]["median_ms"] / cm
    msg = (f"{kind} n={n:.0e} ({nnz / n:.1f} neighbours at r): ball_sum kernel ms (a) "
           f"{res['a_tophat_nv1_r']['kernel']['median_ms']:.2f} (b) "
           f"{res['b_cubic_nv1_hk']['kernel']['median_ms']:.2f} (c) "
           f"{res['c_cubic_nv4_hk']['kernel']['median_ms']:.2f}; ball_count {cm:.2f}")
    if "csr_r" in ops:
        f = res["csr_r"]["kernel"]
        a = res["a_tophat_nv1_r"]["kernel"]["median_ms"]
        for k in ("a_tophat_nv1_r", "b_cubic_nv1_hk", "c_cubic_nv4_hk"):
            res[k]["kernel_over_ball_fill"] = res[k]["kernel"]["median_ms"] / f["median_ms"]
        res["acceptance_a_le_fill_plus_spread"] = bool(
            a <= f["median_ms"] + (f["max_ms"] - f["min_ms"]))
        msg += (f"; ball_fill {f['median_ms']:.2f} (min {f['min_ms']:.2f}, max {f['max_ms']:.2f})"
                f"; acceptance {res['acceptance_a_le_fill_plus_spread']}")
    print(msg, flush=True)
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e7])
    ap.add_argument("--lognormal", type=float, default=1e7, help="0: skip")
    ap.add_argument("--csr-max-ids", type=float, default=6e9)
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_sum.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    runs = [run("uniform", int(n), a.leaf, a.steps, a.csr_max_ids) for n in a.n]
    if a.lognormal:
        runs.append(run("lognormal", int(a.lognormal), a.leaf, a.steps, a.csr_max_ids))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"runs": runs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
