"""Radial profiles (nbkd_query_ball_profile) against the routes to the same
numbers: periodic uniform points at --n and the log-normal set at --lognormal,
leafsize 64, the tree's own points as queries (device I/O), nr = 16 geometric
radii up to 0.01 L.  Per input:
  (a) profile, values = None (counts),
  (b) profile, one real channel,
  (c) profile, four channels,
  (d) (b) with per-query scales = the 32nd-neighbour distance over its mean,
beside ball_hist at the same radii (which only counts), one top-hat ball_sum at
the largest radius (the floor of this walk) and, with --parent-lib, the only
route an earlier library offers for (b)'s numbers: 16 top-hat ball_sum calls at
those radii, timed on that library in the same process.  One process,
interleaved rounds (every operation once per round), a warm-up round, then
--steps rounds: HIP events time the calls, the library's event timers the
kernels; medians, min and max are reported.  so_mass is timed on --so-centres
centres (host arrays, refine = 1) with the wall clock.

Acceptance (written down, not asserted in tests): (b)'s call median must lie
below the 16 calls' median by more than their own max - min.

Writes --out (default profiles/ball_profile.json)."""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402

NR = 16


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def load_capi(lib_path):
    """a second copy of the ctypes binding over another build of the library"""
    spec = importlib.util.spec_from_file_location("nbodyhpc_amd_capi_other", capi.__file__)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(lib_path)
    # an earlier build lacks the symbols added since
    have = ctypes.CDLL(mod.LIB_PATH)
    mod._PROTOS = {k: v for k, v in mod._PROTOS.items() if hasattr(have, k)}
    return mod


def run(kind, n, leaf, steps, parent, so_centres):
    pts = synth.uniform(n) if kind == "uniform" else synth.lognormal(n)
    d = hip.DeviceArray.from_numpy(pts)
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0, stream=s.handle)
    radii = np.geomspace(0.0005, 0.01, NR).astype(np.float32)
    rng = np.random.default_rng(20)
    hk = hip.DeviceArray((n,), np.float32)
    t.query_kth_device(d.ptr, n, 32, hk.ptr, stream=s.handle)
    s.synchronize()
    k32 = hk.numpy()
    scale = hip.DeviceArray.from_numpy((k32 / k32.mean(dtype=np.float64)).astype(np.float32))
    v4 = hip.DeviceArray.from_numpy((0.5 + 1.5 * rng.random((n, 4))).astype(np.float32))
    out1 = hip.DeviceArray((n, NR), np.float32)
    outb = hip.DeviceArray((n, NR), np.float32)
    out4 = hip.DeviceArray((n, NR, 4), np.float32)
    hist = hip.DeviceArray((n, NR), np.uint32)
    hmax = hip.DeviceArray.from_numpy(np.full(n, radii[-1], np.float32))
    sum1 = hip.DeviceArray((n,), np.float32)
    ops = {
        "a_counts": ("ball_profile", lambda: t.ball_profile_device(
            d.ptr, n, radii, None, None, 1, out1.ptr, stream=s.handle)),
        "b_nv1": ("ball_profile", lambda: t.ball_profile_device(
            d.ptr, n, radii, None, v4.ptr, 1, outb.ptr, stream=s.handle)),
        "c_nv4": ("ball_profile", lambda: t.ball_profile_device(
            d.ptr, n, radii, None, v4.ptr, 4, out4.ptr, stream=s.handle)),
        "d_nv1_scaled": ("ball_profile", lambda: t.ball_profile_device(
            d.ptr, n, radii, scale.ptr, v4.ptr, 1, out1.ptr, stream=s.handle)),
        "ball_hist": ("ball_hist", lambda: t.ball_hist_device(
            d.ptr, n, radii, hist.ptr, total=False, stream=s.handle)),
        "ball_sum_rmax": ("ball_sum", lambda: t.ball_sum_device(
            d.ptr, n, hmax.ptr, v4.ptr, 1, capi.KERNEL_TOPHAT, sum1.ptr, None, stream=s.handle)),
    }
    # ((b) and (d) read v4 as an (n, 1) array, its first n floats: any values do)
    if parent is not None:
        pt = parent.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0, stream=s.handle)
        hr = [hip.DeviceArray.from_numpy(np.full(n, r, np.float32)) for r in radii]
        sums = hip.DeviceArray((NR, n), np.float32)

        def sixteen():
            for k in range(NR):
                pt.ball_sum_device(d.ptr, n, hr[k].ptr, v4.ptr, 1, parent.KERNEL_TOPHAT,
                                   sums.ptr + 4 * n * k, None, stream=s.handle)

        ops["parent_16_ball_sum"] = ("ball_sum", sixteen)
    call = {k: [] for k in ops}
    kern = {k: [] for k in ops}
    for c in (capi, parent):
        if c is not None:
            c.timing_enable(True)
    try:
        for rnd in range(steps + 1):  # round 0 warms up (the workspace grows there)
            for k, (scope, fn) in ops.items():
                lib = parent if k.startswith("parent") else capi
                lib.timing_reset()
                e0, e1 = hip.Event(), hip.Event()
                e0.record(s.handle)
                fn()
                e1.record(s.handle)
                s.synchronize()
                if rnd == 0:
                    print(f"{kind} n={n:.0e}: warmed up {k}", flush=True)
                    continue
                call[k].append(e0.elapsed_ms(e1))
                kern[k].append(lib.timing_read(scope)[0])
    finally:
        for c in (capi, parent):
            if c is not None:
                c.timing_enable(False)
    res = {"input": kind, "n": n, "leafsize": leaf, "nr": NR, "radii": [float(r) for r in radii],
           "steps": steps, "mean_k32": float(k32.mean(dtype=np.float64))}
    # (a) against the histogram it claims to equal, (b) against the 16 sums
    head = 100000
    ops["a_counts"][1]()  # ((d) wrote out1 last)
    s.synchronize()
    a_run = np.cumsum(out1.numpy_head(head).astype(np.float64), axis=1)
    if not np.array_equal(a_run, hist.numpy_head(head).astype(np.float64)):
        raise RuntimeError(f"{kind} n={n}: the running sum of (a) differs from ball_hist")
    res["mean_neighbours_at_rmax"] = float(a_run[:, -1].mean())
    b_run = np.cumsum(outb.numpy_head(head).astype(np.float64), axis=1)
    if parent is not None:
        ref = sums.numpy()[:, :head].T.astype(np.float64)
        if not np.allclose(b_run, ref, rtol=1e-5, atol=0):
            raise RuntimeError(f"{kind} n={n}: the running sum of (b) differs from the 16 sums")
    for k in ops:
        res[k] = {"call": stats(call[k]), "kernel": stats(kern[k]), "kernel_scope": ops[k][0]}
    for k in ("a_counts", "b_nv1", "c_nv4", "d_nv1_scaled"):
        res[k]["kernel_over_ball_hist"] = (res[k]["kernel"]["median_ms"]
                                           / res["ball_hist"]["kernel"]["median_ms"])
        res[k]["kernel_over_ball_sum_rmax"] = (res[k]["kernel"]["median_ms"]
                                               / res["ball_sum_rmax"]["kernel"]["median_ms"])
    msg = (f"{kind} n={n:.0e} ({res['mean_neighbours_at_rmax']:.1f} neighbours at r_max): profile "
           f"kernel ms (a) {res['a_counts']['kernel']['median_ms']:.2f} (b) "
           f"{res['b_nv1']['kernel']['median_ms']:.2f} (c) {res['c_nv4']['kernel']['median_ms']:.2f} "
           f"(d) {res['d_nv1_scaled']['kernel']['median_ms']:.2f}; ball_hist "
           f"{res['ball_hist']['kernel']['median_ms']:.2f}; ball_sum at r_max "
           f"{res['ball_sum_rmax']['kernel']['median_ms']:.2f}")
    if parent is not None:
        p, b = res["parent_16_ball_sum"]["call"], res["b_nv1"]["call"]
        res["acceptance_b_below_parent_by_more_than_spread"] = bool(
            p["median_ms"] - b["median_ms"] > p["max_ms"] - p["min_ms"])
        msg += (f"; (b) call {b['median_ms']:.2f} against 16 ball_sum calls {p['median_ms']:.2f} "
                f"(min {p['min_ms']:.2f}, max {p['max_ms']:.2f}): acceptance "
                f"{res['acceptance_b_below_parent_by_more_than_spread']}")
        pt.close()
    print(msg, flush=True)
    t.close()
    for a in (out1, outb, out4, hist, hmax, sum1, scale, hk, v4, d):
        a.free()
    if so_centres:
        from nbodyhpc_amd.kdtree import KDTree
        kt = KDTree(pts, leafsize=leaf, boxsize=1.0)
        centres = pts[:so_centres]
        kt.so_mass(centres[:1000], 200.0 * n, 0.02)  # warm-up
        t0 = time.perf_counter()
        so = kt.so_mass(centres, 200.0 * n, 0.02, refine=1)
        res["so_mass"] = {"centres": int(so_centres), "overdensity": 200.0 * n, "r_max": 0.02,
                          "refine": 1, "wall_ms": 1e3 * (time.perf_counter() - t0),
                          "status_counts": [int((so["status"] == v).sum()) for v in (0, 1, 2)]}
        print(f"{kind} n={n:.0e}: so_mass of {so_centres} centres {res['so_mass']['wall_ms']:.1f} ms,"
              f" status counts {res['so_mass']['status_counts']}", flush=True)
        del kt
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e7])
    ap.add_argument("--lognormal", type=float, default=1e7, help="0: skip")
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--so-centres", type=float, default=1e5, help="0: skip")
    ap.add_argument("--parent-lib", default=None,
                    help="libnbkd.so of an earlier commit: the 16 ball_sum calls run on it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_profile.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    parent = load_capi(a.parent_lib) if a.parent_lib else None
    runs = [run("uniform", int(n), a.leaf, a.steps, parent, int(a.so_centres)) for n in a.n]
    if a.lognormal:
        runs.append(run("lognormal", int(a.lognormal), a.leaf, a.steps, parent, int(a.so_centres)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"parent_lib": bool(parent), "runs": runs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
