"""Anisotropic pair counts (nbkd_query_ball_hist2) against the earlier routes to
pair information: periodic uniform points at --n and the log-normal set at
--lognormal, leafsize 64, the tree's own points as device queries.  Per input:
  (a) SMU, 16 geometric s edges 0.0005 L .. 0.01 L, nmu = 1,
  (b) the same s edges, nmu = 16,
  (c) RPPI, 16 x 16, the same edges as rp, pi_max = rp_max = 0.01 L,
  (d) RPPI, 16 x 40, pi_max = 0.04 L (the elongated cylinder leaf pruning is for),
beside two yardsticks that run on --parent-lib when given (an earlier commit's
library loaded into the same process), else on this library: ball_hist at the
same s edges (totals only) and the whole nbkd_query_ball_csr call at r = s_max
(device queries, device ids, unsorted; its capacity comes from the warm-up's
counts pass, which is not timed).  One process, interleaved rounds (every
operation once per round), a warm-up round, then --steps rounds: HIP events time
the calls, the library's event timers the kernels; medians, min and max are
reported.  --copies-sweep also times (b) and (c) with 1, 2, 4 and 8 interleaved
LDS copies of the wave's histogram (nbkd_set_tuning("hist2_copies")), in
interleaved rounds of their own with the same warm-up and repetitions.
--only KEY ... runs just those operations once per round without the
yardsticks and checks, with --copies N interleaved copies: the form the
counter passes (rocprofv3 --pmc, runs of their own) profile.

Asserted here: (a) equals the differenced ball_hist totals, (b) summed over mu
equals (a), every copies setting gives the default's counts.
Acceptance (written down, not asserted): (b)'s call median lies below the CSR
call's median by more than the CSR call's own max - min.

Writes --out (default profiles/ball_hist2.json)."""
import argparse
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402

N1 = 16
S_MIN, S_MAX, PI_LONG = 0.0005, 0.01, 0.04


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


def run(kind, n, leaf, steps, parent, sweep, only=None, copies=0):
    pts = synth.uniform(n) if kind == "uniform" else synth.lognormal(n)
    d = hip.DeviceArray.from_numpy(pts)
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0, stream=s.handle)
    yard = parent if parent is not None else capi
    yt = t if parent is None else parent.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0,
                                              stream=s.handle)
    edges = np.geomspace(S_MIN, S_MAX, N1).astype(np.float32)
    mu1 = np.array([1.0], np.float32)
    mu16 = ((np.arange(16) + 1.0) / 16).astype(np.float32)
    pi16 = (S_MAX * (np.arange(16) + 1.0) / 16).astype(np.float32)
    pi40 = (PI_LONG * (np.arange(40) + 1.0) / 40).astype(np.float32)
    if only:  # the counter passes: just these operations, no yardsticks, no checks
        capi.set_tuning("hist2_copies", copies)
        e2 = {"a_smu_nmu1": (mu1, capi.NBKD_HIST2_SMU), "b_smu_nmu16": (mu16, capi.NBKD_HIST2_SMU),
              "c_rppi_16x16": (pi16, capi.NBKD_HIST2_RPPI),
              "d_rppi_16x40": (pi40, capi.NBKD_HIST2_RPPI)}
        for _ in range(steps + 1):
            for k in only:
                t.ball_hist2_device(d.ptr, n, edges, e2[k][0], e2[k][1], 2, stream=s.handle)
        capi.set_tuning("hist2_copies", 0)
        t.close()
        d.free()
        return {"input": kind, "n": n, "only": list(only), "copies": copies}
    # the CSR call's capacity: the counts pass (not timed)
    off = np.empty(n + 1, np.uint64)
    yt.ball_csr_device(d.ptr, n, float(edges[-1]), off, None, 0, stream=s.handle)
    cap = int(off[-1])
    ids = hip.DeviceArray((cap,), np.uint32)
    got = {}

    def h2(key, e2, mode):
        def fn():
            got[key] = t.ball_hist2_device(d.ptr, n, edges, e2, mode, 2, stream=s.handle)
        return fn

    def hist():
        got["ball_hist"] = yt.ball_hist_device(d.ptr, n, edges, None, stream=s.handle)

    ops = {
        "a_smu_nmu1": ("ball_hist2", h2("a", mu1, capi.NBKD_HIST2_SMU)),
        "b_smu_nmu16": ("ball_hist2", h2("b", mu16, capi.NBKD_HIST2_SMU)),
        "c_rppi_16x16": ("ball_hist2", h2("c", pi16, capi.NBKD_HIST2_RPPI)),
        "d_rppi_16x40": ("ball_hist2", h2("d", pi40, capi.NBKD_HIST2_RPPI)),
        "yard_ball_hist": ("ball_hist", hist),
        "yard_ball_csr": (None, lambda: yt.ball_csr_device(d.ptr, n, float(edges[-1]), off,
                                                           ids.ptr, cap, stream=s.handle)),
    }
    call = {k: [] for k in ops}
    kern = {k: [] for k in ops}
    libs = {capi, yard}
    for c in libs:
        c.timing_enable(True)
    try:
        for rnd in range(steps + 1):  # round 0 warms up (the workspace grows there)
            for k, (scope, fn) in ops.items():
                lib = yard if k.startswith("yard") else capi
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
                if scope:
                    kern[k].append(lib.timing_read(scope)[0])
        want = np.diff(got["ball_hist"].astype(np.int64), prepend=0).astype(np.uint64)
        if not np.array_equal(got["a"][:, 0], want):
            raise RuntimeError(f"{kind} n={n}: (a) differs from the differenced ball_hist totals")
        if not np.array_equal(got["b"].sum(axis=1), got["a"][:, 0]):
            raise RuntimeError(f"{kind} n={n}: (b) summed over mu differs from (a)")
        if int(got["ball_hist"][-1]) != cap:
            raise RuntimeError(f"{kind} n={n}: the CSR length differs from ball_hist's last total")
        res = {"input": kind, "n": n, "leafsize": leaf, "steps": steps,
               "s_edges": [float(e) for e in edges], "pairs_within_s_max": cap,
               "yardsticks_on_parent_lib": parent is not None}
        for k in ops:
            res[k] = {"call": stats(call[k])}
            if ops[k][0]:
                res[k]["kernel"] = stats(kern[k])
                res[k]["kernel_scope"] = ops[k][0]
        for k, key in (("c_rppi_16x16", "c"), ("d_rppi_16x40", "d")):
            res[k]["pairs_counted"] = int(got[key].sum())
        if sweep:
            # as the main rows: interleaved rounds over the settings, a warm-up
            # round, then `steps` rounds; kernel times
            res["copies_sweep"] = {}
            keys = ("b_smu_nmu16", "c_rppi_16x16")
            ref = {k: got[k[0]].copy() for k in keys}
            ms = {k: {c: [] for c in (1, 2, 4, 8)} for k in keys}
            for rnd in range(steps + 1):
                for copies in (1, 2, 4, 8):
                    capi.set_tuning("hist2_copies", copies)
                    for k in keys:
                        capi.timing_reset()
                        ops[k][1]()
                        if not np.array_equal(got[k[0]], ref[k]):
                            raise RuntimeError(f"{kind}: hist2_copies = {copies} changed {k}")
                        if rnd:
                            ms[k][copies].append(capi.timing_read("ball_hist2")[0])
            capi.set_tuning("hist2_copies", 0)
            for k in keys:
                res["copies_sweep"][k] = {str(c): stats(v) for c, v in ms[k].items()}
    finally:
        capi.set_tuning("hist2_copies", 0)
        for c in libs:
            c.timing_enable(False)
    hk = res["yard_ball_hist"]["kernel"]["median_ms"]
    for k in ("a_smu_nmu1", "b_smu_nmu16", "c_rppi_16x16", "d_rppi_16x40"):
        res[k]["kernel_over_ball_hist"] = res[k]["kernel"]["median_ms"] / hk
    c, dd = res["c_rppi_16x16"], res["d_rppi_16x40"]
    ball = lambda rp, pi: (rp * rp + pi * pi) ** 1.5  # noqa: E731
    res["d_over_c"] = {"kernel": dd["kernel"]["median_ms"] / c["kernel"]["median_ms"],
                       "bounding_ball_volume": ball(S_MAX, PI_LONG) / ball(S_MAX, S_MAX),
                       "cylinder_volume": PI_LONG / S_MAX,
                       "pairs_counted": dd["pairs_counted"] / c["pairs_counted"]}
    p, b = res["yard_ball_csr"]["call"], res["b_smu_nmu16"]["call"]
    res["csr_over_b"] = p["median_ms"] / b["median_ms"]
    res["acceptance_b_below_csr_by_more_than_spread"] = bool(
        p["median_ms"] - b["median_ms"] > p["max_ms"] - p["min_ms"])
    print(f"{kind} n={n:.0e} ({cap / n:.1f} pairs per query within s_max): kernel ms "
          + " ".join(f"({k[0]}) {res[k]['kernel']['median_ms']:.2f}" for k in list(ops)[:4])
          + f"; ball_hist {hk:.2f}; (b) call {b['median_ms']:.2f} against the CSR call "
          f"{p['median_ms']:.2f} (min {p['min_ms']:.2f}, max {p['max_ms']:.2f}): acceptance "
          f"{res['acceptance_b_below_csr_by_more_than_spread']}; (d)/(c) "
          f"{res['d_over_c']['kernel']:.2f} at {res['d_over_c']['bounding_ball_volume']:.1f} times "
          "the bounding ball", flush=True)
    if yt is not t:
        yt.close()
    t.close()
    for a in (ids, d):
        a.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e7])
    ap.add_argument("--lognormal", type=float, default=1e7, help="0: skip")
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--copies-sweep", action="store_true")
    ap.add_argument("--only", nargs="*", default=None, help="operation keys, e.g. b_smu_nmu16")
    ap.add_argument("--copies", type=int, default=0, help="with --only: hist2_copies")
    ap.add_argument("--parent-lib", default=None,
                    help="libnbkd.so of an earlier commit: the yardsticks run on it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_hist2.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    parent = load_capi(a.parent_lib) if a.parent_lib else None
    runs = [run("uniform", int(n), a.leaf, a.steps, parent, a.copies_sweep, a.only, a.copies)
            for n in a.n]
    if a.lognormal:
        runs.append(run("lognormal", int(a.lognormal), a.leaf, a.steps, parent, a.copies_sweep,
                        a.only, a.copies))
    if a.only:
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"parent_lib": bool(parent), "runs": runs}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
