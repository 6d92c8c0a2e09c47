"""Friends-of-friends (nbkd_fof) against the two existing walks with the same
bound: uniform periodic points at each --n (and the log-normal set at
--lognormal), leafsize 64, b = 0.2 n^(-1/3) L, device outputs.  Per input,
after a warm-up of everything, HIP events time
  (a) one fof call (labels and sizes),
  (b) one ball_count of the tree's own points at r = b,
each `--steps` times (the median is reported); the library's event timers give
the per-kernel split (fof_hook / fof_flatten / fof_label, ball_count) and, up
to --csr-max points, the CSR fill pass at r = b (ball_fill).  The number of
groups and the largest group come from one host-output call.  At --check
uniform points the labels are compared once with ball_csr plus a host
connected-components pass.

--ab: the halving-store A/B (plain store / relaxed atomic store / atomicMin),
interleaved rounds in this one process, at the linking lengths --ab-f (in
mean spacings: 0.2 barely links, 0.9 is past percolation).  It needs the
experiments build, `python -m nbodyhpc_amd.build --experiments`, loaded through
NBKD_LIB=nbodyhpc_amd/lib/exp/libnbkd.so, where NBKD_FOF_HALVE selects the
variant per call.

One process; writes the numbers to --out (default profiles/fof.json; with --ab
the "halving_ab" entry of that file is replaced, the rest kept)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402

HALVE = {"plain_store": "0", "atomic_store": "1", "atomic_min": "2"}


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


def kernel_ms(names, stream, steps, fn):
    """per-launch mean of the library's event timers over `steps` runs of fn()"""
    capi.timing_enable(True)
    try:
        capi.timing_reset()
        for _ in range(steps):
            fn()
        stream.synchronize()
        out = {}
        for nm in names:
            ms, cnt = capi.timing_read(nm)
            out[nm] = {"ms_per_call": ms / steps, "launches_per_call": cnt / steps}
        return out
    finally:
        capi.timing_enable(False)


def host_components(off, idx, n):
    """smallest member of each connected component of the CSR graph"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off.astype(np.int64)))
    cols = idx.astype(np.int64)
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = lab.copy()
        np.minimum.at(m, rows, lab[cols])
        m = m[m]
        if np.array_equal(m, lab):
            return lab.astype(np.uint32)
        lab = m


def check_against_csr(n, leaf):
    pts = synth.uniform(n)
    b = 0.2 * n ** (-1.0 / 3.0)
    t = capi.Tree(pts, leafsize=leaf, boxsize=1.0)
    lab, siz, ng = t.fof(b)
    off, idx = t.ball_csr(pts, b)
    ref = host_components(off, idx, n)
    t.close()
    if not np.array_equal(lab, ref):
        raise RuntimeError(f"n={n}: fof labels differ from ball_csr + host components at "
                           f"{int((lab != ref).sum())} rows")
    if not np.array_equal(siz, np.bincount(ref, minlength=n)) or ng != len(np.unique(ref)):
        raise RuntimeError(f"n={n}: fof sizes / ngroups differ from the host components")
    print(f"check n={n:.0e}: labels, sizes and ngroups ({ng}) equal ball_csr + host "
          f"connected components", flush=True)
    return {"n": n, "b": b, "ngroups": int(ng), "equal": True}


def setup(kind, n, leaf):
    pts = synth.uniform(n) if kind == "uniform" else synth.lognormal(n)
    d = hip.DeviceArray.from_numpy(pts)
    del pts
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, boxsize=1.0, stream=s.handle)
    return d, s, t


def run(kind, n, leaf, steps, csr_max):
    d, s, t = setup(kind, n, leaf)
    b = 0.2 * n ** (-1.0 / 3.0)
    lab = hip.DeviceArray((n,), np.uint32)
    siz = hip.DeviceArray((n,), np.uint32)
    cnt = hip.DeviceArray((n,), np.uint32)

    def fof():
        t.fof_device(b, lab.ptr, siz.ptr, stream=s.handle)

    def count():
        t.ball_count_device(d.ptr, n, b, cnt.ptr, s.handle)

    # warm-up (the workspace grows here) and the group statistics
    hl, hs, ng = t.fof(b)
    fof()
    count()
    s.synchronize()
    if not np.array_equal(lab.numpy(), hl) or not np.array_equal(siz.numpy(), hs):
        raise RuntimeError(f"{kind} n={n}: device outputs differ from the host outputs")
    largest = int(hs.max())
    npairs = (int(cnt.numpy().sum(dtype=np.uint64)) - n) // 2
    del hl, hs
    a = timed(s, steps, fof)
    c = timed(s, steps, count)
    s.synchronize()
    ka = kernel_ms(("fof_hook", "fof_flatten", "fof_label"), s, steps, fof)
    kc = kernel_ms(("ball_count",), s, steps, count)
    fof_k = sum(v["ms_per_call"] for v in ka.values())
    res = {"input": kind, "n": n, "leafsize": leaf, "b": b, "steps": steps,
           "ngroups": int(ng), "largest_group": largest, "friend_pairs": npairs,
           "fof_call": a, "ball_count_call": c, "fof_kernels": ka,
           "fof_kernels_ms": fof_k, "ball_count_kernel": kc["ball_count"],
           "fof_over_count_call": a["median_ms"] / c["median_ms"],
           "fof_over_count_kernels": fof_k / kc["ball_count"]["ms_per_call"]}
    msg = (f"{kind} n={n:.0e}: fof {a['median_ms']:.2f} ms (hook "
           f"{ka['fof_hook']['ms_per_call']:.2f}, flatten {ka['fof_flatten']['ms_per_call']:.2f}, "
           f"label {ka['fof_label']['ms_per_call']:.2f}), ball_count {c['median_ms']:.2f} ms "
           f"(kernel {kc['ball_count']['ms_per_call']:.2f}); {ng} groups, largest {largest}")
    if n <= csr_max:
        off = np.empty(n + 1, np.uint64)
        t.ball_csr_device(d.ptr, n, b, off, None, 0, stream=s.handle)
        nnz = int(off[-1])
        ids = hip.DeviceArray((nnz,), np.uint32)

        def csr():
            t.ball_csr_device(d.ptr, n, b, off, ids.ptr, nnz, stream=s.handle)

        csr()
        kf = kernel_ms(("ball_fill",), s, steps, csr)
        res["ball_csr_fill_kernel"] = kf["ball_fill"]
        res["ball_csr_ids"] = nnz
        res["fof_over_csr_fill_kernels"] = fof_k / kf["ball_fill"]["ms_per_call"]
        res["hook_over_csr_fill"] = ka["fof_hook"]["ms_per_call"] / kf["ball_fill"]["ms_per_call"]
        msg += (f"; CSR fill {kf['ball_fill']['ms_per_call']:.2f} ms, fof/fill "
                f"{res['fof_over_csr_fill_kernels']:.2f}")
    print(msg, flush=True)
    t.close()
    return res


def halving_ab(n, leaf, rounds, factors):
    if not os.environ.get("NBKD_LIB"):
        raise SystemExit("--ab needs the experiments build loaded through NBKD_LIB")
    res = {"n": n, "leafsize": leaf, "rounds": rounds, "inputs": {}}
    for kind, f in [(k, f) for k in ("uniform", "lognormal") for f in factors]:
        d, s, t = setup(kind, n, leaf)
        b = f * n ** (-1.0 / 3.0)
        lab = hip.DeviceArray((n,), np.uint32)
        ref = None
        ms = {k: [] for k in HALVE}
        capi.timing_enable(True)
        try:
            for r in range(rounds + 1):  # round 0 warms up
                for k, v in HALVE.items():
                    os.environ["NBKD_FOF_HALVE"] = v
                    capi.timing_reset()
                    t.fof_device(b, lab.ptr, None, stream=s.handle)
                    s.synchronize()
                    if r == 0:
                        got = lab.numpy()
                        if ref is None:
                            ref = got
                        elif not np.array_equal(got, ref):
                            raise RuntimeError(f"halving variant {k} gives other labels")
                    else:
                        ms[k].append(capi.timing_read("fof_hook")[0])
        finally:
            capi.timing_enable(False)
            os.environ.pop("NBKD_FOF_HALVE", None)
        _, hs, ng = t.fof(b)
        res["inputs"][f"{kind}, b = {f} n^(-1/3)"] = dict(
            {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v))}
             for k, v in ms.items()}, ngroups=int(ng), largest_group=int(hs.max()))
        print(f"halving A/B, {kind} n={n:.0e}, b = {f} n^(-1/3) ({ng} groups, largest "
              f"{int(hs.max())}), fof_hook ms: " +
              ", ".join(f"{k} {np.median(v):.2f} (min {min(v):.2f})" for k, v in ms.items()),
              flush=True)
        t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e7, 1e8])
    ap.add_argument("--lognormal", type=float, default=1e7, help="0: skip")
    ap.add_argument("--check", type=float, default=1e6, help="0: skip")
    ap.add_argument("--csr-max", type=float, default=1e7)
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--ab-n", type=float, default=1e7)
    ap.add_argument("--ab-f", type=float, nargs="+", default=[0.2, 0.9],
                    help="linking lengths of the A/B in mean spacings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fof.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    if a.ab:
        out["halving_ab"] = halving_ab(int(a.ab_n), a.leaf, max(a.steps, 5), a.ab_f)
    else:
        keep = out.get("halving_ab")
        out = {"check": check_against_csr(int(a.check), a.leaf) if a.check else None,
               "runs": [run("uniform", int(n), a.leaf, a.steps, a.csr_max) for n in a.n]}
        if a.lognormal:
            out["runs"].append(run("lognormal", int(a.lognormal), a.leaf, a.steps, a.csr_max))
        if keep:
            out["halving_ab"] = keep
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
