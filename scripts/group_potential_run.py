"""Per-group potentials (nbkd_group_potential): device inputs and outputs, one
process, HIP events, the median of `--steps` runs after a warm-up of
everything; the library's event timers give the per-kernel split
(gpot_validate / gpot_gather / gpot_sum / gpot_argmin).

(a) One group holding all --direct-n uniform non-periodic points (leafsize 64,
    unit masses, potentials and the most-bound entry), interleaved round by
    round with nbkd_gravity at theta = 0 on the same tree, potential only: the
    same n^2 terms, and the only route to these numbers before.  Accepted when
    the new call's median is not above the gravity call's median by more than
    that call's own max - min over the rounds.
(b) The friends-of-friends catalogue (b = 0.2 mean spacings) of --n uniform and
    log-normal periodic points at each --min-members: the call, its kernels and
    the sum of s^2 over the groups, with the fof and catalogue calls beside it.
    The largest group's most-bound entry is compared with an argmin on the host.

Writes the numbers to --out (default profiles/group_potential.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nbodyhpc_amd import capi, hip, synth  # noqa: E402
from scripts.fof_run import kernel_ms, setup, timed  # noqa: E402

SCOPES = ("gpot_validate", "gpot_gather", "gpot_sum", "gpot_argmin")


def once(stream, fn):
    e0, e1 = hip.Event(), hip.Event()
    e0.record(stream)
    fn()
    e1.record(stream)
    return e0.elapsed_ms(e1)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def direct(n, leaf, steps):
    pts = (synth.uniform(n) - np.float32(0.5)).astype(np.float32)
    d = hip.DeviceArray.from_numpy(pts)
    s = hip.Stream()
    t = capi.Tree(n=n, dev_ptr=d.ptr, leafsize=leaf, stream=s.handle)
    off = hip.DeviceArray.from_numpy(np.array([0, n], np.uint64))
    mem = hip.DeviceArray.from_numpy(np.arange(n, dtype=np.uint32))
    phi_g, phi_p = hip.DeviceArray((n,), np.float32), hip.DeviceArray((n,), np.float32)
    minpos = hip.DeviceArray((1,), np.uint32)

    def gravity():
        t.gravity_device(d.ptr, n, None, 0.0, 0.0, phi_g.ptr, None, stream=s.handle)

    def potential():
        t.group_potential_device(off.ptr, mem.ptr, 1, n, None, 0.0, 0, phi_p.ptr, minpos.ptr,
                                 stream=s.handle)

    gravity()
    potential()
    s.synchronize()
    # the same terms, float64 here against float32 sums there
    a, b = phi_g.numpy().astype(np.float64), phi_p.numpy().astype(np.float64)
    assert int(minpos.numpy()[0]) == int(np.argmin(phi_p.numpy()))
    tg, tp = [], []
    for _ in range(steps):
        tg.append(once(s, gravity))
        s.synchronize()
        tp.append(once(s, potential))
        s.synchronize()
    g, p = stats(tg), stats(tp)
    terms = float(n) * float(n)
    res = {"n": n, "leafsize": leaf, "steps": steps, "terms": terms,
           "gravity_theta0_phi": g, "group_potential": p,
           "gravity_terms_per_s": terms / (g["median_ms"] * 1e-3),
           "group_potential_terms_per_s": terms / (p["median_ms"] * 1e-3),
           "allowed_excess_ms": g["max_ms"] - g["min_ms"],
           "accepted": bool(p["median_ms"] <= g["median_ms"] + (g["max_ms"] - g["min_ms"])),
           "max_rel_difference_f32_sum": float(np.max(np.abs(a - b) / np.abs(b))),
           "kernels": kernel_ms(SCOPES, s, steps, potential)}
    print(f"(a) n={n:.0e}: gravity theta 0 {g['median_ms']:.2f} ms ({g['min_ms']:.2f} - "
          f"{g['max_ms']:.2f}), group_potential {p['median_ms']:.2f} ms ({p['min_ms']:.2f} - "
          f"{p['max_ms']:.2f}), sum kernel {res['kernels']['gpot_sum']['ms_per_call']:.2f} ms, "
          f"accepted {res['accepted']}", flush=True)
    t.close()
    return res


def catalogue(kind, n, leaf, steps, min_members):
    d, s, t = setup(kind, n, leaf)
    b = 0.2 * n ** (-1.0 / 3.0)
    lab, siz = hip.DeviceArray((n,), np.uint32), hip.DeviceArray((n,), np.uint32)

    def fof():
        t.fof_device(b, lab.ptr, siz.ptr, stream=s.handle)

    fof()
    s.synchronize()
    res = {"input": kind, "n": n, "leafsize": leaf, "b": b, "steps": steps,
           "fof_call": timed(s, steps, fof), "catalogs": []}
    for mm in min_members:
        G, K = t.group_catalog_device(lab.ptr, None, None, 0, mm, 0, 0, stream=s.handle)
        off = hip.DeviceArray((G + 1,), np.uint64)
        mem = hip.DeviceArray((max(K, 1),), np.uint32)

        def catalog():
            return t.group_catalog_device(lab.ptr, None, None, 0, mm, G, K, None, None, off.ptr,
                                          mem.ptr, None, None, stream=s.handle)

        if G == 0:
            off.zero()
        else:
            assert catalog() == (G, K)
        phi = hip.DeviceArray((max(K, 1),), np.float32)
        minpos = hip.DeviceArray((max(G, 1),), np.uint32)

        def potential():
            t.group_potential_device(off.ptr, mem.ptr, G, K, None, 0.0, 0, phi.ptr, minpos.ptr,
                                     stream=s.handle)

        potential()
        s.synchronize()
        sizes = np.diff(off.numpy().astype(np.int64))
        r = {"min_members": mm, "groups": G, "entries": K,
             "largest_group": int(sizes.max()) if G else 0,
             "sum_s2": float(np.sum(sizes.astype(np.float64) ** 2)),
             "catalog_call": timed(s, steps, catalog) if G else None,
             "group_potential_call": timed(s, steps, potential),
             "kernels": kernel_ms(SCOPES, s, steps, potential)}
        if G:
            g = int(np.argmax(sizes))
            a = int(off.numpy()[g])
            hp = phi.numpy()[a:a + int(sizes[g])]
            assert int(minpos.numpy()[g]) == a + int(np.argmin(hp)) and np.all(hp < 0)
        res["catalogs"].append(r)
        kk = r["kernels"]
        print(f"(b) {kind} n={n:.0e} min_members={mm}: {G} groups, {K} entries, largest "
              f"{r['largest_group']}, sum s^2 {r['sum_s2']:.3e}; fof "
              f"{res['fof_call']['median_ms']:.2f} ms, catalogue "
              f"{r['catalog_call']['median_ms'] if G else float('nan'):.2f} ms, group_potential "
              f"{r['group_potential_call']['median_ms']:.2f} ms (validate "
              f"{kk['gpot_validate']['ms_per_call']:.3f}, gather "
              f"{kk['gpot_gather']['ms_per_call']:.3f}, sum {kk['gpot_sum']['ms_per_call']:.3f}, "
              f"argmin {kk['gpot_argmin']['ms_per_call']:.3f})", flush=True)
        for o in (off, mem, phi, minpos):
            o.free()
    t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--direct-n", type=float, default=1e5)
    ap.add_argument("--n", type=float, default=1e7)
    ap.add_argument("--inputs", nargs="*", default=["uniform", "lognormal"])
    ap.add_argument("--min-members", type=int, nargs="+", default=[2, 20])
    ap.add_argument("--leaf", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_potential.json"))
    a = ap.parse_args()
    hip.preload()
    hip.set_device(0)
    out = {"direct": direct(int(a.direct_n), a.leaf, a.steps),
           "catalogues": [catalogue(k, int(a.n), a.leaf, a.steps, a.min_members)
                          for k in a.inputs]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if out["direct"]["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
