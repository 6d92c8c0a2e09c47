"""Static instruction counts per execution path of one collect kernel in a
gfx950 assembly listing (hipcc -S --cuda-device-only with the project's
flags), and the per-packet issue they predict at the bench's traversal
frequencies.  Same prefix classification as scripts/asm_counts.py.

  python scripts/asm_paths.py knn_collect.s 'knn_collect_grp_kernelILb1ELi8ELb0ELb0ELb1ELb1E' \
      [--bench BENCH_r06.json] [--pops 45] [--visit 28,1,7,16 --pop 17,2,4,14]

What is a path here:
  - every loop the compiler annotates ("Loop Header"; its blocks are those
    annotated "in Loop: Header=" with it), named by what only it contains (the pop's
    v_readlane with an SGPR lane select, the pair list's ds_write_b16, the
    candidate store global_store_dwordx2); counts are given for the whole body
    and exclusive of the loops inside it.  The kernel holds the periodic and the
    plain instance of the packet; of two loops with the same name the first is
    the periodic one;
  - inside the scan loop, the hit region (from the s_and_saveexec before the
    candidate store to the exec restore after it);
  - the hand-scheduled descent (packet.hpp walk_descend), traced through its
    own labels for each outcome of a visit;
  - everything outside the loops: prologue, per-leaf code the compiler did not
    shape as a loop (the staging, the leaf bookkeeping), epilogue.
The compiled walk loop (parent listing, periodic instance) has no labels to
trace by; its per-visit paths were counted by hand (profiles/r08a_*.txt).

A one-off analysis aid for profiles/r08a_collect_issue_breakdown.txt, not a
maintained tool: it recognises the loops by opcodes only they contain and the
descent by its .Lwd_* labels, so it follows this kernel's shape as compiled
today and breaks when the loop shapes or the labels change; the parent's visit
and pop figures come from the command line (hand counts), and pops per packet
are an assumed lower bound, not a counter."""
import argparse
import json
import re

from asm_counts import classify

KEYS = ("salu", "smem", "branch", "valu", "lane", "lds", "vmem", "wait/nop")


def is_inst(ln):
    t = ln.split()
    return bool(t) and not t[0].endswith(":") and not t[0].startswith((".", ";"))


def count(lines):
    c = dict.fromkeys(KEYS, 0)
    for ln in lines:
        if is_inst(ln):
            k = classify(ln.split()[0])
            c[k] = c.get(k, 0) + 1
    return c


def fmt(c):
    return " ".join(f"{k}={c.get(k, 0)}" for k in KEYS if c.get(k, 0))


def sub(a, b):
    return {k: a.get(k, 0) - b.get(k, 0) for k in set(a) | set(b)}


def kernel_body(text, key):
    start = next(i for i, ln in enumerate(text) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", ln))
    end = next(i for i in range(start, len(text)) if text[i].strip().startswith("s_endpgm"))
    return text[start:end + 1]


def find_loops(body):
    """The loops the compiler annotates, by block membership (a loop's blocks
    need not be contiguous, and its back edge may be a fall-through): a list of
    (header label, depth, parent header or None, lines of its own blocks,
    index of the header)."""
    starts = [i for i, ln in enumerate(body) if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln)]
    loops, order = {}, []
    for n, i in enumerate(starts):
        end = starts[n + 1] if n + 1 < len(starts) else len(body)
        j, head = i, body[i]
        while j + 1 < end and body[j + 1].strip().startswith(";") and not is_inst(body[j + 1]):
            j += 1
            head += "\n" + body[j]
        own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", head)
        if own:
            name = re.match(r"^\.L(BB\d+_\d+):", body[i]).group(1)
            parents = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", head)
            parent = max(parents, key=lambda p: int(p[1]))[0] if parents else None
            loops[name] = {"depth": int(own.group(1)), "parent": parent, "lines": [], "head": i}
            order.append(name)
        else:
            m = re.search(r"in Loop: Header=(BB\d+_\d+)", head)
            name = m.group(1) if m else None
        if name:
            lp = loops.setdefault(name, {"depth": 0, "parent": None, "lines": []})
            lp["lines"] += body[i:end]
    return [(n, loops[n]["depth"], loops[n]["parent"], loops[n]["lines"], loops[n]["head"])
            for n in order]


def loop_tree_lines(loops, name):
    """a loop's own lines and those of the loops inside it"""
    out = []
    for (n, d, p, ls, f) in loops:
        q = n
        while q is not None and q != name:
            q = next(pp for (nn, dd, pp, ll, ff) in loops if nn == q)
        if q == name:
            out += ls
    return out


def loop_name(lines):
    txt = "\n".join(lines)
    if "ds_write_b16" in txt and "global_store_dwordx2" in txt:
        return "leaf loop" if re.search(r"v_readlane_b32 s\d+, v\d+, s\d+", txt) else "chunk loop"
    if re.search(r"v_readlane_b32 s\d+, v\d+, s\d+", txt):
        return "pop+walk loop" if ".Lwd_top" not in txt else "pop loop (descent in walk_descend)"
    if "ds_write_b16" in txt:
        return "group-test loop"
    if "global_store_dwordx2" in txt:
        return "scan loop"
    return "loop"


def hit_region(lines):
    st = next((i for i, ln in enumerate(lines) if "global_store_dwordx2" in ln), None)
    if st is None:
        return None
    a = max((i for i in range(st) if "s_and_saveexec_b64" in lines[i]), default=None)
    if a is None:
        return None
    b = next((i for i in range(st, len(lines)) if re.search(r"s_(or|mov)_b64 exec,", lines[i])),
             len(lines) - 1)
    return lines[a:b + 1]


def trace_asm(block, start, decisions, stops):
    """instructions from label `start`, taking conditional branch n iff
    decisions[n], following s_branch, until a label in `stops` is reached"""
    label = {ln.strip().rstrip(":"): i for i, ln in enumerate(block) if ln.strip().endswith(":")}
    i, out, d = label[start] + 1, [], list(decisions)
    while True:
        ln = block[i].strip()
        if ln.endswith(":"):
            if ln.rstrip(":") in stops:
                return out
            i += 1
            continue
        if not is_inst(ln):
            i += 1
            continue
        out.append(ln)
        op = ln.split()[0]
        if op == "s_branch" or (op.startswith("s_cbranch") and d.pop(0)):
            tgt = ln.split()[-1]
            if tgt in stops:
                return out
            i = label[tgt] + 1
        else:
            i += 1


def asm_paths(body):
    a = next((i for i, ln in enumerate(body) if ".Lwd_top" in ln and ln.strip().endswith(":")), None)
    if a is None:
        return None
    s = max(i for i in range(a) if "#ASMSTART" in body[i])
    e = next(i for i in range(a, len(body)) if "#ASMEND" in body[i])
    block = body[s + 1:e]
    sfx = re.search(r"\.Lwd_top(_\d+):", body[a]).group(1)
    L = lambda n: ".Lwd_" + n + sfx  # noqa: E731
    top, end = L("top"), L("end")
    paths = {}
    # dispatch decisions: leaf?, y?, x? (z falls through after three tests)
    for ax, disp in (("z", [False, False, False]), ("y", [False, True]), ("x", [False, False, True])):
        paths[f"visit {ax}: left only"] = trace_asm(block, top, disp + [True, True], {top, end})
        paths[f"visit {ax}: right only"] = trace_asm(block, top, disp + [False, True], {top, end})
        paths[f"visit {ax}: both, left near"] = trace_asm(block, top, disp + [False, False, False], {top, end})
        paths[f"visit {ax}: both, right near"] = trace_asm(block, top, disp + [False, False, True], {top, end})
        paths[f"visit {ax}: none wanted"] = trace_asm(block, top, disp + [True, False], {top, end})
    paths["leaf found"] = trace_asm(block, top, [True], {top, end})
    entry = [ln.strip() for ln in block[:block.index(next(x for x in block if ".Lwd_top" in x))]]
    paths["descent entry"] = [ln for ln in entry if is_inst(ln)]
    return {k: count(v) for k, v in paths.items()}


def mean(cs):
    return {k: sum(c.get(k, 0) for c in cs) / len(cs) for k in KEYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("key")
    ap.add_argument("--bench", default=None, help="a BENCH_*.json with traversal_per_packet")
    ap.add_argument("--pops", type=float, default=None,
                    help="pops per packet (not counted by the bench; default leaves_reached + 1, "
                         "its lower bound)")
    ap.add_argument("--visit", default=None,
                    help="hand-counted SALU,SMEM,branch,VALU of one compiled visit (single child) "
                         "for a listing without the hand-scheduled descent")
    ap.add_argument("--pop", default=None,
                    help="hand-counted SALU,SMEM,branch,VALU of one accepted pop, likewise")
    a = ap.parse_args()
    body = kernel_body(open(a.listing).read().splitlines(), a.key)
    print("kernel", body[0].split(":")[0])
    whole = count(body)
    print("  whole kernel:", fmt(whole))
    loops = find_loops(body)
    named = []
    inloop = dict.fromkeys(KEYS, 0)
    # the plain instance follows the periodic one: from the loop with the second pop on
    pop_re = re.compile(r"v_readlane_b32 s\d+, v\d+, s\d+")
    pops_at = [f for (n, d, p, ls, f) in loops
               if p is None and any(pop_re.search(x) for x in loop_tree_lines(loops, n))]
    plain_from = sorted(pops_at)[1] if len(pops_at) > 1 else len(body)
    for (name, d, parent, own, first) in loops:
        lines = loop_tree_lines(loops, name)
        nm = loop_name(lines)
        inst = "plain" if first >= plain_from else "periodic"
        if nm.startswith("pop loop"):
            # the descent's block sits inside the pop loop's blocks: counted by path below
            own = [x for x in own if not re.match(r"^[sv]_|^\.Lwd_", x)]
            lines = own
        named.append((nm, inst, count(lines), count(own), lines))
        print(f"  {inst:8s} {nm} (header {name}, depth {d}): body {fmt(count(lines))}")
        if len(own) != len(lines):
            print(f"  {'':8s}   exclusive of its inner loops: {fmt(count(own))}")
        if nm == "scan loop":
            hr = hit_region(lines)
            if hr:
                print(f"  {'':8s}   hit region: {fmt(count(hr))}; a step without a hit: "
                      f"{fmt(sub(count(lines), count(hr)))}")
        inloop = {k: inloop[k] + count(own)[k] for k in KEYS}
    outside = sub(whole, inloop)
    print("  outside every loop (both instances: prologue, instance choice, staging and leaf "
          "bookkeeping, epilogue):", fmt(outside))
    ap_ = asm_paths(body)
    if ap_:
        print("  hand-scheduled descent (plain instance), per outcome of one visit:")
        for k, v in ap_.items():
            print(f"    {k:28s} {fmt(v)}")
    if not a.bench:
        return
    raw = open(a.bench).read()
    m = re.search(r'\\?"traversal_per_packet\\?": (\{[^}]*\})', raw)
    tp = json.loads(m.group(1).replace('\\"', '"'))
    lanes = float(re.search(r'\\?"lanes_per_scanned_chunk\\?": ([0-9.]+)', raw).group(1))
    leaves, visits, steps = tp["leaves_reached"], tp["node_visits"], tp["sparse_iters"]
    chunks = tp["leaves_scanned"]
    pops = a.pops if a.pops is not None else leaves + 1
    giter = chunks * (lanes * 8 / 64 + 0.5)
    internal = visits - leaves
    pushes = pops - 1
    print(f"\nper packet ({a.bench}): node_visits {visits:.1f} = {internal:.1f} internal + {leaves:.1f} leaves, "
          f"scan steps {steps:.1f}, scanned chunks {chunks:.1f} ({lanes:.1f} lanes each: about {giter:.0f} "
          f"group-test iterations), pops {pops:.1f} (assumed), pushes {pushes:.1f}")
    plain = {nm: (c, x) for (nm, inst, c, x, ls) in named if inst == "plain"}
    rows = []
    if ap_:
        single = mean([v for k, v in ap_.items() if "only" in k])
        both = mean([v for k, v in ap_.items() if "both" in k])
        none = mean([v for k, v in ap_.items() if "none" in k])
        dead = max(pops - leaves - 1, 0.0)
        rows.append(("visits, single child", internal - pushes - dead, single))
        rows.append(("visits, both children", pushes, both))
        rows.append(("visits, none wanted", dead, none))
        rows.append(("leaf found", leaves, ap_["leaf found"]))
        rows.append(("descent entry", leaves + dead, ap_["descent entry"]))
        rows.append(("pop", pops, plain["pop loop (descent in walk_descend)"][0]))
    elif a.visit:
        v = dict(zip(("salu", "smem", "branch", "valu"), map(float, a.visit.split(","))))
        rows.append(("visits (hand count, single child)", visits, v))
        if a.pop:
            v = dict(zip(("salu", "smem", "branch", "valu"), map(float, a.pop.split(","))))
            rows.append(("pops (hand count, accepted)", pops, v))
    for nm, label, f in (("group-test loop", "group-test iteration", giter), ("scan loop", "scan step", steps)):
        if nm in plain:
            rows.append((label, f, plain[nm][0]))
    if "chunk loop" in plain:
        rows.append(("chunk, outside its inner loops", chunks, plain["chunk loop"][1]))
    # the per-leaf code around the walk and the chunk loop (staging, leaf bookkeeping).  Where
    # the compiler does not shape the plain instance's leaf loop as a loop (the descent's
    # block in it), its lines are among "outside every loop": the periodic instance's
    # per-leaf count (the same source) stands in and is taken off that remainder
    per = {nm: x for (nm, inst, c, x, ls) in named if inst == "periodic"}
    if "leaf loop" in plain:
        rows.append(("leaf, outside its inner loops", leaves, plain["leaf loop"][1]))
    elif "leaf loop" in per:
        rows.append(("leaf, outside its inner loops (periodic stand-in)", leaves, per["leaf loop"]))
        outside = sub(outside, per["leaf loop"])
    rows.append(("outside every loop, once (upper bound: both instances)", 1.0, outside))
    tot = dict.fromkeys(KEYS, 0.0)
    print(f"  {'path':52s} {'per packet':>10s}   SALU    SMEM  branch    VALU")
    for label, f, c in rows:
        print(f"  {label:52s} {f:10.1f} " + " ".join(f"{f * c.get(k, 0):7.0f}" for k in ("salu", "smem", "branch", "valu")))
        for k in KEYS:
            tot[k] += f * c.get(k, 0)
    print(f"  {'predicted total':52s} {'':10s} " + " ".join(f"{tot[k]:7.0f}" for k in ("salu", "smem", "branch", "valu")))


if __name__ == "__main__":
    main()
