"""Static instruction counts of one kernel in a gfx950 assembly listing
(hipcc -S --cuda-device-only with the project's flags): the whole kernel, and
every loop that pops the wave stack (the packet walk: a v_readlane_b32 with an
SGPR lane select, which only the pop has), each from its loop header label to
its last backward branch.
python scripts/asm_counts.py knn_collect.s 'knn_collect_grp_kernelILb1ELi8ELb0ELb0ELb1E' [--max-sgprs N]
--max-sgprs N: exit 1 if the kernel's TotalNumSgprs is above N.  The collect kernel's
hand-scheduled descent (packet.hpp walk_descend) owns four fixed SGPRs; 80 is what the
compiler itself keeps a kernel of 8 waves per SIMD under, and a kernel above it loses a wave."""
import re
import sys


def classify(op):
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep", "s_setprio")):
        return "wait/nop"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "other"


def counts(lines):
    c = {}
    for ln in lines:
        t = ln.split()
        if not t or t[0].endswith(":") or t[0].startswith((".", ";")):
            continue
        k = classify(t[0])
        c[k] = c.get(k, 0) + 1
        if t[0].startswith("s_mov_b64"):
            c["s_mov_b64"] = c.get("s_mov_b64", 0) + 1
        if t[0].startswith("s_cselect"):
            c["s_cselect"] = c.get("s_cselect", 0) + 1
        if t[0].startswith("v_mov_b32"):
            c["v_mov_b32"] = c.get("v_mov_b32", 0) + 1
    return c


def main():
    path, key = sys.argv[1], sys.argv[2]
    max_sgprs = int(sys.argv[sys.argv.index("--max-sgprs") + 1]) if "--max-sgprs" in sys.argv else None
    text = open(path).read().splitlines()
    start = next(i for i, ln in enumerate(text) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", ln))
    end = next(i for i in range(start, len(text)) if text[i].strip().startswith("s_endpgm"))
    body = text[start:end + 1]
    meta = [ln.strip() for ln in text[end:end + 120]
            if re.search(r"\.(sgpr_count|vgpr_count|sgpr_spill_count|vgpr_spill_count|"
                         r"group_segment_fixed_size|private_segment_fixed_size)|; (NumSgprs|NumVgprs|"
                         r"ScratchSize|Occupancy|LDSByteSize|SGPRBlocks)", ln)]
    print("kernel", text[start].rstrip(":"))
    for m in meta:
        print("  ", m)
    if max_sgprs is not None:
        # the first TotalNumSgprs after the kernel's end is its own
        n = next(int(re.search(r"; TotalNumSgprs: (\d+)", ln).group(1)) for ln in text[end:]
                 if "; TotalNumSgprs:" in ln)
        print("   ; TotalNumSgprs:", n)
        if n > max_sgprs:
            sys.exit(f"{n} SGPRs, more than {max_sgprs}")
    print("  whole kernel:", dict(sorted(counts(body).items())))
    label = {ln.split(":")[0]: i for i, ln in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", ln)}
    pops = [i for i, ln in enumerate(body) if re.match(r"\s*v_readlane_b32 s\d+, v\d+, s\d+", ln)]
    for p in pops:
        # the innermost loop around the pop: the closest header label above it
        # that some later branch jumps back to
        best = None
        for name, li in label.items():
            if li > p:
                continue
            back = [i for i in range(p, len(body)) if re.search(r"s_c?branch\S* " + re.escape(name) + r"$",
                                                                body[i].strip())]
            if back and (best is None or li > best[0]):
                best = (li, max(back))
        if best:
            print(f"  walk loop lines {best[0]}..{best[1]} ({best[1] - best[0] + 1} lines):",
                  dict(sorted(counts(body[best[0]:best[1] + 1]).items())))


if __name__ == "__main__":
    main()
