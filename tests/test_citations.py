"""Every `file:line` citation of a reference source in this repo resolves:
the cited lines exist in that file of the reference (VERDICT r03 found
kdtree_impl.hpp citations past the end of the 275-line file).  The reference's
file names and line counts are recorded in tests/golden/reference_lines.json,
so the check runs everywhere; where the reference itself is present the
record is compared with it first."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
LINES = os.path.join(ROOT, "tests", "golden", "reference_lines.json")
CITED_EXT = (".cpp", ".hpp", ".h", ".py", ".asm", ".pyi", ".txt", ".vert", ".frag")
SCAN = ["oracle", "nbodyhpc_amd", "include", "tests", "nbodyhpc", "DESIGN.md", "INTEGRATION.md",
        "bench.py", "README.md", "BASELINE.md", "__graft_entry__.py"]
EXT = (".py", ".c", ".cpp", ".h", ".hpp", ".hip", ".md", ".pyi")
CITE = re.compile(r"([A-Za-z0-9_./-]+\.(?:cpp|hpp|h|py|asm|pyi|txt|vert|frag)):(\d+)(?:-(\d+))?")
# bare continuations of a citation: "file.hpp:52-61, :111-120" or "file.cpp:90 and :128"
MORE = re.compile(r"\s*(?:,|;|and|&)?\s*:(\d+)(?:-(\d+))?")
# a bare ":NNN" on a line of its own (no file before it on that line) names no file:
# such lines are flagged, since the reader cannot tell which file they cite
BARE = re.compile(r"\(\s*:(\d+)(?:-(\d+))?(?:\s*,\s*:(\d+)(?:-(\d+))?)*\s*\)")


def walk_reference(ref=REF):
    """{path relative to the reference: its line count} of every file a
    citation can name (tests/golden/gen_golden.py --only cites records it)."""
    out = {}
    for d, _, fs in os.walk(ref):
        if "/.git" in d:
            continue
        for f in fs:
            if f.endswith(CITED_EXT):
                p = os.path.join(d, f)
                with open(p, "rb") as fh:
                    out[os.path.relpath(p, ref)] = fh.read().count(b"\n") + 1
    return out


def _ref_files():
    """The recorded index (names and line counts only), so the check runs where
    the reference is absent; where it is present the index must equal it."""
    with open(LINES) as f:
        by_path = json.load(f)
    if os.path.isdir(os.path.join(REF, "kdtree")):
        assert by_path == walk_reference(), "tests/golden/reference_lines.json is stale"
    by_name = {}
    for rel in by_path:
        by_name.setdefault(os.path.basename(rel), []).append(rel)
    return by_name, by_path


def test_reference_citations_resolve():
    by_name, lines = _ref_files()
    by_path = {rel: rel for rel in lines}
    _lines = lines.__getitem__
    bad, checked = [], 0
    for top in SCAN:
        p0 = os.path.join(ROOT, top)
        files = [p0] if os.path.isfile(p0) else [
            os.path.join(d, f) for d, _, fs in os.walk(p0) for f in fs if f.endswith(EXT)]
        for fp in files:
            if "/golden/" in fp or "__pycache__" in fp:
                continue
            txt = open(fp, encoding="utf-8", errors="replace").read()
            for m in CITE.finditer(txt):
                name = m.group(1)
                cands = [by_path[name]] if name in by_path else [
                    p for p in by_name.get(os.path.basename(name), [])
                    if os.path.join(REF, p).endswith(name)]
                if not cands:
                    continue  # not a reference file
                ranges = [(int(m.group(2)), int(m.group(3) or m.group(2)))]
                pos = m.end()
                while True:  # ", :111-120" continuations cite the same file
                    c = MORE.match(txt, pos)
                    if not c:
                        break
                    ranges.append((int(c.group(1)), int(c.group(2) or c.group(1))))
                    pos = c.end()
                # an ambiguous bare name (pybind.cpp in kdtree/ and rasterization/)
                # must fit at least one of the files it may name
                ns = [_lines(c) for c in cands]
                for a, b in ranges:
                    checked += 1
                    if not any(1 <= a <= b <= n for n in ns):
                        bad.append(f"{os.path.relpath(fp, ROOT)}: {name}:{a}-{b} (files have {ns} lines)")
            for m in BARE.finditer(txt):
                # a parenthesised bare line number with no file: resolvable only by the reader's guess
                line = txt[:m.start()].rsplit("\n", 1)[-1]
                if not CITE.search(line):
                    bad.append(f"{os.path.relpath(fp, ROOT)}: bare citation {m.group(0)}")
    assert checked > 100
    assert not bad, "\n".join(bad[:40])
