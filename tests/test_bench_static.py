"""bench.py's N > 1 lines: every collective (gloo all-reduce / all-gather /
barrier) must run on every rank, so none may follow the point where the other
ranks return and rank 0 alone writes the JSON line.  (Round 3 found C5's
second-round summary all-reduces after that point: N = 2 ended with
"connection closed by peer".)"""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLECTIVES = {"allsum", "allmax", "allgather_int", "barrier", "all_reduce", "all_gather",
               "broadcast", "second_round", "slab_roofline"}


def _is_rank0_return(node):
    """`if rank != 0: return`"""
    if not isinstance(node, ast.If) or not node.body or not isinstance(node.body[0], ast.Return):
        return False
    t = node.test
    return (isinstance(t, ast.Compare) and isinstance(t.left, ast.Name) and t.left.id == "rank"
            and isinstance(t.ops[0], ast.NotEq))


def _called_names(node):
    for n in ast.walk(node):
        if isinstance(n, ast.Call):
            f = n.func
            if isinstance(f, ast.Name):
                yield f.id
            elif isinstance(f, ast.Attribute):
                yield f.attr


def test_no_collective_after_rank0_return():
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    checked = 0
    for fn in ast.walk(tree):
        if not isinstance(fn, ast.FunctionDef):
            continue
        for i, stmt in enumerate(fn.body):
            if _is_rank0_return(stmt):
                checked += 1
                late = {name for s in fn.body[i + 1:] for name in _called_names(s)} & COLLECTIVES
                assert not late, f"{fn.name}: {sorted(late)} after `if rank != 0: return`"
    assert checked >= 2  # main's headline line and run_c5's line


def _run_bench(args, env_extra=None, timeout=120):
    import json
    import subprocess
    import sys
    env = {kk: v for kk, v in os.environ.items()
           if kk not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NBKD_BENCH_SAME_DEVICE")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, [json.loads(ln) for ln in lines], p.stderr


def test_gpus_n_without_launcher_starts_n_ranks():
    """`python bench.py --gpus 2` with no WORLD_SIZE starts two ranks itself
    (torch.distributed.run children; the parent never execs) and forwards rank
    0's one JSON line: the --launch-probe ranks meet over gloo without a GPU."""
    rc, lines, err = _run_bench(["--gpus", "2", "--launch-probe"])
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines
    assert lines[0]["n_gpus"] == 2 and lines[0]["ranks"] == [0, 1]


def test_n_gt_1_line_reports_rccl_errors_and_per_rank_numbers():
    """an N > 1 line is readable on its own.  A forced RCCL
    failure on rank 1 reaches the line as halo.rccl_error (every rank falls
    back to gloo, so the line is marked degraded), and each rank's numbers come
    back as lists over the ranks; without a failure there is no error and the
    line is not degraded."""
    rc, lines, err = _run_bench(["--gpus", "2", "--launch-probe", "--probe-rccl-fail", "1"])
    assert rc == 0, err[-2000:]
    h = lines[0]["halo"]
    assert h["degraded"] is True
    assert len(h["rccl_error"]) == 1 and h["rccl_error"][0].startswith("rank 1: RCCL unavailable")
    assert "forced RCCL failure" in h["rccl_error"][0]
    assert h["per_rank"]["step_ms"] == [1.0, 2.0]
    assert h["per_rank"]["halo_transport"] == ["gloo-staged", "gloo-staged"]
    rc, lines, err = _run_bench(["--gpus", "2", "--launch-probe"])
    assert rc == 0, err[-2000:]
    h = lines[0]["halo"]
    assert h["degraded"] is False and h["rccl_error"] is None
    assert h["per_rank"]["collect_ms"] == [0.5, 1.5]


def test_gpus_n_with_fewer_gpus_fails_cleanly():
    """Fewer visible GPUs than --gpus (none here): a non-zero exit and no JSON
    line, never an n_gpus: 1 line for an N = 2 request."""
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("two GPUs are visible")
    rc, lines, err = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert rc != 0 and not lines
    assert "GPU(s) visible" in err


def test_pmc_lookups_match_the_library_sha(tmp_path, monkeypatch):
    """roofline.traffic / step_traffic come only from a PMC summary whose
    lib_sha256 is the loaded library's (no GPU: the lookups read files)."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "lib_sha256", lambda: "abc")
    json.dump({"lib_sha256": "abc", "n_particles": 100, "k": 32, "hbm_bytes_per_step": 7.0},
              open(prof / "r99_pmc_step.json", "w"))
    json.dump({"lib_sha256": "zzz", "n_particles": 100, "k": 32, "hbm_bytes_per_step": 9.0},
              open(prof / "r98_pmc_step.json", "w"))
    assert bench.pmc_step_traffic(100, 32) == (7.0, "profiles/r99_pmc_step.json")
    assert bench.pmc_step_traffic(100, 16) == (None, None)
    monkeypatch.setattr(bench, "lib_sha256", lambda: "other")
    assert bench.pmc_step_traffic(100, 32) == (None, None)
    r = bench.roofline_entry(8e9, "x", 2.0, 1000.0, step_traffic=1.0)
    assert abs(r["frac"] - 8e9 / 2e-3 / 1e9 / 8000.0) < 1e-12 and r["frac"] <= 1.0


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_and_under_64_mb():
    """--dump-outputs at the headline shape (1e8 rows, k = 32: f32 distances,
    ids as f64, the row numbers as f64): the sampled row blocks depend on the
    seed alone, lie inside the output, do not overlap and stay under 64 MB on
    disk; an output that fits is written whole."""
    bench = _bench_module()
    n, per_row = 100_000_000, 8 + 32 * 4 + 32 * 8
    starts, blk = bench.sample_blocks(n, 20261015, per_row)
    again, _ = bench.sample_blocks(n, 20261015, per_row)
    other, _ = bench.sample_blocks(n, 7, per_row)
    assert (starts == again).all() and not (starts == other).all()
    assert blk == bench.DUMP_BLOCK_ROWS and (starts % blk == 0).all()
    assert len(set(starts.tolist())) == len(starts) and starts.min() >= 0 and starts.max() + blk <= n
    assert 32_000_000 < len(starts) * blk * per_row <= 64_000_000
    starts, blk = bench.sample_blocks(1000, 20261015, per_row)
    assert starts.tolist() == [0] and blk == 1000


def test_n_gt_1_roofline_from_per_rank_slab_profiles(tmp_path, monkeypatch):
    """an N > 1 line finds the slab profile of its own build
    and decomposition (library SHA, world, scaling, --particles, k, leafsize,
    seed), and the roofline sums every rank's own queries x bytes per query over
    the slowest rank's time against N x 8 TB/s."""
    import json
    import types
    bench = _bench_module()
    monkeypatch.setattr(bench, "lib_sha256", lambda: "abc")
    monkeypatch.setattr(bench, "PROFILES", str(tmp_path))
    entry = {"world": 2, "rank": 0, "scaling": "strong", "n_arg": 100_000_000, "k": 32,
             "leafsize": 64, "seed": 20261015, "own": 50_000_000, "n_local": 54_000_000,
             "collect_bytes_per_query": 1000.0, "step_bytes_per_query": 2000.0}
    other = dict(entry, world=4)
    json.dump({"lib_sha256": "abc", "entries": [other, entry]},
              open(tmp_path / "r99_pmc_slab.json", "w"))
    json.dump({"lib_sha256": "old", "entries": [dict(entry, step_bytes_per_query=1.0)]},
              open(tmp_path / "r98_pmc_slab.json", "w"))
    args = types.SimpleNamespace(scaling="strong", n=1e8, leafsize=64, seed=20261015)
    e, src = bench.pmc_slab(args, 2, 32)
    assert e == entry and src.endswith("r99_pmc_slab.json")
    assert bench.pmc_slab(args, 8, 32) == (None, None)
    assert bench.pmc_slab(types.SimpleNamespace(**dict(vars(args), scaling="weak")), 2, 32) \
        == (None, None)
    # two ranks (the reducers stand in for gloo): rank times 10 and 12 ms
    world = 2
    allsum = lambda v: v * world  # noqa: E731  (both ranks hold the same values)
    allmax = lambda v: max(v, 12.0) if v > 1 else v  # noqa: E731
    r = bench.slab_roofline(e, src, world, 4951.6, 5e7, 5e7, 10.0, 0.025, allsum, allmax)
    assert r["kernel_ms"] == 12.0 and r["peak"] == 16000.0
    assert r["traffic"] == 2 * 1000.0 * 5e7 and r["step_traffic"] == 2 * 2000.0 * 5e7
    assert abs(r["step_achieved"] - 2 * 2000.0 * 5e7 / 0.025 / 1e9) < 1e-6
    assert "rank 0's slab" in r["basis"]
    # a rank without a profile: no traffic terms on any rank
    r0 = bench.slab_roofline(None, None, world, 4951.6, 5e7, 5e7, 10.0, 0.025,
                             lambda v: v, allmax)
    assert r0["traffic"] is None and r0["step_traffic"] is None and r0["basis"] is None
