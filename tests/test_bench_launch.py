"""bench.py's N > 1 path on a CPU-only machine: the driver's launcher line (torch.distributed.run, one process per "GPU", RANK / WORLD_SIZE
from the environment), the default workload at N > 1 (cfg5), the query sharding, the REAL host planner on every rank's shard, the
per-step result gather (ResultGather.rebind + all_gather_into_tensor) and the one JSON line of rank 0 — everything up to the kernels,
which --dry-run leaves out (zeros in the result blocks, gloo instead of RCCL)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_bench(nproc, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "2", "--warmup", "1", "--dry-run", "--full", "--docs", "100000", "--vocab", "10000"] + extra  # fmt: skip
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]  # ONE line, from rank 0
    return json.loads(lines[0])


POINT_KEYS = {"workload", "scaling", "total_queries", "n_gpus", "value", "unit", "per_gpu_value", "ms_per_step", "gather_ms", "hbm_bytes_in_use", "n1", "speedup_vs_n1", "what"}


def check_scaling_point(out, n, total):
    """Every line carries the scaling curve's point it stands for, self-contained: the mixed batch, strong scaling, the same workload's one-GPU rate (n1) beside it."""
    sp = out["scaling_point"]
    assert POINT_KEYS <= set(sp), sorted(POINT_KEYS - set(sp))
    assert sp["scaling"] == "strong" and sp["n_gpus"] == n and sp["total_queries"] == total and sp["workload"].startswith("cfg5")
    assert sp["per_gpu_value"] * n == pytest.approx(sp["value"]) and set(sp["hbm_bytes_in_use"]) == {"engine_pool_in_use", "engine_pool_idle", "device_in_use", "device_total"}
    n1 = sp["n1"]
    assert n1["n_gpus"] == 1 and n1["total_queries"] == total and n1["workload"] == sp["workload"] and n1["value"] > 0
    assert sp["speedup_vs_n1"] == pytest.approx(sp["value"] / n1["value"])
    assert (sp["gather_ms"] is None) == (n == 1)
    assert "hbm_bytes_in_use" in out


def test_two_ranks_default_workload_is_the_mixed_batch_split_over_the_ranks():
    out = run_bench(2, ["--queries", "1000"])
    assert out["n_gpus"] == 2 and out["dry_run"] and out["scaling"] == "strong"  # (north_star: ONE batch sharded over the GPUs)
    assert out["config"]["workload"].startswith("cfg5") and out["config"]["queries_per_gpu_per_step"] == 500 and out["config"]["queries_per_step"] == 1000
    assert [b["queries"] for b in out["config"]["batches_per_step"]] == [350, 150]
    assert out["gather_check"] == {"ranks": 2, "blocks": ["counts", "docs", "scores", "topk_counts"], "equal_on_every_rank": True}
    assert out["per_gpu_value"] * 2 == out["value"] and out["gather_ms"] >= 0
    check_scaling_point(out, 2, 1000)
    for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "roofline", "kernels_only", "end_to_end"):
        assert k in out


def test_eight_ranks_carry_the_same_block():
    out = run_bench(8, ["--queries", "1600"])
    assert out["n_gpus"] == 8 and out["scaling"] == "strong" and out["config"]["queries_per_gpu_per_step"] == 200
    check_scaling_point(out, 8, 1600)


def test_one_gpu_line_carries_the_mixed_batch_point_beside_the_cfg2_headline():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--dry-run", "--full", "--docs", "100000", "--vocab", "10000", "--queries", "512", "--scaling-total", "800",
           "--scaling-ref-steps", "2"]  # fmt: skip
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 1 and out["scaling"] == "weak" and out["config"]["workload"].startswith("cfg2")  # the headline stays BASELINE.json's configs[1]
    check_scaling_point(out, 1, 800)
    assert out["scaling_point"]["speedup_vs_n1"] == 1.0


FULL_ONLY = ("roofline", "scaling_point", "rotating", "delivered", "cpu_baseline", "parity_check", "gather_check", "pipelined_results_equal_resident_batch", "docids_materialised_per_step")


def test_plain_run_times_the_headline_alone_and_dumps_what_its_last_step_delivered(tmp_path):
    """Without --full the line carries the headline and what the timed steps measured, none of the legs beside it; --steps is the number of
    timed steps; --dump-outputs writes the last step's result blocks as float .npy files, the same on every run with the same arguments."""
    import numpy as np

    def run(d):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dry-run", "--docs", "100000", "--vocab", "10000", "--queries", "512",
               "--workload", "cfg5", "--dump-outputs", str(d)]  # fmt: skip
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="1"))
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, res.stdout[-2000:]
        return json.loads(lines[0])

    out = run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["metric"] == "queries/sec" and out["unit"] == "queries/s" and out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert out["steps"] == 3 and out["end_to_end"]["creates_in_timed_region"] <= 3 + 2
    assert not [k for k in FULL_ONLY if k in out], [k for k in FULL_ONLY if k in out]
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["part0_counts.npy", "part1_counts.npy", "part1_topk_counts.npy", "part1_topk_docs.npy", "part1_topk_scores.npy"]
    parts = out["config"]["batches_per_step"]
    for f in files:
        a = np.load(tmp_path / "a" / f)
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == parts[int(f[4])]["queries"]
    assert np.load(tmp_path / "a" / "part1_topk_docs.npy").shape == (parts[1]["queries"], 100)
    run(tmp_path / "b")
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_outputs_keeps_to_its_budget():
    """bench.dump_outputs: every per-query array of every part, the docset hashes split into exact 32-bit halves, a seeded docID sample; past the
    budget the per-query arrays are cut to one seeded sample of rows per part, the same rows in every array, and the files stay within it."""
    import importlib.util
    import tempfile
    from types import SimpleNamespace

    import numpy as np

    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(3)
    nq, k = 5000, 100

    class Docs:
        flags, topk = 1, 0

        def __init__(self):
            self.nq = nq
            self.c = rng.integers(0, 40000, nq).astype(np.uint64)
            self.h = rng.integers(0, 1 << 63, nq, dtype=np.uint64) * np.uint64(2) + np.uint64(1)

        def counts(self):
            return self.c

        def docset_hashes(self):
            return self.h

        def docset(self, q, n):
            assert n == int(self.c[q])
            return np.arange(n, dtype=np.uint32) * 7 + q

    class Scored:
        flags, topk = 2, k

        def __init__(self):
            self.nq = nq
            self.d = rng.integers(0, 1 << 32, (nq, k), dtype=np.uint64).astype(np.uint32)
            self.s = rng.random((nq, k), dtype=np.float32)

        def counts(self):
            return np.full(nq, 1000, np.uint64)

        def topk_results(self):
            return self.d, self.s, np.full(nq, k, np.uint32)

    T = SimpleNamespace(FLAG_ACCUMULATED_SCORE=2)
    parts = [SimpleNamespace(flags=1, topk=0), SimpleNamespace(flags=2, topk=k)]
    bs = [Docs(), Scored()]
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, T, parts, bs, False)  # (5000 x 100 top-K rows: 6 MB, within 64 MB)
        got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
        assert "part1_rows" not in got and np.array_equal(got["part1_topk_docs"], bs[1].d.astype(np.float64))
        h = got["part0_docset_hash_lo"].astype(np.uint64) | (got["part0_docset_hash_hi"].astype(np.uint64) << np.uint64(32))
        assert np.array_equal(h, bs[0].h)
        qs = got["part0_sample_queries"].astype(np.int64)
        assert len(qs) == bench.DUMP_SAMPLE_QUERIES and got["part0_sample_docids"].shape == (len(qs), bench.DUMP_SAMPLE_DOCS)
        for i, q in enumerate(qs):
            n = min(int(bs[0].c[q]), bench.DUMP_SAMPLE_DOCS)
            row = got["part0_sample_docids"][i]
            assert np.array_equal(row[:n], np.arange(n) * 7 + q) and (row[n:] == -1).all()
    bench.DUMP_BUDGET_BYTES = 12 << 20  # the sample alone is 8 MB: the top-K blocks must be cut
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, T, parts, bs, False)
        got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_BUDGET_BYTES
        for p in (0, 1):
            rows = got[f"part{p}_rows"].astype(np.int64)
            assert 0 < len(rows) < nq and np.all(np.diff(rows) > 0) and np.array_equal(got[f"part{p}_counts"], bs[p].counts()[rows].astype(np.float64))
        rows = got["part1_rows"].astype(np.int64)
        assert np.array_equal(got["part1_topk_docs"], bs[1].d[rows].astype(np.float64)) and np.array_equal(got["part1_topk_scores"], bs[1].s[rows])


def test_weak_and_strong_scaling_on_request():
    out = run_bench(2, ["--queries", "1000", "--scaling", "strong", "--workload", "cfg2", "--scaling-ref-steps", "0"])
    assert out["scaling"] == "strong" and out["config"]["queries_per_gpu_per_step"] == 500 and out["config"]["queries_per_step"] == 1000 and out["scaling_point"]["n1"] is None
    out = run_bench(2, ["--queries", "600", "--scaling", "weak", "--scaling-ref-steps", "0"])
    assert out["scaling"] == "weak" and out["config"]["queries_per_gpu_per_step"] == 600 and out["config"]["queries_per_step"] == 1200


REPLAY = """#!%s
# ref_driver's `timed` command answered from tests/golden/ref_cpu_leg.json: the corpus, the command and the query texts must be the stored ones
import json, sys
g = json.load(open(%r))
c = g["corpus"]
assert sys.argv[1:] == [str(c["D"]), str(c["V"]), str(c["slots"]), str(c["seed"])], sys.argv
head, *texts = sys.stdin.read().splitlines()
cmd, flags, budget, n = head.split()[:4]
assert cmd == "timed" and int(n) == len(texts) and texts == g["driver_texts"][: len(texts)], (head, texts)
lines = next(r["lines"] for r in g["runs"] if r["flags"] == int(flags))
for ln in lines:
    if "counts" in ln:
        ln = dict(ln, queries=len(texts), counts=ln["counts"][: len(texts)])
    print(json.dumps(ln))
"""


def test_reference_cpu_leg_runs_the_genuine_reference_on_the_sample(tmp_path):
    """bench.py's cpu_baseline of kind "reference": the sampled programs as query text through oracle/_ref/ref_driver's `timed` command (exec_query of the
    reference compiled from its own sources) — the match counts it reports equal the oracle's for conjunctions, unions, phrases, exclusions and
    optional parts, unscored and scored; a program without a text (matchsome) is refused, a missing driver is an error entry, not an exception.
    The reference's answers are stored in tests/golden/ref_cpu_leg.json (tests/golden/make_golden.py --cpu-leg-only) and replayed by a stand-in
    driver; where the prebuilt reference driver is present, the leg runs it live as well."""
    import importlib.util
    import stat
    from types import SimpleNamespace

    import numpy as np
    import oracle_lib as O
    import trinity_amd as T

    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.program_text(O.parse_query("t1 t2")) == "t1 t2" and bench.program_text(O.parse_query("[t0, t1, t2]", some_min=2)) is None
    golden = os.path.join(ROOT, "tests", "golden", "ref_cpu_leg.json")
    with open(golden) as f:
        g = json.load(f)
    replay = tmp_path / "ref_driver_replay"
    replay.write_text(REPLAY % (sys.executable, golden))
    replay.chmod(replay.stat().st_mode | stat.S_IXUSR)
    drivers = [str(replay)] + ([O.REF_DRIVER] if os.path.exists(O.REF_DRIVER) else [])
    D, V = 20000, 2000
    assert g["corpus"] == {"D": D, "V": V, "slots": 10, "seed": 42}
    seg = T.Segment(D, V, 10, 42)
    ora = O.Index.wrap(seg.index, seg.terms, seg.docs_cnt, seg.sum_terms_docs, seg.sum_term_hits)
    texts = ["t0 t1", "t3 OR t5 OR t9", "t0 t1 (t2 OR t3 OR t4)", "t3 t5 NOT t1", '"t0 t1" t2', '"t4 t5 t6"', "t0 <t7>", "t1 NOT (t2 OR t3)", "t11 t400", "t1999 t3"]
    assert g["texts"] == texts
    progs = [O.parse_query(t) for t in texts]
    for flags, oflag in ((1, O.FLAG_DOCUMENTS_ONLY), (2, O.FLAG_ACCUM_SCORE)):
        want = [len(ora.exec(p, oflag)[0]) for p in progs]
        stored = next(ln for r in g["runs"] if r["flags"] == flags for ln in r["lines"] if ln["cmd"] == "timed")
        assert stored["counts"] == want  # the genuine reference's answers are the oracle's
        for exe in drivers:
            r = bench.cpu_reference(seg, SimpleNamespace(flags=flags), progs, np.array(want), 5.0, exe=exe)
            assert "error" not in r, (exe, r)
            assert r["kind"] == "reference" and r["match_counts_equal_gpu"] and r["value"] > 0 and f"first {len(progs)} queries" in r["sample"]
        r = bench.cpu_reference(seg, SimpleNamespace(flags=flags), progs, np.array(want) + 1, 5.0, exe=str(replay))
        assert "error" not in r and not r["match_counts_equal_gpu"]
    assert "error" in bench.cpu_reference(seg, SimpleNamespace(flags=1), [O.parse_query("[t0, t1, t2]", some_min=2)], np.array([0]), 1.0)
    assert "error" in bench.cpu_reference(seg, SimpleNamespace(flags=1), progs, np.array(want), 1.0, exe=str(tmp_path / "no_such_driver"))


def test_ranks_of_a_node_pin_their_planner_threads_to_disjoint_cpus():
    """Eight ranks started side by side (LOCAL_RANK / LOCAL_WORLD_SIZE as torch.distributed.run exports them): each one's planner pool pins its
    workers inside its own slice of the affinity mask — disjoint from every other rank's, whatever CPU the creating thread runs on (round 4's
    pool took the CPUs next to the creator's: ranks landing within 16 CPUs of each other stacked their spinning workers)."""
    ncpu = len(os.sched_getaffinity(0))
    world = 8 if ncpu >= 16 else max(1, min(4, ncpu // 2))  # (slices of two CPUs or more: a one-CPU slice gets no worker at all — below)
    seen = {}
    for r in range(world):
        env = dict(os.environ, LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(world))
        res = subprocess.run([sys.executable, "-c", "import json, sys; sys.path.insert(0, %r); from trinity_amd import hostplan as HP; print(json.dumps(HP.pool_cpus(16)))" % ROOT],
                             capture_output=True, text=True, timeout=120, env=env)  # fmt: skip
        assert res.returncode == 0, res.stderr[-2000:]
        seen[r] = json.loads(res.stdout.strip().splitlines()[-1])
    allowed = sorted(os.sched_getaffinity(0))
    for r, cpus in seen.items():
        lo, hi = len(allowed) * r // world, len(allowed) * (r + 1) // world
        assert cpus and set(cpus) <= set(allowed[lo:hi]) and len(set(cpus)) == len(cpus) == min(15, hi - lo), (r, cpus)
    flat = [c for cpus in seen.values() for c in cpus]
    assert len(flat) == len(set(flat))  # no CPU carries two ranks' pollers
    # a slice of ONE CPU: no worker (it would poll on the CPU the unpinned caller runs on) — the caller plans alone
    env = dict(os.environ, LOCAL_RANK="0", LOCAL_WORLD_SIZE=str(ncpu))
    res = subprocess.run([sys.executable, "-c", "import json, sys; sys.path.insert(0, %r); from trinity_amd import hostplan as HP; print(json.dumps(HP.pool_cpus(16)))" % ROOT],
                         capture_output=True, text=True, timeout=120, env=env)  # fmt: skip
    assert res.returncode == 0 and (ncpu < 2 or json.loads(res.stdout.strip().splitlines()[-1]) == []), res.stdout[-500:] + res.stderr[-1000:]
    # the CPU budget the pools are sized to: the mask capped by the container's quota, a rank's share of it under a launcher
    def budget(env):
        res = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from trinity_amd import hostplan as HP; print(HP.cpu_budget())" % ROOT],
                             capture_output=True, text=True, timeout=120, env=env)  # fmt: skip
        assert res.returncode == 0, res.stderr[-2000:]
        return int(res.stdout.strip().splitlines()[-1])

    solo_env = {k: v for k, v in os.environ.items() if k not in ("LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    whole = budget(solo_env)
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        quota = None if q == "max" else max(1, int(int(q) / int(p)))
    except (OSError, ValueError):
        pass
    assert 1 <= whole <= ncpu and (quota is None or whole == min(ncpu, quota))
    assert budget(dict(solo_env, LOCAL_RANK="1", LOCAL_WORLD_SIZE="4")) == max(1, whole // 4)
    # without the launcher's variables: next to the creating thread, still distinct CPUs
    env = {k: v for k, v in os.environ.items() if k not in ("LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    res = subprocess.run([sys.executable, "-c", "import json, sys; sys.path.insert(0, %r); from trinity_amd import hostplan as HP; print(json.dumps(HP.pool_cpus(4)))" % ROOT],
                         capture_output=True, text=True, timeout=120, env=env)  # fmt: skip
    solo = json.loads(res.stdout.strip().splitlines()[-1])
    assert len(solo) == min(3, ncpu) and len(set(solo)) == len(solo)
