"""StatsCounter on the C++ operator surface (trinity_amd/csrc/host/trinity_gpu.hpp: StatsCounter, MatchedIndexDocumentsFilter::device_consumer).  The driver
tests/cpp/host_mirror_stats_test.cpp aggregates three queries by four stats — one ungrouped — over the three sources of tests/crank_cases.py: on the device (exec_query
sets the stats and reads tri_batch_stats) and through the replay (consider(ids, cnt) on the host), under a device filter, under a host filter, and over the collection
(each source under the registry of the newer ones, the records combined).  Device, replay and tests/stats_cases.py::stats_rows over the CPU oracle's sets must agree,
integer for integer."""
import os
import subprocess

import numpy as np
import pytest

import crank_cases as CR
import oracle_lib as O
import stats_cases as X

QUERIES = ["t0 t1", "t0 OR t1 OR t2", "t3 (t4 OR t5)"]  # (the driver's)
STATS = [(None, 0, "hash"), ("mod7", 5, "hash"), ("huge", 5, "low16"), ("low16", 1000, "huge")]
NONE = np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_stats_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_STATS_BIN

    assert os.path.exists(MIRROR_STATS_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_STATS_BIN], capture_output=True, text=True).stdout


def rows_of(sets, D):
    cols = X.columns(D)
    return [X.stats_rows(sets, None if g is None else cols[g], nb, cols[v]) for g, nb, v in STATS]


def planes(rows, q):
    return {name: [int(x) for x in p[q]] for name, p in zip(X.Stats._fields, rows)}


@pytest.mark.gpu
def test_device_replay_and_stats_rows_agree(T, tmp_path):
    from trinity_amd.build import MIRROR_STATS_BIN

    args = []
    for si, w in enumerate(CR.WORLDS):
        seg = T.Segment(*w)
        ipath, tpath = str(tmp_path / f"index{si}"), str(tmp_path / f"terms{si}")
        np.asarray(seg.index).tofile(ipath)
        np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
        args += [ipath, tpath, str(w[0]), str(CR.UPDATES[si])]
    res = subprocess.run([MIRROR_STATS_BIN] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        parts = l.split()
        if parts[0] in ("single", "filtered", "collection"):
            n = 6 if parts[0] == "single" else 5
            lines[tuple(parts[:n])] = [int(x) for x in parts[n:]]
    assert "unbound invalid_argument" in res.stdout and "ungrouped-with-buckets invalid_argument" in res.stdout

    def got(*key):
        return {name: lines[key + (name,)] for name in X.Stats._fields}

    progs = [O.parse_query(q) for q in QUERIES]
    parts = [[[] for _ in STATS] for _ in QUERIES]
    for si, (D, *_) in enumerate(CR.WORLDS):
        ora = CR.oracle_of(si)
        plain = rows_of([ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs], D)
        for q in range(len(QUERIES)):
            for k in range(len(STATS)):
                want = planes(plain[k], q)
                assert got("single", str(si), str(q), "device", str(k)) == got("single", str(si), str(q), "replay", str(k)) == want, (si, q, k)
        if si == 0:
            s = ora.exec(progs[0], O.FLAG_DOCUMENTS_ONLY)[0]
            kept = rows_of([s[s % 4 != 1]], D)
            assert 0 < len(s[s % 4 != 1]) < len(s)
            for k in range(len(STATS)):
                for where in ("ondevice", "onhost"):
                    for mode in ("device", "replay"):
                        assert got("filtered", where, mode, str(k)) == planes(kept[k], 0), (where, mode, k)
        ora.set_masked(CR.masks()[si])
        try:
            under = rows_of([ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs], D)
        finally:
            ora.set_masked(NONE)
        for q in range(len(QUERIES)):
            for k in range(len(STATS)):
                parts[q][k].append(X.Stats(*(p[q : q + 1] for p in under[k])))
    for q in range(len(QUERIES)):
        for k in range(len(STATS)):
            want = planes(X.combine(parts[q][k]), 0)
            assert got("collection", str(q), "device", str(k)) == got("collection", str(q), "replay", str(k)) == want, (q, k)
    assert sum(planes(X.combine(parts[0][0]), 0)["counts"]) > 0
