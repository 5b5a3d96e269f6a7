"""ColumnOrder on the C++ operator surface (trinity_amd/csrc/host/trinity_gpu.hpp: ColumnOrder, MatchedIndexDocumentsFilter::device_consumer).  The driver
tests/cpp/host_mirror_order_test.cpp lists three queries' first K by two columns over the three sources of tests/crank_cases.py — on the device (exec_query sets the
order and reads tri_batch_ordered) and through the replay (consider(ids, cnt) on the host), under a device filter, under a host filter, and over the collection (each
source under the registry of the newer ones, the lists blended).  Device, replay and tests/order_cases.py::first_k / blend over the CPU oracle's sets must agree,
integer for integer."""
import os
import subprocess

import numpy as np
import pytest

import crank_cases as CR
import oracle_lib as O
import order_cases as OC

QUERIES = ["t0 t1", "t0 OR t1 OR t2", "t3 (t4 OR t5)"]  # (the driver's)
COLUMNS = ["mod7", "hash"]
NONE = np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_order_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_ORDER_BIN

    assert os.path.exists(MIRROR_ORDER_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_ORDER_BIN], capture_output=True, text=True).stdout


def flat(d, v):
    return [int(x) for pair in zip(d.tolist(), v.tolist()) for x in pair]


@pytest.mark.gpu
def test_device_replay_and_first_k_agree(T, tmp_path):
    from trinity_amd.build import MIRROR_ORDER_BIN

    args = []
    for si, w in enumerate(CR.WORLDS):
        seg = T.Segment(*w)
        ipath, tpath = str(tmp_path / f"index{si}"), str(tmp_path / f"terms{si}")
        np.asarray(seg.index).tofile(ipath)
        np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
        args += [ipath, tpath, str(w[0]), str(CR.UPDATES[si])]
    res = subprocess.run([MIRROR_ORDER_BIN] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        parts = l.split()
        n = {"single": 7, "filtered": 3, "collection": 6}.get(parts[0])
        if n:
            lines[tuple(parts[:n])] = [int(x) for x in parts[n:]]
    assert "unbound invalid_argument" in res.stdout
    progs = [O.parse_query(q) for q in QUERIES]
    under = []
    for si, (D, *_) in enumerate(CR.WORLDS):
        ora = CR.oracle_of(si)
        cols = OC.columns(D)
        sets = [ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs]
        for q in range(len(QUERIES)):
            for name in COLUMNS:
                for k in (1, 10, 256):
                    for desc, way in ((False, "up"), (True, "down")):
                        want = flat(*OC.first_k(sets[q], cols[name], k, desc))
                        key = ("single", str(si), str(q), name, str(k), way)
                        assert lines[key + ("device",)] == lines[key + ("replay",)] == want, key
        if si == 0:
            s = sets[0]
            kept = s[s % 4 != 1]
            assert 0 < len(kept) < len(s)
            want = flat(*OC.first_k(kept, cols["hash"], 10))
            for where in ("ondevice", "onhost"):
                for mode in ("device", "replay"):
                    assert lines["filtered", where, mode] == want, (where, mode)
        ora.set_masked(CR.masks()[si])
        try:
            under.append([ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs])
        finally:
            ora.set_masked(NONE)
    seen = 0
    for q in range(len(QUERIES)):
        for name in COLUMNS:
            for k in (10, 256):
                for desc, way in ((False, "up"), (True, "down")):
                    parts = [OC.first_k(under[si][q], OC.columns(D)[name], k, desc) for si, (D, *_) in enumerate(CR.WORLDS)]
                    want = flat(*OC.blend(parts, k, desc))
                    key = ("collection", str(q), name, str(k), way)
                    assert lines[key + ("device",)] == lines[key + ("replay",)] == want, key
                    seen += len(want)
    assert seen > 0
