"""FacetCounter on the C++ operator surface (trinity_amd/csrc/host/trinity_gpu.hpp: DeviceColumn, FacetCounter, MatchedIndexDocumentsFilter::device_consumer).  The driver
tests/cpp/host_mirror_facets_test.cpp counts three queries by four facets over the three sources of tests/crank_cases.py — on the device (exec_query sets the facets and
reads tri_batch_facets) and through the replay (consider(ids, cnt) on the host), under a device filter, under a host filter, and over the collection (each source under
the registry of the newer ones, the counters summed).  Device, replay and tests/facet_cases.py::facet_rows over the CPU oracle's sets must agree, integer for integer."""
import os
import subprocess

import numpy as np
import pytest

import crank_cases as CR
import facet_cases as F
import oracle_lib as O

QUERIES = ["t0 t1", "t0 OR t1 OR t2", "t3 (t4 OR t5)"]  # (the driver's)
FACETS = [("mod7", 7), ("mod7", 5), ("huge", 5), ("low16", 4096)]
NONE = np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_facets_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_FACETS_BIN

    assert os.path.exists(MIRROR_FACETS_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_FACETS_BIN], capture_output=True, text=True).stdout


def rows_of(sets, D):
    cols = F.columns(D)
    return [F.facet_rows(sets, cols[name], nb) for name, nb in FACETS]


@pytest.mark.gpu
def test_device_replay_and_facet_rows_agree(T, tmp_path):
    from trinity_amd.build import MIRROR_FACETS_BIN

    args = []
    for si, w in enumerate(CR.WORLDS):
        seg = T.Segment(*w)
        ipath, tpath = str(tmp_path / f"index{si}"), str(tmp_path / f"terms{si}")
        np.asarray(seg.index).tofile(ipath)
        np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
        args += [ipath, tpath, str(w[0]), str(CR.UPDATES[si])]
    res = subprocess.run([MIRROR_FACETS_BIN] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        parts = l.split()
        if parts[0] in ("single", "filtered", "collection"):
            n = 5 if parts[0] == "single" else 4
            lines[tuple(parts[:n])] = [int(x) for x in parts[n:]]
    assert "unbound invalid_argument" in res.stdout
    progs = [O.parse_query(q) for q in QUERIES]
    total = [[np.zeros(nb + 1, dtype=np.uint64) for _, nb in FACETS] for _ in QUERIES]
    for si, (D, *_) in enumerate(CR.WORLDS):
        ora = CR.oracle_of(si)
        plain = rows_of([ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs], D)
        for q in range(len(QUERIES)):
            for k in range(len(FACETS)):
                want = plain[k][q].tolist()
                assert lines["single", str(si), str(q), "device", str(k)] == lines["single", str(si), str(q), "replay", str(k)] == want, (si, q, k)
        if si == 0:
            s = ora.exec(progs[0], O.FLAG_DOCUMENTS_ONLY)[0]
            kept = rows_of([s[s % 4 != 1]], D)
            assert 0 < len(s[s % 4 != 1]) < len(s)
            for k in range(len(FACETS)):
                for where in ("ondevice", "onhost"):
                    for mode in ("device", "replay"):
                        assert lines["filtered", where, mode, str(k)] == kept[k][0].tolist(), (where, mode, k)
        ora.set_masked(CR.masks()[si])
        try:
            under = rows_of([ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs], D)
        finally:
            ora.set_masked(NONE)
        for q in range(len(QUERIES)):
            for k in range(len(FACETS)):
                total[q][k] += under[k][q]
    for q in range(len(QUERIES)):
        for k in range(len(FACETS)):
            assert lines["collection", str(q), "device", str(k)] == lines["collection", str(q), "replay", str(k)] == total[q][k].tolist(), (q, k)
    assert int(total[0][0].sum()) > 0
