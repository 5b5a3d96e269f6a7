"""The C++ operator surface's collection form (trinity_amd/csrc/host/trinity_gpu.hpp): IndexSourcesCollection, exec_query<T>(roots, collection, ...) and
ProximityRanker::blend.  The driver tests/cpp/host_mirror_collection_test.cpp runs each query over the three sources of tests/crank_cases.py — every source under
the registry of the sources newer than it — once ranked on the device and once through the per-match replay, and prints the blended lists.  They must be identical,
and equal to the restatement of tests/crank_cases.py over the CPU oracle."""
import os
import subprocess

import numpy as np
import pytest

import crank_cases as CR
import oracle_lib as O

QUERIES = {"and2": "t0 t1", "or3": "t0 OR t1 OR t2", "phrases": '"t0 t1" OR "t1 t2" OR "t2 t3"', "opt": 't0 <"t1 t2">', "and3": "t3 t1 t0"}


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_collection_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_COLLECTION_BIN

    assert os.path.exists(MIRROR_COLLECTION_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_COLLECTION_BIN], capture_output=True, text=True).stdout


@pytest.mark.gpu
def test_device_and_replay_blend_to_the_restatements_lists(T, tmp_path):
    from trinity_amd.build import MIRROR_COLLECTION_BIN

    args = [MIRROR_COLLECTION_BIN, str(CR.K)]
    for si, (D, V, slots, seed) in enumerate(CR.WORLDS):
        seg = T.Segment(D, V, slots, seed)
        ipath, tpath = str(tmp_path / f"index{si}"), str(tmp_path / f"terms{si}")
        np.asarray(seg.index).tofile(ipath)
        np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
        args += [ipath, tpath, str(D), str(CR.UPDATES[si])]
    res = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        name, path, n, *pairs = l.split()
        assert int(n) == len(pairs)
        lines[(name, path)] = [tuple(int(x) for x in p.split(":")) for p in pairs]
    sources_seen = set()
    for name, text in QUERIES.items():
        prog = O.parse_query(text)
        rows = CR.want(prog, CR.K, CR.CAP, CR.ADJ, CR.w3)
        want = [(r[0], CR.bits(r[1])) for r in rows]
        sources_seen |= {r[-1] for r in rows}
        assert len(want) == CR.K
        assert lines[(name, "dev")] == lines[(name, "host")] == want, name
    assert sources_seen == {0, 1, 2}  # (the blended lists draw on every source)
    assert lines[("none", "dev")] == lines[("none", "host")] == []
