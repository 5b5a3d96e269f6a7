"""The C++ operator surface's ProximityRanker (trinity_amd/csrc/host/trinity_gpu.hpp): the driver tests/cpp/host_mirror_rank_test.cpp runs each query twice through
exec_query's default mode — ranked on the device (tri_batch_set_ranker) and through the per-match replay into ProximityRanker::consider — and prints both lists.
They must be identical, and equal to the restatement of tests/rank_cases.py over the CPU oracle."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rank_cases as R
from wide_terms_cases import WORLDS

QUERIES = {"and2": "t0 t1", "or3": "t0 OR t1 OR t2", "phrases": '"t0 t1" OR "t1 t2" OR "t2 t3"', "opt": 't0 <"t1 t2">', "and3": "t3 t1 t0"}


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_rank_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_RANK_BIN

    assert os.path.exists(MIRROR_RANK_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_RANK_BIN], capture_output=True, text=True).stdout


@pytest.mark.gpu
def test_device_and_replay_give_the_restatements_lists(T, tmp_path):
    from trinity_amd.build import MIRROR_RANK_BIN

    D, V, slots, seed = WORLDS[0]
    seg = T.Segment(D, V, slots, seed)
    ora = O.Index.generate(D, V, slots, seed)
    ipath, tpath = str(tmp_path / "index"), str(tmp_path / "terms")
    np.asarray(seg.index).tofile(ipath)
    np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
    res = subprocess.run([MIRROR_RANK_BIN, ipath, tpath, str(D)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        name, path, n, *pairs = l.split()
        assert int(n) == len(pairs)
        lines[(name, path)] = [tuple(int(x) for x in p.split(":")) for p in pairs]
    for name, text in QUERIES.items():
        prog = O.parse_query(text)
        docs, scores, _ = R.ranked(ora.exec_rich(prog)[1], prog, 10, 3, 4.0, R.token_weights([prog], lambda k: 1 + k % 3))
        want = [(d, int(np.array([s], dtype=np.float64).view(np.uint64)[0])) for d, s in zip(docs, scores)]
        assert len(want) == 10
        assert lines[(name, "dev")] == lines[(name, "host")] == want, name
    assert lines[("none", "dev")] == lines[("none", "host")] == []
