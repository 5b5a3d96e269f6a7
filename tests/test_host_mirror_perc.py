"""The percolator on the C++ operator surface (trinity_amd/csrc/host/trinity_gpu.hpp: percolator_query, percolator_document_proxy, PercolatorSet).  The driver
tests/cpp/host_mirror_perc_test.cpp stores a case file's queries in a PercolatorSet, matches its documents on the device in both orders and compares every query's
answer with percolator_query::match over a proxy; the pairs it prints must be the restatement's (tests/perc_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

import perc_cases as PC
from random_programs import random_program


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_perc_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_PERC_BIN

    assert os.path.exists(MIRROR_PERC_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_PERC_BIN], capture_output=True, text=True).stdout


@pytest.mark.gpu
def test_the_set_on_the_device_equals_the_recursion_on_the_host(T, tmp_path):
    from trinity_amd.build import MIRROR_PERC_BIN

    rng = np.random.default_rng(13)
    programs, docs = [], []
    for fam in PC.FAMILIES.values():
        p, d, _ = fam()
        programs += p
        docs += d
    programs += [[]] + [random_program(rng, True).tolist() for _ in range(200)]
    docs += [{int(t): [int(x) for x in np.sort(rng.integers(0, 9, size=rng.integers(0, 4)))] for t in rng.choice(40, size=rng.integers(0, 14), replace=False)} for _ in range(80)]
    path = str(tmp_path / "cases.txt")
    PC.write_case_file(path, programs, docs)
    res = subprocess.run([MIRROR_PERC_BIN, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = res.stdout.splitlines()
    got = {k: [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith(k + " ")] for k in ("q", "d")}
    (q1, d1), (q2, d2), _ = PC.pairs_of(PC.match_batch(programs, docs), len(docs))
    assert got["q"] == list(zip(q1.tolist(), d1.tolist())) and got["d"] == list(zip(q2.tolist(), d2.tolist())) and q1.size > 500
    assert "refused 1" in lines
