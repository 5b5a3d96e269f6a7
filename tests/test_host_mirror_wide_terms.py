"""The C++ operator surface's default mode on queries of more than 16 terms (trinity_amd/csrc/host/trinity_gpu.hpp: exec_query_default_mode through the _wide result
calls, IndexSource::set_option("rich_max_terms", 64)): the driver tests/cpp/host_mirror_wide_terms_test.cpp folds what consider(const matched_document &) receives
into the oracle's canonical default-mode stream and prints its hash; it must be the hash of the oracle's own stream."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from wide_terms_cases import SHAPES, WORLDS


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_wide_terms_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_WIDE_TERMS_BIN

    assert os.path.exists(MIRROR_WIDE_TERMS_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_WIDE_TERMS_BIN], capture_output=True, text=True).stdout


@pytest.mark.gpu
def test_default_mode_delivers_the_oracles_stream_for_wide_report_queries(T, tmp_path):
    from trinity_amd.build import MIRROR_WIDE_TERMS_BIN

    D, V, slots, seed = WORLDS[0]
    seg = T.Segment(D, V, slots, seed)
    ora = O.Index.generate(D, V, slots, seed)
    ipath, tpath = str(tmp_path / "index"), str(tmp_path / "terms")
    np.asarray(seg.index).tofile(ipath)
    np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
    res = subprocess.run([MIRROR_WIDE_TERMS_BIN, ipath, tpath, str(D)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        k, _, rest = l.partition(" ")
        lines[k] = rest.split()
    texts = {sh[0]: (sh[1], sh[2]) for sh in SHAPES}
    texts["or3"] = ("t0 OR t1 OR t2", 1)
    for name in ("or33", "straddle", "or3"):
        docs, flat, tt, ht = ora.exec_rich(O.parse_query(texts[name][0], some_min=texts[name][1]))
        got = lines[name]
        assert got[1:4] == [f"matches={len(docs)}", f"terms={tt}", f"hits={ht}"], (name, got)
        assert got[0] == str(O.fnv1a_u32_stream(flat)), name
    assert 1 <= int(lines["or33"][4].split("=")[1]) <= slots  # (the widest matched_document: a document of this corpus holds at most `slots` terms)
    assert lines["default"] == ["exception"]  # left out at the default, as ever: run_batch turns the query's status into the exception it always threw
