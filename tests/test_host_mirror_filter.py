"""The C++ operator surface with a filter the DEVICE applies (trinity_amd/csrc/host/trinity_gpu.hpp: DeviceDocumentsFilter, IndexDocumentsFilter::device_filter): the
driver tests/cpp/host_mirror_filter_test.cpp runs exec_query with it and with the equivalent plain host filter, in DocumentsOnly and AccumulatedScore mode, and prints
both result lists; they must be equal — and equal to the oracle's matches that the rule keeps."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_filter_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_FILTER_BIN

    assert os.path.exists(MIRROR_FILTER_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_FILTER_BIN], capture_output=True, text=True).stdout


@pytest.mark.gpu
def test_device_filter_equals_the_host_filter(T, tmp_path):
    from trinity_amd.build import MIRROR_FILTER_BIN

    D, V = 20000, 500
    seg = T.Segment(D, V, 12, 7)
    ora = O.Index.generate(D, V, 12, 7)
    ipath, tpath = str(tmp_path / "index"), str(tmp_path / "terms")
    np.asarray(seg.index).tofile(ipath)
    np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
    res = subprocess.run([MIRROR_FILTER_BIN, ipath, tpath, str(D)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        k, _, rest = l.partition(" ")
        lines[k] = rest.split()
    assert lines["device_filter"] == ["handle=1", "plain=0"]
    keep = lambda d: (d % 3 != 0) & (d <= 15000)  # noqa: E731  (the driver's rule)
    docs, scores = ora.exec(O.parse_query("t0 (t1 OR t2 OR t3)"), O.FLAG_ACCUM_SCORE)
    m = keep(docs)
    assert 0 < m.sum() < len(docs)
    # DocumentsOnly: the device's filter, the same rule as an allow-list, the host's filter
    assert lines["docs_device"] == lines["docs_allow"] == lines["docs_host"] == [str(x) for x in docs[m].tolist()]
    # AccumulatedScore: ids and scores
    assert lines["scored_device"] == lines["scored_allow"] == lines["scored_host"]
    got = [x.split(":") for x in lines["scored_device"]]
    assert [int(a) for a, _ in got] == docs[m].tolist()
    np.testing.assert_allclose([float(b) for _, b in got], scores[m], rtol=1e-9, atol=0)
    # the host filter is asked once per match of the UNFILTERED query; the device's never (its matches arrive filtered)
    assert lines["docs_asked"] == [f"host={len(docs)}"] and lines["scored_asked"] == [f"host={len(docs)}"]
    assert lines["rich_device"] == lines["rich_host"] == lines["docs_device"]
    # exec_queries: a filter per query
    assert lines["batch_filtered"] == lines["docs_device"] and lines["batch_plain"] == [str(x) for x in docs.tolist()]
    other = ora.exec(O.parse_query("t8 OR t9"), O.FLAG_DOCUMENTS_ONLY)[0]
    assert lines["batch_other"] == [str(x) for x in other[keep(other)].tolist()]
    assert lines["host_filter_in_batch"] == ["invalid_argument"]
