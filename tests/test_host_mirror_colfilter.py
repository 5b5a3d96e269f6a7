"""The C++ operator surface with a filter made of COLUMN PREDICATES (trinity_amd/csrc/host/trinity_gpu.hpp: ColumnPredicateFilter, an IndexDocumentsFilter over
DeviceColumns built on the device through tri_filters_from_columns): the driver tests/cpp/host_mirror_colfilter_test.cpp runs exec_query with it on the device — as an
allow-list and in the drop form of the same rule —, through the replay (filter(id) answered by csrc/host/column_pred.hpp from the columns' host copies) and with a plain
host filter of the same rule, in DocumentsOnly, AccumulatedScore and the default mode; the lists must be equal — and equal to the oracle's matches that the rule keeps."""
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


def test_colfilter_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_COLFILTER_BIN

    assert os.path.exists(MIRROR_COLFILTER_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_COLFILTER_BIN], capture_output=True, text=True).stdout


@pytest.mark.gpu
def test_column_predicate_filter_on_the_device_equals_the_replay_and_the_host_filter(T, tmp_path):
    from trinity_amd.build import MIRROR_COLFILTER_BIN

    D, V = 20000, 500
    seg = T.Segment(D, V, 12, 7)
    ora = O.Index.generate(D, V, 12, 7)
    ipath, tpath = str(tmp_path / "index"), str(tmp_path / "terms")
    np.asarray(seg.index).tofile(ipath)
    np.ascontiguousarray(seg.terms, dtype=np.uint32).tofile(tpath)
    res = subprocess.run([MIRROR_COLFILTER_BIN, ipath, tpath, str(D)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = {}
    for l in res.stdout.splitlines():
        k, _, rest = l.partition(" ")
        lines[k] = rest.split()
    assert lines["device_filter"] == ["device=1", "drop=1", "replay=0", "plain=0"]

    def keep(d):  # the driver's rule
        price, cat = d * 7 % 1000, d % 11
        return (price >= 100) & (price <= 600) & np.isin(cat, [3, 5, 8])

    every = np.arange(1, D + 1)
    assert lines["bitmap"] == [f"words={(D // 131072 + 2) * 4096}", "differ=0", f"dropped={int((~keep(every)).sum())}"]
    docs, scores = ora.exec(O.parse_query("t0 (t1 OR t2 OR t3)"), O.FLAG_ACCUM_SCORE)
    m = keep(docs)
    assert 0 < m.sum() < len(docs)
    want = [str(x) for x in docs[m].tolist()]
    assert lines["docs_device"] == lines["docs_dropform"] == lines["docs_replay"] == lines["docs_host"] == want
    assert lines["scored_device"] == lines["scored_dropform"] == lines["scored_replay"] == lines["scored_host"]
    got = [x.split(":") for x in lines["scored_device"]]
    assert [int(a) for a, _ in got] == docs[m].tolist()
    np.testing.assert_allclose([float(b) for _, b in got], scores[m], rtol=1e-9, atol=0)
    assert lines["docs_asked"] == [f"host={len(docs)}"] and lines["scored_asked"] == [f"host={len(docs)}"]
    assert lines["rich_device"] == lines["rich_replay"] == lines["rich_host"] == want
    assert lines["batch_filtered"] == want and lines["batch_plain"] == [str(x) for x in docs.tolist()]
    other = ora.exec(O.parse_query("t8 OR t9"), O.FLAG_DOCUMENTS_ONLY)[0]
    assert lines["batch_other"] == [str(x) for x in other[keep(other)].tolist()]
    price = docs * 7 % 1000
    both = (docs % 2 == 0) & (price >= 100) & (price <= 600)
    assert lines["also_differ"] == ["0"] and 0 < both.sum() < m.sum() + len(docs) and lines["also_device"] == [str(x) for x in docs[both].tolist()]
    assert lines["set_value_65536"] == ["refused"]
