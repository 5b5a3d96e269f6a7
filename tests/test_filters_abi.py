"""CPU tests of the per-query document filters (include/trinity_hip.h: tri_filter_create / tri_filter_from_docset / tri_filter_destroy / tri_batch_set_filters):
the symbols are declared, exported and bound; the calls refuse null handles without a device; and the filters tests/test_gpu_filters.py runs on the stream corpus
leave the oracle's top-K lists comparable by structured.check_topk — at most 10 % of the scored cases under its set-wise rule.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filter_cases as F
import oracle_lib as O
import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tri_filter_create", "tri_filter_from_docset", "tri_filter_destroy", "tri_batch_set_filters"]
TRI_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L():
    import trinity_amd
    from trinity_amd.engine import hip_lib

    trinity_amd.build_all()
    return hip_lib()


def test_the_four_calls_are_declared_exported_and_bound(L):
    from trinity_amd.engine import ABI_SYMBOLS

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trinity_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in ABI_SYMBOLS and getattr(L, n) is not None, n
    assert re.search(r"#define\s+TRI_FILTER_DROP\s+0\b", src) and re.search(r"#define\s+TRI_FILTER_KEEP\s+1\b", src)
    assert re.search(r"typedef\s+struct\s+tri_filter\s+tri_filter\s*;", src)
    assert L.tri_abi_version() == 9  # (additions within 9)


def test_python_surface():
    import trinity_amd as T

    assert (T.FILTER_DROP, T.FILTER_KEEP, T.NO_FILTER) == (0, 1, 0xFFFFFFFF)
    assert callable(T.Filter.from_docset) and callable(T.Filter.close) and callable(T.Batch.set_filters)


def test_null_handles_are_refused_without_a_device(L):
    ids = np.array([1, 2, 3], dtype=np.uint32)
    foq = np.zeros(4, dtype=np.uint32)
    out = C.c_void_p()

    def refused(rc):
        assert rc == TRI_ERR_INVALID and L.tri_last_error() and not out.value

    refused(L.tri_filter_create(None, ids.ctypes.data, ids.size, 0, C.byref(out)))
    assert b"tri_filter_create" in L.tri_last_error()
    refused(L.tri_filter_from_docset(None, 0, 1, C.byref(out)))
    assert b"tri_filter_from_docset" in L.tri_last_error()
    refused(L.tri_batch_set_filters(None, None, 0, foq.ctypes.data))
    assert b"tri_batch_set_filters" in L.tri_last_error()
    L.tri_filter_destroy(None)  # a no-op


def test_stream_filters_are_what_they_say():
    D = S.D_STREAM
    fl = F.stream_filters()
    hdr = S.header_constants("dev_structs.hpp")
    assert (hdr["SPAN_BITS"], hdr["PL_W"], hdr["FUS_W"]) == (S.SPAN_BITS, S.PL_W, S.FUS_W)
    span = set(F.dropped(fl["span"], D).tolist())
    assert {1, D, S.SPAN_BITS - 1, S.SPAN_BITS, S.SPAN_BITS + 1, 2 * S.SPAN_BITS - 1, 2 * S.SPAN_BITS, 2 * S.SPAN_BITS + 1} == span
    win = set(F.dropped(fl["windows"], D).tolist())
    for w in (S.PL_W, S.FUS_W):
        for k in range(1, D // w + 1):
            assert {k * w - 1, k * w} <= win and (k * w + 1 > D or k * w + 1 in win), (w, k)
    kept = np.setdiff1d(np.arange(1, D + 1), F.dropped(fl["one"], D))
    assert sorted((kept // S.SPAN_BITS).tolist()) == [0, 1, 2]  # one document in each of the three windows
    assert F.dropped(fl["all"], D).size == D and F.dropped(fl["empty"], D).size == 0


def test_filtered_top_k_stays_inside_the_tie_cap():
    """structured.check_topk's set-wise rule (distinct oracle scores within rtol of each other among ranks 1 .. K + 1) may decide at most 10 % of the scored cases
    tests/test_gpu_filters.py compares: every stream query under every stream filter and unfiltered, top-10, on the oracle with the filter as its masked set."""
    c = S.stream_corpus()
    ora = c.oracle()
    queries = F.stream_queries(c)
    progs = S.programs(queries)
    cases = setwise = 0
    smallest = np.inf
    try:
        for name, flt in list(F.stream_filters().items()) + [("none", (np.zeros(0, np.uint32), False))]:
            ora.set_masked(F.dropped(flt, c.D))
            for p in progs:
                docs, scores = ora.exec(p, O.FLAG_ACCUM_SCORE)
                if not len(docs):
                    continue  # (nothing to rank: no comparison rule involved)
                exact, gap = S.score_gaps(scores, F.K)
                cases += 1
                setwise += not exact
                smallest = min(smallest, gap)
    finally:
        ora.set_masked(np.zeros(0, np.uint32))
    print(f"filtered score-gap condition: {setwise} of {cases} scored cases ({100.0 * setwise / cases:.1f} %) under the set-wise rule; smallest relative gap {smallest:.3g}")
    # (six runs per query; `all` ranks nothing and `one` little: at least four of the six rank something for every query)
    assert cases >= 4 * len(progs) and setwise <= 0.10 * cases, (setwise, cases)
