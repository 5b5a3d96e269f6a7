"""CPU tests of the surface of the stats of a column (include/trinity_hip.h: tri_batch_set_stats / tri_batch_stats / tri_cbatch_stats): the symbols are declared,
exported by the built library and bound in engine.py with the header's signatures; the limits agree between the header, the binding and the kernel's constants; the
ABI version stays 9; every export's header comment cites the reference's consumer (exec.h:12-23); the calls refuse null arguments without a device and name
themselves.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tri_batch_set_stats", "tri_batch_stats", "tri_cbatch_stats"]
TRI_ERR_INVALID = -1
SIGNATURES = {
    "tri_batch_set_stats": ("int", ["tri_batch *", "const tri_stat *stats", "size_t n"]),
    "tri_batch_stats": ("int", ["tri_batch *", "size_t k", "uint64_t *sums", "uint32_t *counts", "uint32_t *mins", "uint32_t *maxs", "size_t cap"]),
    "tri_cbatch_stats": ("int", ["tri_cbatch *", "size_t k", "uint64_t *sums", "uint64_t *counts", "uint32_t *mins", "uint32_t *maxs", "size_t cap"]),
}


@pytest.fixture(scope="module")
def L():
    import trinity_amd
    from trinity_amd.engine import hip_lib

    trinity_amd.build_all()
    return hip_lib()


def raw_header():
    return open(os.path.join(ROOT, "include", "trinity_hip.h")).read()


def header():
    return re.sub(r"/\*.*?\*/", "", raw_header(), flags=re.S)


def test_the_calls_are_declared_exported_and_bound_with_the_headers_signatures(L):
    from trinity_amd.engine import ABI_SYMBOLS

    src = header()
    for n in NAMES:
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(2).split(",")]
        assert (m.group(1), params) == SIGNATURES[n], (n, m.group(1), params)
        assert n in ABI_SYMBOLS, n
        fn = getattr(L, n)
        assert len(fn.argtypes) == len(params), n
        for p, a in zip(params, fn.argtypes):
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (n, p, a)
            else:
                assert p.startswith("size_t") and a is C.c_size_t, (n, p, a)
        assert fn.restype is C.c_int, n
    assert re.search(r"typedef\s+struct\s+tri_stat\s*\{\s*tri_column\s*\*group;\s*tri_column\s*\*value;\s*uint32_t\s+nbuckets;\s*uint32_t\s+reserved;\s*\}\s*tri_stat\s*;", src)
    assert L.tri_abi_version() == 9  # (additions within 9)
    assert int(re.search(r"#define\s+TRI_ABI_VERSION\s+(\d+)", src).group(1)) == 9


def test_every_exports_comment_cites_the_references_consumer():
    raw = raw_header()
    for n in NAMES:
        assert re.search(r"\* %s \(exec\.h:12-23\)" % n, raw), n
    assert re.search(r'"stats_last_us" \(read-only; exec\.h:12-23\)', raw)
    assert re.search(r"within 9: tri_batch_set_stats / tri_batch_stats / tri_cbatch_stats, read-only option stats_last_us", raw)


def test_the_limits_agree_between_header_binding_and_kernel():
    import trinity_amd as T
    from trinity_amd.engine import TriStat

    smax = int(re.search(r"#define\s+TRI_STATS_MAX\s+(\d+)\b", header()).group(1))
    k = S.header_constants("dev_structs.hpp")
    assert smax == T.STATS_MAX == k["STATS_MAX"] == 4
    assert len(re.findall(r"#define\s+TRI_FACET_MAX_BUCKETS\b", header())) == 1 and T.FACET_MAX_BUCKETS == k["FACET_MAX_BUCKETS"]  # (the stats' nbuckets limit is the facets')
    assert (k["STATS_LDS_BUCKETS"] + k["STATS_MAX"]) * 20 <= 16 * 1024  # (a workgroup's static LDS: four planes, 20 bytes a record, and the ungrouped stats' records)
    assert k["STATS_SHORT_SEGMENT"] in (32, 128) and k["STATS_WG"] == 256
    assert C.sizeof(TriStat) == 24 and TriStat.value.offset == 8 and TriStat.nbuckets.offset == 16 and TriStat.reserved.offset == 20
    assert callable(T.Batch.set_stats) and callable(T.Batch.stats) and callable(T.CollectionBatch.stats) and T.Stats._fields == ("sums", "counts", "mins", "maxs")


def test_null_arguments_are_refused_without_a_device_and_name_the_call(L):
    from trinity_amd.engine import TriStat

    out = np.zeros(8, dtype=np.uint64)
    spec = TriStat(None, None, 0, 0)
    p = out.ctypes.data
    for call, name in ((lambda: L.tri_batch_set_stats(None, C.byref(spec), 1), b"tri_batch_set_stats"), (lambda: L.tri_batch_set_stats(None, None, 0), b"tri_batch_set_stats"),
                       (lambda: L.tri_batch_stats(None, 0, p, p, p, p, 1), b"tri_batch_stats"), (lambda: L.tri_cbatch_stats(None, 0, p, p, p, p, 1), b"tri_cbatch_stats")):  # fmt: skip
        assert call() == TRI_ERR_INVALID and name in L.tri_last_error() and b"null argument" in L.tri_last_error(), name
    assert not out.any()
