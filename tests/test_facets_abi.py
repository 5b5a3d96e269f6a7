"""CPU tests of the facet counts' surface (include/trinity_hip.h: tri_column_create / tri_column_destroy / tri_batch_set_facets / tri_batch_facets / tri_cbatch_facets):
the symbols are declared, exported by the built library and bound in engine.py with the header's signatures; the two limits agree between the header, the binding and
the kernels' constants; the calls refuse null handles without a device.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tri_column_create", "tri_column_destroy", "tri_batch_set_facets", "tri_batch_facets", "tri_cbatch_facets"]
TRI_ERR_INVALID = -1
# the header's parameter lists, as ctypes (a pointer parameter: c_void_p or a POINTER; size_t: c_size_t)
SIGNATURES = {
    "tri_column_create": ("int", ["tri_index *", "const uint32_t *values", "size_t n", "tri_column **out"]),
    "tri_column_destroy": ("void", ["tri_column *"]),
    "tri_batch_set_facets": ("int", ["tri_batch *", "const tri_facet *facets", "size_t n"]),
    "tri_batch_facets": ("int", ["tri_batch *", "size_t k", "uint32_t *counts", "size_t cap"]),
    "tri_cbatch_facets": ("int", ["tri_cbatch *", "size_t k", "uint64_t *counts", "size_t cap"]),
}


@pytest.fixture(scope="module")
def L():
    import trinity_amd
    from trinity_amd.engine import hip_lib

    trinity_amd.build_all()
    return hip_lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trinity_hip.h")).read(), flags=re.S)


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
        assert fn.restype is (None if m.group(1) == "void" else C.c_int), n
    assert re.search(r"typedef\s+struct\s+tri_column\s+tri_column\s*;", src)
    assert re.search(r"typedef\s+struct\s+tri_facet\s*\{\s*tri_column\s*\*column;\s*uint32_t\s+nbuckets;\s*uint32_t\s+reserved;\s*\}\s*tri_facet\s*;", src)
    assert L.tri_abi_version() == 9  # (additions within 9)


def test_the_limits_agree_between_header_binding_and_kernels():
    import trinity_amd as T
    from trinity_amd.engine import TriFacet

    src = header()
    fmax = int(re.search(r"#define\s+TRI_FACETS_MAX\s+(\d+)\b", src).group(1))
    bmax = int(re.search(r"#define\s+TRI_FACET_MAX_BUCKETS\s+(\d+)u\b", src).group(1))
    k = S.header_constants("dev_structs.hpp")
    assert fmax == T.FACETS_MAX == k["FACETS_MAX"] == 4
    assert bmax == T.FACET_MAX_BUCKETS == k["FACET_MAX_BUCKETS"] == 65536
    assert 0 < k["FACET_SHORT_SEGMENT"] and k["FACET_LDS_COUNTERS"] * 4 <= 64 * 1024  # (an LDS row: 64 KB a workgroup at the very most)
    assert C.sizeof(TriFacet) == 16 and TriFacet.nbuckets.offset == 8 and TriFacet.reserved.offset == 12
    assert callable(T.Column.close) and callable(T.Batch.set_facets) and callable(T.Batch.facets) and callable(T.CollectionBatch.facets)


def test_null_handles_are_refused_without_a_device(L):
    from trinity_amd.engine import TriFacet

    vals = np.zeros(4, dtype=np.uint32)
    out = C.c_void_p()
    spec = (TriFacet * 1)()
    for call, name in ((lambda: L.tri_column_create(None, vals.ctypes.data, vals.size, C.byref(out)), b"tri_column_create"), (lambda: L.tri_batch_set_facets(None, spec, 1), b"tri_batch_set_facets"),
                       (lambda: L.tri_batch_facets(None, 0, vals.ctypes.data, vals.size), b"tri_batch_facets"), (lambda: L.tri_cbatch_facets(None, 0, vals.ctypes.data, 2), b"tri_cbatch_facets")):  # fmt: skip
        assert call() == TRI_ERR_INVALID and name in L.tri_last_error() and not out.value, name
    L.tri_column_destroy(None)  # (a null column: nothing to do)
