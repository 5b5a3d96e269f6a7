"""CPU tests of the C-ABI of column predicates as document filters (include/trinity_hip.h: tri_filters_from_columns / tri_filter_bitmap): the two calls, the two structs
and the limits are declared, exported, bound and mirrored by csrc/dev_structs.hpp and the Python package; the ABI version stays 9; and the refusals that need no device —
null arguments, a bad mode, a bad count of predicates or clauses, non-zero reserved fields, null clause arrays and columns — come back as TRI_ERR_INVALID with `out`
untouched and a message that names the predicate and the clause.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tri_filters_from_columns", "tri_filter_bitmap"]
TRI_ERR_INVALID = -1


@pytest.fixture(scope="module")
def L():
    import trinity_amd
    from trinity_amd.engine import hip_lib

    trinity_amd.build_all()
    return hip_lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trinity_hip.h")).read(), flags=re.S)


def test_exports_equal_the_header_equal_the_python_list(L):
    from trinity_amd.engine import ABI_SYMBOLS

    src = header()
    declared = set(re.findall(r"\b(tri_\w+)\s*\(", src))
    assert declared == set(ABI_SYMBOLS) and len(ABI_SYMBOLS) == len(set(ABI_SYMBOLS))
    for n in ABI_SYMBOLS:
        assert getattr(L, n) is not None, n
    # ... and the library's own dynamic symbol table: every declared call is exported, and nothing named tri_* is exported that the header does not declare —
    # but for the one link between two of the library's translation units (commit_sort.hip's sort, called by write_side.hpp), which predates this file
    from trinity_amd.build import LIB_HIP

    table = subprocess.run(["nm", "-D", "--defined-only", LIB_HIP], capture_output=True, text=True, check=True).stdout
    exported = {f[2] for f in (l.split() for l in table.splitlines()) if len(f) == 3 and f[1] in "TW" and f[2].startswith("tri_")}
    assert exported - {"tri_sort_pairs_u64_u32"} == declared, (sorted(exported - declared), sorted(declared - exported))
    for n in NAMES:
        assert n in declared and n in ABI_SYMBOLS
    assert re.search(r"#define\s+TRI_ABI_VERSION\s+9\b", open(os.path.join(ROOT, "include", "trinity_hip.h")).read()) and L.tri_abi_version() == 9  # (additions within 9)


def test_limits_and_structs_are_declared_and_mirrored():
    import trinity_amd as T
    from trinity_amd.engine import TriClause, TriPredicate

    src = header()
    want = {"TRI_PRED_MAX_CLAUSES": 8, "TRI_PRED_MAX_COLUMNS": 8, "TRI_PREDS_MAX": 256, "TRI_CLAUSE_RANGE": 0, "TRI_CLAUSE_SET": 1}
    for k, v in want.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (k, v), src), k
    hdr = S.header_constants("dev_structs.hpp")
    assert (hdr["COLFILTER_MAX_CLAUSES"], hdr["COLFILTER_MAX_COLUMNS"], hdr["COLFILTER_MAX_PREDS"], hdr["COLFILTER_RANGE"], hdr["COLFILTER_SET"]) == (8, 8, 256, 0, 1)
    assert hdr["COLFILTER_CHUNK"] % 64 == 0 and hdr["SPAN_BITS"] % hdr["COLFILTER_CHUNK"] == 0 and hdr["COLFILTER_MAX_COLUMNS"] * hdr["COLFILTER_CHUNK"] * 4 <= 64 << 10
    assert hdr["COLFILTER_WAVE_WORDS"] * 32 * (hdr["COLFILTER_WG"] // 64) == hdr["COLFILTER_CHUNK"] and hdr["COLFILTER_WAVE_WORDS"] <= 64
    assert (T.PRED_MAX_CLAUSES, T.PRED_MAX_COLUMNS, T.PREDS_MAX, T.CLAUSE_RANGE, T.CLAUSE_SET) == (8, 8, 256, 0, 1)
    assert re.search(r"typedef\s+struct\s+tri_clause\s*\{[^}]*\}\s*tri_clause\s*;", src) and re.search(r"typedef\s+struct\s+tri_predicate\s*\{[^}]*\}\s*tri_predicate\s*;", src)
    # the layouts of the header's structs on an LP64 target
    assert C.sizeof(TriClause) == 40 and [getattr(TriClause, f).offset for f, _ in TriClause._fields_] == [0, 8, 12, 16, 20, 24, 32, 36]
    assert C.sizeof(TriPredicate) == 32 and [getattr(TriPredicate, f).offset for f, _ in TriPredicate._fields_] == [0, 8, 12, 16, 24]
    assert callable(T.Filter.from_columns) and callable(T.Filter.bitmap) and callable(T.Clause.range) and callable(T.Clause.among) and callable(T.Predicate)


def test_refusals_that_need_no_device(L):
    from trinity_amd.engine import TriClause, TriPredicate

    index, colmem = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()  # non-null handles: every refusal below is decided before a handle is looked into
    ix, column = C.cast(index, C.c_void_p), C.cast(colmem, C.c_void_p)
    out = (C.c_void_p * 2)()
    words = np.zeros(4, dtype=np.uint32)
    n = C.c_size_t(77)

    def pred(nclauses=1, reserved=0, clauses=True, col=True, creserved=0):
        cl = (TriClause * 8)()
        cl[0].column, cl[0].kind, cl[0].lo, cl[0].hi, cl[0].reserved = (column if col else None), 0, 1, 2, creserved
        p = TriPredicate()
        p.clauses, p.nclauses, p.reserved = (cl if clauses else None), nclauses, reserved
        p._alive = cl
        return p

    def call(preds, np_, mode, ix=ix, out=out):
        arr = (TriPredicate * max(1, len(preds)))(*preds) if preds is not None else None
        return L.tri_filters_from_columns(ix, arr, np_, mode, out)

    def refused(rc, *msg):
        text = L.tri_last_error().decode()
        assert rc == TRI_ERR_INVALID and not out[0] and not out[1], (rc, text)
        assert "tri_filters_from_columns" in text and all(m in text for m in msg), text

    refused(call([pred()], 1, 1, ix=None), "null argument")
    refused(call(None, 1, 1), "null argument")
    refused(call([pred()], 1, 1, out=None), "null argument")
    refused(call([pred()], 1, 2), "mode 2")
    refused(call([pred()], 0, 0), "0 predicates")
    refused(call([pred()] * 2, 257, 0), "257 predicates")
    refused(call([pred(nclauses=0)], 1, 0), "predicate 0", "0 clauses")
    refused(call([pred(nclauses=9)], 1, 0), "predicate 0", "9 clauses")
    refused(call([pred(reserved=5)], 1, 1), "predicate 0", "reserved")
    refused(call([pred(clauses=False)], 1, 1), "predicate 0", "null argument")
    refused(call([pred(col=False)], 1, 1), "predicate 0 clause 0", "null argument")
    # tri_filter_bitmap
    assert L.tri_filter_bitmap(None, words.ctypes.data, words.size, C.byref(n)) == TRI_ERR_INVALID and b"tri_filter_bitmap" in L.tri_last_error() and n.value == 77
    assert not words.any()
