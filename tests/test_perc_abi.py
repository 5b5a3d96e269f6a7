"""The C-ABI of the percolator (CPU: no device is touched): the tri_perc_* entry points are exported, engine.py lists and binds them, the ABI version did not move,
include/trinity_hip.h declares each with its percolator.cpp citation, NULL arguments are refused with nothing written, and — through the host library, which
compiles the same lowering and the same document check as the engine — a malformed program fails the call while an oversize one does not, and every refusal of a
batch of documents names what is wrong."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["tri_perc_create", "tri_perc_query_status", "tri_perc_set_enabled", "tri_perc_get_info", "tri_perc_destroy", "tri_perc_match", "tri_perc_result_pairs",
           "tri_perc_result_doc_counts", "tri_perc_result_get_info", "tri_perc_result_destroy"]  # fmt: skip
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_the_exports_resolve_and_the_version_stays(T):
    L = T.engine.hip_lib()
    for name in EXPORTS:
        assert getattr(L, name) is not None, name
        assert name in T.engine.ABI_SYMBOLS, name
    assert L.tri_abi_version() == 9


def test_the_header_declares_them_and_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "trinity_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b(?:int|void)\s+%s\s*\(" % name, text), name
    block = text[text.index("---- the percolator") : text.index("void tri_perc_result_destroy(tri_perc_result *);")]
    assert "percolator.cpp:5-137" in block and "percolator.h:1-3" in block and "unarynot" in block and "perc_max_bytes" in block and "perc_prune" in block
    for name in ("tri_perc_create", "tri_perc_set_enabled", "tri_perc_get_info", "tri_perc_match", "tri_perc_result_pairs"):
        assert re.search(r"^ \* %s\b" % name, block, re.M), name


def test_the_structs_match_the_binding_and_the_options_exist(T):
    E = T.engine
    assert C.sizeof(E.TriPercDocs) == 56 and E.TriPercDocs.doc_first.offset == 8 and E.TriPercDocs.npositions.offset == 40 and E.TriPercDocs.reserved.offset == 48
    assert C.sizeof(E.TriPercInfo) == 48 and C.sizeof(E.TriPercResultInfo) == 64 and E.TriPercResultInfo.pairs.offset == 24
    text = open(os.path.join(ROOT, "trinity_amd", "csrc", "trinity_hip.hip")).read()
    for name in ("perc_max_bytes", "perc_prune"):
        assert '{"%s", &tri_options::%s}' % (name, name) in text
    for name in ("status", "set_enabled", "match", "close", "create"):
        assert callable(getattr(T.Percolator, name))
    for name in ("pairs", "doc_counts", "close"):
        assert callable(getattr(E.PercolatorResult, name))


def test_null_arguments_are_refused(T):
    L = T.engine.hip_lib()
    n = C.c_size_t(77)
    buf = (C.c_uint64 * 8)()
    out = C.c_void_p(5)
    assert L.tri_perc_create(None, buf, 1, buf, 1, 4, C.byref(out)) == INVALID and b"tri_perc_create: null argument" in L.tri_last_error()
    assert L.tri_perc_match(None, None, C.byref(out)) == INVALID and b"tri_perc_match: null argument" in L.tri_last_error()
    assert out.value == 5
    assert L.tri_perc_query_status(None, buf) == INVALID and b"tri_perc_query_status" in L.tri_last_error()
    assert L.tri_perc_set_enabled(None, buf, 1, 0) == INVALID and b"tri_perc_set_enabled" in L.tri_last_error()
    assert L.tri_perc_get_info(None, None) == INVALID and b"tri_perc_get_info" in L.tri_last_error()
    assert L.tri_perc_result_pairs(None, 0, buf, buf, 4, C.byref(n)) == INVALID and b"tri_perc_result_pairs" in L.tri_last_error()
    assert L.tri_perc_result_doc_counts(None, buf) == INVALID and b"tri_perc_result_doc_counts" in L.tri_last_error()
    assert L.tri_perc_result_get_info(None, None) == INVALID and b"tri_perc_result_get_info" in L.tri_last_error()
    L.tri_perc_destroy(None)
    L.tri_perc_result_destroy(None)
    assert n.value == 77 and not any(buf)


def lower(T, programs, nterms):
    flat, q = T.engine.flatten(programs)
    status, info, err = np.full(max(1, len(programs)), 99, dtype=np.int32), np.zeros(6, dtype=np.uint64), C.create_string_buffer(512)
    rc = T.engine.host_lib().tri_host_perc_lower(flat.ctypes.data, flat.size, q.ctypes.data, len(programs), nterms, status.ctypes.data, info.ctypes.data, err, 512)
    return rc, status[: len(programs)].tolist(), [int(x) for x in info], err.value.decode()


def test_a_malformed_program_fails_the_call_an_oversize_one_does_not(T):
    tk = lambda *a: [T.tok(T.OP_TERM, t) for t in a]
    good = tk(1, 2) + [T.tok(T.OP_AND, 2)]
    wide = tk(*range(1023)) + [T.tok(T.OP_OR, 1023)]  # 1024 nodes: runs
    over = tk(*range(1024)) + [T.tok(T.OP_OR, 1024)]  # 1025 nodes
    deep = tk(0)
    for k in range(65):  # OR(k, AND(..)) nested 65 deep: the innermost leaf sits under 65 open accumulators
        deep = tk(k % 7) + deep + [T.tok(T.OP_AND if k % 2 else T.OP_OR, 2)]
    deep64 = tk(0)
    for k in range(64):
        deep64 = tk(k % 7) + deep64 + [T.tok(T.OP_AND if k % 2 else T.OP_OR, 2)]
    rc, status, info, err = lower(T, [good, wide, over, deep, deep64, [], tk(3) + [T.tok(T.OP_NOT, 1)]], 2000)
    assert rc == 0 and status == [0, 0, UNSUPPORTED, UNSUPPORTED, 0, 0, 0], (rc, status, err)
    assert info[0] == 2 and info[4] == 64 and info[5] == 1 and "query 3" in err
    # the same phrase in many queries is one leaf; a one-word phrase is its word
    ph = tk(5, 6, 7) + [T.tok(T.OP_PHRASE, 3)]
    rc, status, info, _ = lower(T, [ph] * 100 + [tk(5) + [T.tok(T.OP_PHRASE, 1)]], 10)
    assert rc == 0 and info[1] == 3 and info[2] == 1
    bad = {
        "operands": tk(1) + [T.tok(T.OP_AND, 2)],
        "leaves 2 values": tk(1, 2),
        "term 9": tk(9),
        "at least 3 of 2": tk(1, 2) + [T.tok(T.OP_SOME, (3 << 16) | 2)],
        "at least 0 of 2": tk(1, 2) + [T.tok(T.OP_SOME, 2)],
        "operator 5 with 3": tk(1, 2, 3) + [T.tok(T.OP_OPT, 3)],
        "operator 4 with 3": tk(1, 2, 3) + [T.tok(T.OP_NOT, 3)],
        "operator 7": tk(1, 2) + [T.tok(7, 2)],
        "TERM tokens": tk(1) + good + [T.tok(T.OP_PHRASE, 2)],
        "a phrase of 17": tk(*([1] * 17)) + [T.tok(T.OP_PHRASE, 17)],
    }
    for what, p in bad.items():
        rc, _, _, err = lower(T, [good, p], 8)
        assert rc == INVALID and what in err and "query 1" in err, (what, rc, err)
    flat, q = T.engine.flatten([good])
    q[0, 1] = 9  # a query that reaches past the program
    err = C.create_string_buffer(512)
    assert T.engine.host_lib().tri_host_perc_lower(flat.ctypes.data, flat.size, q.ctypes.data, 1, 8, None, None, err, 512) == INVALID and b"past prog_len" in err.value


def check(T, doc_first, terms, freqs, positions, nterms=10, reserved=0, ndocs=None, npositions=None):
    d, keep = T.engine.perc_docs(doc_first, terms, freqs, positions, reserved)
    if ndocs is not None:
        d.ndocs = ndocs
    if npositions is not None:
        d.npositions = npositions
    err = C.create_string_buffer(512)
    return T.engine.host_lib().tri_host_perc_check_docs(C.byref(d), nterms, err, 512), err.value.decode()


def test_every_refusal_of_a_batch_names_what_is_wrong(T):
    ok = ([0, 2, 2, 4], [1, 3, 2, 0xFFFFFFFF], [2, 0, 1, 1], [4, 9, 7, 7])
    assert check(T, *ok) == (0, "")
    assert check(T, [0, 3, 4], [1, 0xFFFFFFFF, 0xFFFFFFFF, 2], [0, 0, 0, 0], []) == (0, "")  # the unknown terms stand last and may repeat
    assert check(T, [1, 2], [9, 3], [1, 1], [5, 6]) == (0, "")  # a slice: positions run beside freqs from their first entry
    for args, kw, what in [
        (ok, {"ndocs": 0}, "0 documents"),
        (ok, {"ndocs": 65537}, "65537 documents"),
        (ok, {"reserved": 1}, "reserved is not 0"),
        (([0, 2, 1, 4],) + ok[1:], {}, "doc_first does not ascend at document 1"),
        ((ok[0], [3, 1, 2, 5]) + ok[2:], {}, "document 0: term 1 after term 3"),
        ((ok[0], [3, 3, 2, 5]) + ok[2:], {}, "document 0: term 3 after term 3"),
        ((ok[0], [1, 3, 0xFFFFFFFF, 2]) + ok[2:], {}, "document 2: term 2 after term 4294967295"),
        ((ok[0], [1, 3, 2, 10]) + ok[2:], {}, "document 2: term 10 of a dictionary of 10"),
        (ok, {"npositions": 3}, "document 2, term 4294967295: 1 positions run past npositions = 3"),
        (ok[:3] + ([9, 4, 7, 7],), {}, "document 0, term 1: position 4 after 9"),
    ]:
        rc, err = check(T, *args, **kw)
        assert rc == INVALID and what in err and err.startswith("tri_perc_match: "), (what, rc, err)
