"""The percolator on the device (tri_perc_create / tri_perc_match, trinity_amd/csrc/k_perc.hpp) against the plain-Python contract of tests/perc_cases.py, which
tests/test_perc_cases.py pins to the reference's answers.  Every comparison is exact: (query, document) pairs in both orders, per-document counts."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import perc_cases as PC
from perc_limit_cases import check, cut  # (one call against the restatement, both orders exact: shared with tests/test_gpu_perc_limits.py)
from random_programs import random_program

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


@pytest.fixture(scope="module")
def dev(T):
    from conftest import apply_test_options

    d = apply_test_options(T.Device(0))
    yield d
    d.close()


@pytest.fixture(scope="module")
def fixtures():
    """The 549 programs the reference compiled and answered (165 + 384), over one corpus: (corpus parameters, programs, records)."""
    progs, recs, corpus = [], [], None
    for name in ("ref_trees.json", "ref_random.json"):
        g = json.load(open(os.path.join(GOLDEN, name)))
        assert corpus in (None, g["corpus"])
        corpus = g["corpus"]
        recs += g["results"]
        progs += [O.program_from_exec_tree(r["tree"]) for r in g["results"]]
    return corpus, progs, recs


@pytest.fixture(scope="module")
def wide_corpus(fixtures):
    """The fixtures' corpus parameters at 4097 documents (two tiles of a wave and a word more), as a batch and as the restatement's documents — made once."""
    c = fixtures[0]
    ix = O.Index.generate(4097, c["V"], c["slots"], c["seed"])
    arrays = PC.corpus_batch(ix.corpus, 4097)
    return c["V"], arrays, PC.docs_of(*arrays)


def negations(T):
    tk = PC.tk
    return [tk(3) + [T.tok(T.OP_NOT, 1)], tk(1, 2) + [T.tok(T.OP_OR, 2), T.tok(T.OP_NOT, 1)], tk(0) + [T.tok(T.OP_NOT, 1)] + tk(5) + [T.tok(T.OP_NOT, 2)],
            tk(4) + tk(0) + [T.tok(T.OP_NOT, 1), T.tok(T.OP_AND, 2)], tk(0, 1) + [T.tok(T.OP_NOT, 1), T.tok(T.OP_SOME, (1 << 16) | 2)]]  # fmt: skip


def test_the_reference_s_answers(T, dev, fixtures):
    """The 549 fixture programs as ONE stored set, the corpus's 2000 documents as one call (a partly filled last tile): per query the documents hash to the
    reference's own number."""
    c, progs, recs = fixtures
    ix = O.Index.generate(c["D"], c["V"], c["slots"], c["seed"])
    arrays = PC.corpus_batch(ix.corpus, c["D"])
    p = T.Percolator(dev, progs, c["V"])
    try:
        assert p.status().tolist() == [0] * len(progs) and p.info["queries"] == 549
        r = p.match(*arrays)
        q, d = r.pairs(T.PERC_BY_QUERY)
        assert np.all(np.diff(q.astype(np.int64)) >= 0)
        first = np.searchsorted(q, np.arange(len(progs) + 1))
        for i, rec in enumerate(recs):
            mine = d[first[i] : first[i + 1]] + 1
            assert mine.size == rec["n"] and str(O.fnv1a_docs(mine)) == rec["fnv"], rec["q"]
        q2, d2 = r.pairs(T.PERC_BY_DOCUMENT)
        key = d2.astype(np.int64) * len(progs) + q2
        assert np.all(np.diff(key) > 0) and np.array_equal(np.sort(key), np.sort(d.astype(np.int64) * len(progs) + q))
        assert np.array_equal(r.doc_counts(), np.bincount(d, minlength=c["D"]))
        assert r.info["pairs"] == q.size == sum(rec["n"] for rec in recs)
        r.close()
    finally:
        p.close()


@pytest.fixture(scope="module")
def boundary_set(T, dev, fixtures, wide_corpus):
    V = wide_corpus[0]
    progs = fixtures[1][::8] + negations(T) + [[]]
    p = T.Percolator(dev, progs, V + 8)
    yield p, progs
    p.close()


@pytest.mark.parametrize("ndocs", [1, 31, 32, 33, 2047, 2048, 2049, 4097])
def test_width_boundaries(T, boundary_set, wide_corpus, ndocs):
    """across a word, a wave's tile of 2048 documents and two tiles: negations too — no pair names a document >= ndocs"""
    p, progs = boundary_set
    info = check(T, p, progs, cut(wide_corpus[1], ndocs), wide_corpus[2][:ndocs])
    assert info["pairs"] > 0


def test_stale_scratch(T, boundary_set, wide_corpus):
    """a big call, a small one, then documents that share no term with either (terms only the dictionary's last eight ids name)"""
    p, progs = boundary_set
    V = wide_corpus[0]
    check(T, p, progs, cut(wide_corpus[1], 4097), wide_corpus[2])
    check(T, p, progs, cut(wide_corpus[1], 33), wide_corpus[2][:33])
    other = [{V + k: [k + 1], V + 7: [9]} for k in range(5)] + [{}]
    info = check(T, p, progs, PC.arrays_of(other), other)
    assert info["leaf_rows"] == 0 and info["pairs"] > 0  # (the negations hold)


def test_phrases_named_cases(T, dev):
    """tests/perc_cases.py family_phrase: adjacency, order, a repeated word, frequency 0, position 0 on either word, positions at 65534 / 65535, a posting of
    PHRASE_PASS + 1 positions (one more than a pass of k_perc_phrases takes) whose last position alone starts the phrase; the same phrase in 100 queries is one row"""
    progs, docs, nterms = PC.family_phrase()
    assert PC.PHRASE_PASS == 64 and len(docs[9][1]) == PC.PHRASE_PASS + 1
    progs = progs + [PC.phrase(1, 2)] * 100
    bits = PC.match_batch(progs, docs)
    assert bits[0] == (1 << 0) | (1 << 7) | (1 << 9) | (1 << 11) | (1 << 12) | (1 << 13) and bits[2] == 1 << 4
    p = T.Percolator(dev, progs, nterms)
    try:
        assert p.info["phrases"] == 5 and p.info["terms"] == 7
        info = check(T, p, progs, PC.arrays_of(docs), docs, bits)
        assert info["phrase_rows"] == 5 and info["leaf_rows"] == 7
        only = [docs[0], docs[4]]  # no 5 / 6 / 7: the six-word phrase has no row
        assert check(T, p, progs, PC.arrays_of(only), only)["phrase_rows"] == 4
    finally:
        p.close()


def test_phrases_from_the_corpus(T, dev, wide_corpus):
    """phrases of 2 .. 6 words drawn from tokens adjacent in the corpus's documents (they match), and the same words with two swapped"""
    V, arrays, docs = wide_corpus
    rng = np.random.default_rng(5)
    progs = []
    for d in rng.choice(300, size=40, replace=False):
        at = sorted((p, t) for t, ps in docs[d].items() for p in ps if p)
        for n in range(2, 7):
            s = int(rng.integers(0, max(1, len(at) - n)))
            run = [at[s]]
            for p, t in at[s + 1 :]:
                if p == run[-1][0] + 1 and len(run) < n:
                    run.append((p, t))
            if len(run) == n:
                words = [t for _, t in run]
                progs.append(PC.phrase(*words))
                progs.append(PC.phrase(*(words[1:2] + words[0:1] + words[2:])))
    assert len(progs) >= 100
    ndocs = 300
    bits = PC.match_batch(progs, docs[:ndocs])
    assert all(bits[0::2]) and any(b == 0 for b in bits[1::2])
    p = T.Percolator(dev, progs, V)
    try:
        check(T, p, progs, cut(arrays, ndocs), bits=bits)
    finally:
        p.close()


def test_tree_limits(T, dev):
    tk = PC.tk
    wide = tk(*range(1023)) + [T.tok(T.OP_OR, 1023)]  # 1024 nodes
    over = tk(*range(1024)) + [T.tok(T.OP_OR, 1024)]
    deep = tk(0)
    for k in range(65):
        deep = tk(k % 7) + deep + [T.tok(T.OP_AND if k % 2 else T.OP_OR, 2)]
    deep64 = tk(0)
    for k in range(64):
        deep64 = tk(k % 7) + deep64 + [T.tok(T.OP_AND if k % 2 else T.OP_OR, 2)]
    some = tk(*range(100)) + [T.tok(T.OP_SOME, (3 << 16) | 100)]
    progs = [tk(1), wide, over, tk(2), deep, deep64, [], some, tk(1022)]
    docs = [{1: [1]}, {1022: [1]}, {2: [1], 0: [2]}, {}, {5: [1], 6: [1], 90: [2]}, {k: [1] for k in range(7)}]
    p = T.Percolator(dev, progs, 1100)
    try:
        assert p.status().tolist() == [0, 0, UNSUPPORTED, 0, UNSUPPORTED, 0, 0, 0, 0] and p.info["unsupported"] == 2
        bits = PC.match_batch(progs, docs)
        bits[2] = bits[4] = 0  # left out: no matches, and the rest of the set answers
        assert bits[1] and bits[5] and bits[7] and not bits[6]
        check(T, p, progs, PC.arrays_of(docs), docs, bits)
    finally:
        p.close()


def test_the_wide_fold_at_its_limits(T, dev):
    """tests/wide_tree_cases.py's programs over terms 0 .. 59 as ONE stored set — matchsomes of 300 and 1020 children at thresholds around 255 / 256 and 510 / 511 (the
    ninth and tenth counter plane of csrc/tree_fold.hpp), a 1024-node OR, the 64-level alternation and the chain of nested matchsomes (64 stack words each) — against 130
    documents, document j holding terms 0 .. j % 61 - 1: every count 0 .. 60 occurs, and the restatement's answer is the closed form h(j) >= ceil(thr / multiplicity);
    with perc_prune at 1 and at 0."""
    import wide_tree_cases as W

    progs, docs = W.perc_programs(), W.perc_docs()
    bits = PC.match_batch(progs, docs)
    for name, b in zip(W.PERC_CASES, bits):
        assert b == sum(1 << j for j in range(len(docs)) if j % W.HMOD >= W.CLOSED[name]), name
    assert bits[W.PERC_CASES.index("some300_255")] != bits[W.PERC_CASES.index("some300_256")] == bits[W.PERC_CASES.index("some300_260")]
    arrays = PC.arrays_of(docs)
    p = T.Percolator(dev, progs, W.NLADDER)
    try:
        assert p.status().tolist() == [0] * len(progs)
        for prune in (1, 0):
            dev.set_option("perc_prune", prune)
            try:
                info = check(T, p, progs, arrays, docs, bits)
            finally:
                dev.set_option("perc_prune", 1)
            assert info["hit_queries"] == len(progs) and (prune or info["evaluated"] == len(progs))
    finally:
        p.close()


def test_many_queries_and_the_prune(T, dev):
    """70 000 stored programs over 64 documents: past 65 535 in every count a grid is sized by; perc_prune 0 and 1 give the same pairs, 1 evaluates fewer queries"""
    rng = np.random.default_rng(3)
    progs = [random_program(rng, True).tolist() for _ in range(40000)]
    pairs = rng.integers(40, 4000, size=(30000, 2))
    progs += [PC.tk(int(a), int(b)) + [T.tok(T.OP_AND, 2)] for a, b in pairs]
    docs = [{int(t): [1] for t in np.r_[rng.choice(40, size=rng.integers(0, 10), replace=False), rng.choice(np.arange(40, 4000), size=40, replace=False)]} for _ in range(64)]
    arrays = PC.arrays_of(docs)
    bits = PC.match_batch(progs, docs)
    p = T.Percolator(dev, progs, 4000)
    try:
        info1 = check(T, p, progs, arrays, bits=bits)
        dev.set_option("perc_prune", 0)
        try:
            info0 = check(T, p, progs, arrays, bits=bits)
        finally:
            dev.set_option("perc_prune", 1)
        assert info0["evaluated"] == 70000 and info1["hit_queries"] > 0 and info1["hit_queries"] <= info1["evaluated"] < info0["evaluated"]
    finally:
        p.close()


def test_enable_and_disable(T, dev):
    progs, docs, nterms = PC.family_not()
    arrays = PC.arrays_of(docs)
    bits = PC.match_batch(progs, docs)
    p = T.Percolator(dev, progs, nterms)
    try:
        check(T, p, progs, arrays, docs, bits)
        p.set_enabled([1, 3], False)
        off = list(bits)
        off[1] = off[3] = 0
        assert bits[1] and bits[3]
        check(T, p, progs, arrays, docs, off)
        with pytest.raises(T.TrinityError, match="query 5 of a set of 5"):
            p.set_enabled([0, 5], False)
        check(T, p, progs, arrays, docs, off)  # (refused whole: query 0 is still there)
        p.set_enabled([1, 3], True)
        check(T, p, progs, arrays, docs, bits)
    finally:
        p.close()


def test_documents(T, dev):
    """an empty document matches exactly the negations; terms unknown to the dictionary are ignored; a set of no queries answers no pairs"""
    progs = negations(T) + [PC.tk(1), PC.tk(1, 2) + [T.tok(T.OP_AND, 2)]]
    p = T.Percolator(dev, progs, 8)
    try:
        info = check(T, p, progs, PC.arrays_of([{}]), [{}])
        assert info["pairs"] == sum(1 for prog in progs if PC.match_one(prog, {})) >= 3 and info["leaf_rows"] == 0
        arrays = (np.array([0, 3, 5], np.uint64), np.array([1, 2, PC.NONE, PC.NONE, PC.NONE], np.uint32), np.array([1, 1, 2, 0, 1], np.uint32), np.array([4, 5, 1, 2, 3], np.uint16))
        check(T, p, progs, arrays, [{1: [4], 2: [5]}, {}])
    finally:
        p.close()
    p = T.Percolator(dev, [], 8)
    try:
        r = p.match(*PC.arrays_of([{1: [1]}, {}]))
        assert r.pairs()[0].size == 0 and r.pairs(T.PERC_BY_DOCUMENT)[1].size == 0 and r.doc_counts().tolist() == [0, 0] and r.info["evaluated"] == 0
        r.close()
    finally:
        p.close()


def test_refusals_and_lifecycle(T, dev):
    E, L = T.engine, T.engine.hip_lib()
    before = dev.memory()["pool_in_use_bytes"]
    progs, docs, nterms = PC.family_some()
    p = T.Percolator(dev, progs, nterms)
    ok = ([0, 2, 2, 4], [1, 3, 2, 5], [2, 0, 1, 1], [4, 9, 7, 7])

    def refused(args, what, code=INVALID, **kw):
        d, keep = E.perc_docs(*args, reserved=kw.get("reserved", 0))
        for k in ("ndocs", "npositions"):
            if k in kw:
                setattr(d, k, kw[k])
        out = C.c_void_p(5)
        assert L.tri_perc_match(p.h, C.byref(d), C.byref(out)) == code and what in L.tri_last_error().decode(), (what, L.tri_last_error())
        assert out.value == 5

    try:
        refused(ok, "0 documents", ndocs=0)
        refused(ok, "65537 documents", ndocs=65537)
        refused(ok, "reserved is not 0", reserved=1)
        refused(([0, 2, 1, 4],) + ok[1:], "doc_first does not ascend at document 1")
        refused((ok[0], [3, 1, 2, 5]) + ok[2:], "document 0: term 1 after term 3")
        refused((ok[0], [1, 1, 2, 5]) + ok[2:], "document 0: term 1 after term 1")
        refused((ok[0], [1, 3, 2, 8]) + ok[2:], "document 2: term 8 of a dictionary of 8")
        refused(ok, "run past npositions = 3", npositions=3)
        refused(ok[:3] + ([9, 4, 7, 7],), "document 0, term 1: position 4 after 9")
        out = C.c_void_p(5)
        assert L.tri_perc_match(p.h, None, C.byref(out)) == INVALID and out.value == 5
        r = p.match(*ok)
        n, buf = C.c_size_t(77), np.zeros(64, np.uint32)
        assert L.tri_perc_result_pairs(r.h, 2, buf.ctypes.data, buf.ctypes.data, 64, C.byref(n)) == INVALID and b"order 2" in L.tri_last_error()
        assert L.tri_perc_result_pairs(r.h, 0, buf.ctypes.data, None, 64, C.byref(n)) == INVALID
        if r.info["pairs"]:
            assert L.tri_perc_result_pairs(r.h, 0, buf.ctypes.data, buf.ctypes.data, 0, C.byref(n)) == INVALID and b"room for 0" in L.tri_last_error()
        assert n.value == 77 and not buf.any()
        r.close()
        dev.set_option("perc_max_bytes", 1024)
        try:
            refused(ok, "exceed perc_max_bytes = 1024", code=UNSUPPORTED)
        finally:
            dev.set_option("perc_max_bytes", 4 << 30)
        check(T, p, progs, PC.arrays_of(docs), docs)
    finally:
        p.close()
    assert dev.memory()["pool_in_use_bytes"] == before
