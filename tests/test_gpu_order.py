"""GPU tests of ordering by a column (run with -m gpu on an MI355X): tri_batch_set_order / tri_batch_ordered — per query the first topk documents of its docID set by
(column value, docID), selected on the device by csrc/k_order.hpp at the end of every run.

The reference is tests/order_cases.py::first_k (numpy.lexsort) over structured.Corpus.evaluate's docID sets — for the reference's own records, over the oracle's sets,
which tests/golden pins to the genuine reference by count and hash — never the engine's own docsets.  tests/test_order_cases.py shows on the CPU that these expected
rows tell a right answer from a column read one docID off, from descending ties broken by the higher docID, from signed compares, from the unmasked set and from an
unmerged first task.  Every comparison is integer equality.

One device handle for the file; every index, column, batch and filter is closed by the test or fixture that made it; nothing sleeps, retries or loops over a timing."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import facet_cases as F
import oracle_lib as O
import order_cases as OC
import structured as S
from test_gpu_parity import GOLDEN, World, options
from test_gpu_structured import OVERRIDDEN, SWorld, T, corpora, dev, worlds  # noqa: F401  (T, dev, corpora, worlds: fixtures)

pytestmark = pytest.mark.gpu
EMPTY = np.zeros(0, np.uint32)
TRI_ERR_INVALID = -1


class Cols:
    """The named columns of order_cases over one uploaded index, each created on first use."""

    def __init__(self, T, ix, D):
        self.T, self.ix, self.D, self.values, self.made = T, ix, D, OC.columns(D), {}

    def get(self, name):
        if name not in self.made:
            self.made[name] = self.T.Column(self.ix, self.values[name])
        return self.made[name]

    def close(self):
        for c in self.made.values():
            c.close()
        self.made = {}


@pytest.fixture(scope="module")
def cols(T, worlds):
    made = {}

    def get(name, codec):
        if (name, codec) not in made:
            w = worlds(name, codec)
            made[name, codec] = Cols(T, w.ix, w.c.D)
        return made[name, codec]

    yield get
    for c in made.values():  # (before the worlds fixture closes the indexes: a column is destroyed before its index)
        c.close()


def select(b, cl, name, k, descending):
    """Set the order, run, sync: (docids, values, counts)."""
    b.set_order(cl.get(name), k, descending)
    b.run()
    b.sync()
    return b.ordered()


def check(got, cl, name, k, descending, sets, tag):
    want = OC.rows(sets, cl.values[name], k, descending)
    for g, w, what in zip(got, want, ("docids", "values", "counts")):
        assert g.shape == w.shape and g.dtype == np.uint32, (tag, name, k, descending, what)
        bad = np.flatnonzero((g != w).reshape(len(sets), -1).any(axis=1))
        assert not bad.size, (tag, name, k, descending, what, bad[:5].tolist(), g[bad[0]].tolist()[:12], w[bad[0]].tolist()[:12])


def check_all(b, cl, names, ks, sets, tag):
    for name in names:
        for k in ks:
            for desc in (False, True):
                check(select(b, cl, name, k, desc), cl, name, k, desc, sets, tag)


# ------------------------------------------------------------------------------------------ the stream corpus: every matching kernel, both result forms
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("opt", range(len(S.DOCS_OPTION_SETS)))
def test_stream_corpus_under_every_docs_option_set(T, dev, worlds, cols, codec, opt):
    """stream_docs_queries (documents on every window boundary) under each DocumentsOnly option set — the sets come from k_and, k_and_dense, k_psets and k_probe, as docIDs
    and as bitmaps — ordered by mod7 (seven values: ties everywhere), hash and rev, K = 10, both directions."""
    w, cl = worlds("stream", codec), cols("stream", codec)
    queries = S.stream_docs_queries(w.c)
    progs, sets, _ = w.want("docs", queries)
    opts = S.DOCS_OPTION_SETS[opt][0]
    with options(dev, **opts):
        b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        check_all(b, cl, OC.STREAM_COLUMNS, [OC.STREAM_K], sets, (codec, opts))
        assert b.counts().tolist() == [len(s) for s in sets]
        forms = {b.docset_form(i) for i in range(len(progs))}
        if not OVERRIDDEN and not opts:
            assert forms == {0, 1}, forms  # (both result forms in one batch)
        if "result_bitmaps" in opts:
            assert forms == {0}
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ K edges
def test_k_edges_on_the_main_corpus(T, dev, worlds, cols):
    """K = 1, 32, 128 and 256 over: an empty result, docID 1, docID D, lists of K - 1, K and K + 1 documents (31 / 32 / 33, 127 / 128 / 129), and RESULT_BITMAP queries
    whose last window is the 37 documents past 4 SPAN_BITS."""
    w, cl = worlds("main", 1), cols("main", 1)
    queries = [(w.c.q(t), 1) for t in OC.EDGE_QUERIES]
    progs, sets, _ = w.want("order_edges", queries)
    assert [len(s) for s in sets[:9]] == [0, 1, 1, 31, 32, 33, 127, 128, 129] and sets[1].tolist() == [1] and sets[2].tolist() == [w.c.D]
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        check_all(b, cl, ["hash", "mod7"], OC.EDGE_KS, sets, "edges")
        d, v, c = select(b, cl, "hash", 32, False)
        assert c.tolist()[:9] == [0, 1, 1, 31, 32, 32, 32, 32, 32] and not d[0].any() and not v[0].any() and d[1, 0] == 1 and d[2, 0] == w.c.D
        if not OVERRIDDEN:
            assert b.docset_form(9) == 1 and b.docset_form(10) == 1 and b.docset_form(4) == 0, [b.docset_form(i) for i in range(len(progs))]
    finally:
        b.close()


def test_single_task_segments_on_both_sides_of_every_size_the_kernel_names(T, dev):
    """Lists of one below, at and one above ORDER_TILE, a wave's pass, ORDER_PRUNE_AT, ORDER_BUF, ORDER_MAX_TOPK, a workgroup's pass and two of them: each one candidate
    tile, one task.  K = 256, 255 and 10; by hash, by rev ascending (every document beats the threshold) and by one (every value ties)."""
    c = OC.sizes_corpus()
    ix = c.upload(T, dev, 1)
    cl = Cols(T, ix, c.D)
    texts = [c.q("{n%d}" % n) for n in OC.SIZE_EDGES]
    progs = [O.parse_query(t) for t in texts]
    sets = [c.evaluate(p) for p in progs]
    assert [len(s) for s in sets] == OC.SIZE_EDGES
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        check_all(b, cl, ["hash", "rev", "one"], [256, 255, 10], sets, "sizes")
    finally:
        b.close()
        cl.close()
        ix.close()


# ------------------------------------------------------------------------------------------ worst cases for the selection
def test_worst_cases_for_the_selection(T, dev, worlds, cols):
    """`one`: every key ties, the list is the lowest K docIDs in both directions; `rev` ascending: the best come last; `huge`: 0xffffffff on every third document."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    progs, sets, _ = w.want("docs", S.stream_docs_queries(w.c))
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        check_all(b, cl, OC.WORST_COLUMNS, [256, 10], sets, "worst")
        up, down = select(b, cl, "one", 256, False), select(b, cl, "one", 256, True)
        assert all(np.array_equal(x, y) for x, y in zip(up, down))
        for i, s in enumerate(sets):
            assert np.array_equal(up[0][i, : up[2][i]], s[:256]), i
        d, v, c = select(b, cl, "huge", 10, True)
        assert all(int(v[i, 0]) == OC.HUGE and int(d[i, 0]) % 3 == 0 for i, s in enumerate(sets) if (s % 3 == 0).any())
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ many tasks per query: the merge
@pytest.mark.parametrize("task_cost", [None, 4096])
def test_a_set_that_spans_many_tasks(T, dev, worlds, cols, task_cost):
    """The tall corpus (D = 2^21 + 2^17 + 5): sets of a million documents, cut into many tasks (cand_task_cost = 4096: many more — past ORDER_FANIN: a second round of the
    merge), K = 256 and 10."""
    w, cl = worlds("tall", 1), cols("tall", 1)
    queries = [(w.c.q(t), 1) for t in OC.TALL_QUERIES]
    progs, sets, _ = w.want("facet_tall", queries)
    assert max(len(s) for s in sets) > (1 << 20)
    with options(dev, **({} if task_cost is None else {"cand_task_cost": task_cost})):
        b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        launches = b.info()["launches"]
        check_all(b, cl, OC.TALL_COLUMNS, [256], sets, task_cost)
        check(select(b, cl, "hash", 10, True), cl, "hash", 10, True, sets, task_cost)
        rounds = b.info()["launches"] - launches - 1  # (k_order, then a k_order_merge per round)
        if task_cost is not None and not OVERRIDDEN:
            assert rounds >= 2, rounds  # (some query has more tasks than one merge group folds: its lists take a second round)
        assert rounds >= 1
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ the reference's answers
def test_the_references_docsets(T, dev):
    """The DocumentsOnly records of tests/golden/ref_small.json: the oracle's sets are pinned to the genuine reference by count and hash, the rows equal first_k over them."""
    small = json.load(open(os.path.join(GOLDEN, "ref_small.json")))
    c = small["corpus"]
    recs = [r for r in small["results"] if r["cmd"] in ("query", "querysome") and r["flags"] == 1]
    w = World(T, dev, c["D"], c["V"], c["slots"], c["seed"])
    cl = Cols(T, w.ix, c["D"])
    try:
        progs = [O.parse_query(r["q"], some_min=r["min"] or 1) for r in recs]
        sets = [w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs]
        for r, s in zip(recs, sets):
            assert len(s) == r["n"] and str(O.fnv1a_docs(s)) == r["fnv"], r["q"]
        b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
        try:
            check_all(b, cl, ["hash", "huge"], [10], sets, "ref_small")
        finally:
            b.close()
        assert len(recs) >= 300
    finally:
        cl.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ masks and filters
def test_masked_documents_and_filters_are_not_listed(T, dev, worlds, cols):
    """set_masked, then three filters of both polarities in one batch: the rows are first_k of the expected masked / filtered sets."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    queries = S.stream_docs_queries(w.c)
    progs, full, _ = w.want("docs", queries)
    masked = F.stream_masked(w.c.D)
    drops = F.stream_filter_drops(w.c.D)
    filters = []
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        w.ix.set_masked(masked)
        msets = [s[~np.isin(s, masked)] for s in full]
        check_all(b, cl, ["rev", "hash"], [10], msets, "mask")
        w.ix.set_masked(EMPTY)
        filters = [T.Filter(w.ix, ids, keep=keep) for ids, keep in F.stream_filters(w.c.D)]
        b.set_filters(filters, [i % 3 for i in range(len(progs))])
        fsets = [s[~np.isin(s, drops[i % 3])] for i, s in enumerate(full)]
        check_all(b, cl, ["rev", "hash"], [10], fsets, "filters")
        b.set_filters([])
        check_all(b, cl, ["rev"], [10], full, "neither")
    finally:
        w.ix.set_masked(EMPTY)
        b.close()
        for f in filters:
            f.close()


# ------------------------------------------------------------------------------------------ the default mode; an order, facets and a ranker together
def test_default_mode_with_a_left_out_query_and_facets_and_a_ranker_beside_the_order(T, dev):
    """A TRI_FLAG_MATCHED_TERMS batch; one of its queries reports 17 terms and is left out (rich_max_terms is 16): count 0, a zero row.  Then an order, facets and a ranker
    on the one batch: each yields what it yields alone."""
    w = World(T, dev, 20000, 2000, 10, 42)
    cl = Cols(T, w.ix, 20000)
    texts = ["t0 t1", "t2 OR t3 OR t5", " OR ".join(f"t{i}" for i in range(20, 37)), '"t0 t1"', "t1 (t2 OR t3) NOT t4", "t1999 t1998"]
    progs = [O.parse_query(t) for t in texts]
    try:
        with options(dev, rich_max_terms=16):
            b = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS, allow_unsupported=True)
        try:
            status = b.query_status()
            assert status.tolist() == [0, 0, -3, 0, 0, 0]
            sets = [w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] if st == 0 else EMPTY for p, st in zip(progs, status)]
            alone = {}
            for desc in (False, True):
                alone[desc] = select(b, cl, "hash", 10, desc)
                check(alone[desc], cl, "hash", 10, desc, sets, "default mode")
            assert alone[False][2][2] == 0 and not alone[False][0][2].any() and alone[False][2][0] > 0
            b.clear_order()
            b.set_facets([(cl.get("mod7"), 7)])
            b.run()
            b.sync()
            facets_alone = b.facets(0)
            b.set_facets([])
            b.set_ranker(5)
            b.run()
            b.sync()
            ranked_alone = b.ranked()
            b.set_facets([(cl.get("mod7"), 7)])
            got = select(b, cl, "hash", 10, True)
            assert all(np.array_equal(x, y) for x, y in zip(got, alone[True]))
            assert np.array_equal(b.facets(0), facets_alone) and np.array_equal(facets_alone, F.facet_rows(sets, cl.values["mod7"], 7))
            assert all(np.array_equal(x, y) for x, y in zip(b.ranked(), ranked_alone))
        finally:
            b.close()
    finally:
        cl.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ lifecycle and launches
def test_lifecycle_and_launches(T, dev, corpora):
    """The same batch run twice: the same rows; the order replaced between runs (another column, K and direction); a run queued behind a replacement keeps the spec it was
    launched with... and the next run takes the new one; removed: info().launches back at what it was, the read call refuses; set again."""
    c = corpora("stream")
    ix = c.upload(T, dev, 1)
    cl = Cols(T, ix, c.D)
    progs = S.programs(S.stream_docs_queries(c))
    sets = [c.evaluate(p) for p in progs]
    plain = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        plain.run()
        plain.sync()
        launches = b.info()["launches"]
        assert launches == plain.info()["launches"]
        a = select(b, cl, "hash", 10, False)
        check(a, cl, "hash", 10, False, sets, "first run")
        assert b.info()["launches"] == launches + 2  # (k_order and one round of k_order_merge: no query of these has more than ORDER_FANIN tasks)
        b.run()
        b.sync()
        assert all(np.array_equal(x, y) for x, y in zip(a, b.ordered()))
        assert dev.get_option("order_last_us") > 0
        b.set_order(cl.get("rev"), 256, True)  # replaced: the rows of the last run are gone with their block
        with pytest.raises(T.TrinityError, match="tri_batch_sync first"):
            b.ordered()
        b.run()
        b.sync()
        check(b.ordered(), cl, "rev", 256, True, sets, "replaced")
        assert b.info()["launches"] == launches + 2
        b.run()  # a run queued ...
        b.set_order(cl.get("mod7"), 7, False)  # ... and a replacement behind it: the setter waits for the run, which selected by `rev`
        b.sync()
        with pytest.raises(T.TrinityError, match="tri_batch_sync first"):
            b.ordered()
        b.run()
        b.sync()
        check(b.ordered(), cl, "mod7", 7, False, sets, "behind a replacement")
        b.clear_order()
        assert b.info()["launches"] == launches
        b.run()
        b.sync()
        with pytest.raises(T.TrinityError, match="no order is set"):
            b.ordered()
        assert b.info()["launches"] == launches == plain.info()["launches"]
        assert b.counts().tolist() == [len(s) for s in sets] and np.array_equal(b.docset_hashes(), plain.docset_hashes())
        check(select(b, cl, "hash", 10, True), cl, "hash", 10, True, sets, "set again")
    finally:
        b.close()  # the batch first ...
        plain.close()
        cl.close()  # ... then its columns ...
        ix.close()  # ... then their index


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(T, dev, corpora):
    """Every refusal of the header: TRI_ERR_INVALID, a message, nothing changed."""
    from trinity_amd.engine import TriOrder, hip_lib

    L = hip_lib()
    c = corpora("stream")
    ix, other = c.upload(T, dev, 1), c.upload(T, dev, 2)
    cl, cl_other = Cols(T, ix, c.D), Cols(T, other, c.D)
    progs = S.programs(S.stream_docs_queries(c))[:6]
    sets = [c.evaluate(p) for p in progs]
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    scored = T.Batch(ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=10)

    def refused(rc, *words):
        msg = L.tri_last_error().decode()
        assert rc == TRI_ERR_INVALID and all(x in msg for x in words), (rc, msg, words)

    def set_raw(batch, col, topk, desc=0, res=0):
        spec = TriOrder(col, topk, desc, res)
        return L.tri_batch_set_order(batch.h if batch is not None else None, C.byref(spec))

    try:
        col = cl.get("hash").h
        before = select(b, cl, "hash", 10, False)
        refused(set_raw(None, col, 10), "tri_batch_set_order", "null")
        refused(set_raw(b, None, 10), "tri_batch_set_order", "null")
        refused(set_raw(b, cl_other.get("hash").h, 10), "another index")
        refused(set_raw(b, col, 0), "topk 0")
        refused(set_raw(b, col, T.ORDER_MAX_TOPK + 1), "topk 257")
        refused(set_raw(b, col, 10, 0, 1), "reserved")
        refused(set_raw(scored, col, 10), "TRI_FLAG_ACCUMULATED_SCORE", "keep no docID sets")
        assert all(np.array_equal(x, y) for x, y in zip(b.ordered(), before))  # nothing changed: the rows of the last run still stand
        d, v, n = (np.zeros((len(progs), 10), dtype=np.uint32), np.zeros((len(progs), 10), dtype=np.uint32), np.zeros(len(progs), dtype=np.uint32))
        for args in ((None, v.ctypes.data, n.ctypes.data), (d.ctypes.data, None, n.ctypes.data), (d.ctypes.data, v.ctypes.data, None)):
            refused(L.tri_batch_ordered(b.h, *args), "tri_batch_ordered", "null")
        refused(L.tri_batch_ordered(None, d.ctypes.data, v.ctypes.data, n.ctypes.data), "tri_batch_ordered", "null")
        b.run()
        refused(L.tri_batch_ordered(b.h, d.ctypes.data, v.ctypes.data, n.ctypes.data), "tri_batch_sync first")
        assert not d.any() and not v.any() and not n.any()
        b.sync()
        assert L.tri_batch_ordered(b.h, d.ctypes.data, v.ctypes.data, n.ctypes.data) == 0
        check((d, v, n), cl, "hash", 10, False, sets, "after the refusals")
        fresh = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
        try:
            fresh.run()
            fresh.sync()
            refused(L.tri_batch_ordered(fresh.h, d.ctypes.data, v.ctypes.data, n.ctypes.data), "no order is set")
        finally:
            fresh.close()
    finally:
        scored.close()
        b.close()
        cl.close()
        cl_other.close()
        ix.close()
        other.close()
