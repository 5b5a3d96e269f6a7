"""GPU tests of the facet counts (run with -m gpu on an MI355X): tri_column_create / tri_batch_set_facets / tri_batch_facets — per query a histogram of its docID set
over per-document columns, counted on the device by csrc/k_facet.hpp at the end of every run.

The reference is tests/facet_cases.py::facet_rows (numpy.bincount) over structured.Corpus.evaluate's docID sets — for the reference's own records, over the oracle's
sets, which tests/golden pins to the genuine reference by count and hash.  tests/test_facet_cases.py shows on the CPU that these expected rows tell a right answer from
a column read one docID off, from overflow clamped into the last bucket and from the unmasked, unfiltered set.  Every comparison is integer equality.

One device handle for the file; every index, column, batch and filter is closed by the test or fixture that made it; nothing sleeps, retries or loops over a timing."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import facet_cases as F
import oracle_lib as O
import structured as S
from test_gpu_parity import GOLDEN, World, options
from test_gpu_structured import OVERRIDDEN, SWorld, T, corpora, dev, worlds  # noqa: F401  (T, dev, corpora, worlds: fixtures)

pytestmark = pytest.mark.gpu
EMPTY = np.zeros(0, np.uint32)
TRI_ERR_INVALID = -1


class Cols:
    """The named columns of facet_cases over one uploaded index, each created on first use."""

    def __init__(self, T, ix, D):
        self.T, self.ix, self.D, self.values, self.made = T, ix, D, F.columns(D), {}

    def get(self, name):
        if name not in self.made:
            self.made[name] = self.T.Column(self.ix, self.values[name])
        return self.made[name]

    def spec(self, facets):
        return [(self.get(n), nb) for n, nb in facets]

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


def count(b, cl, facets):
    """Set the facets, run, sync: [rows of facet k]."""
    b.set_facets(cl.spec(facets))
    b.run()
    b.sync()
    return [b.facets(k) for k in range(len(facets))]


def check(b, cl, facets, rows, sets, tag):
    counts = b.counts()
    assert counts.tolist() == [len(s) for s in sets], tag
    for (name, nb), got in zip(facets, rows):
        want = F.facet_rows(sets, cl.values[name], nb)
        assert got.shape == want.shape and got.dtype == np.uint32, (tag, name, nb)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert not bad.size, (tag, name, nb, bad[:5].tolist(), got[bad[0]][:12].tolist(), want[bad[0]][:12].tolist())
        assert got.sum(axis=1, dtype=np.uint64).tolist() == counts.tolist(), (tag, name, nb)


# ------------------------------------------------------------------------------------------ the stream corpus: every matching kernel, both result forms
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("opt", range(len(S.DOCS_OPTION_SETS)))
def test_stream_corpus_under_every_docs_option_set(T, dev, worlds, cols, codec, opt):
    """stream_docs_queries (documents on every window boundary) under each DocumentsOnly option set — the sets come from k_and, k_and_dense, k_psets and k_probe, as docIDs
    and as bitmaps — counted by mod7 at 7 buckets (no overflow) and at 5 (overflow), and by every column at a bucket count that fits it."""
    w, cl = worlds("stream", codec), cols("stream", codec)
    queries = S.stream_docs_queries(w.c)
    progs, sets, _ = w.want("docs", queries)
    opts = S.DOCS_OPTION_SETS[opt][0]
    facets = F.resolve(F.STREAM_FACETS, w.c.D)
    with options(dev, **opts):
        b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        for group in (facets[:4], facets[4:]):
            rows = count(b, cl, group)
            check(b, cl, group, rows, sets, (codec, opts))
        flat, offs = b.docsets()
        assert all(np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], s) for i, s in enumerate(sets))
        forms = {b.docset_form(i) for i in range(len(progs))}
        if not OVERRIDDEN and not opts:
            assert forms == {0, 1}, forms  # (both result forms in one batch)
        if "result_bitmaps" in opts:
            assert forms == {0}
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ both sides of the LDS budget; four facets at once
def test_both_sides_of_the_lds_budget_and_four_facets_at_once(T, dev, worlds, cols):
    """One facet of FACET_LDS_COUNTERS - 2, - 1 and + 0 buckets (one counter below the budget, exactly on it, one above: the last takes global atomics), low16 at 65 536
    buckets; four facets at once — inside the budget together, and beyond it — against each of the four alone."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    queries = S.stream_docs_queries(w.c)
    progs, sets, _ = w.want("docs", queries)
    assert [nb + 1 - F.LDS_COUNTERS for _, nb in F.THRESHOLD_FACETS[:3]] == [-1, 0, 1] and F.THRESHOLD_FACETS[3] == ("low16", T.FACET_MAX_BUCKETS)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        for f in F.THRESHOLD_FACETS:
            check(b, cl, [f], count(b, cl, [f]), sets, f)
        for four in (F.FOUR_ON_CHIP, F.FOUR_DIRECT):
            together = count(b, cl, four)
            check(b, cl, four, together, sets, four)
            for k, f in enumerate(four):
                alone = count(b, cl, [f])[0]
                assert np.array_equal(alone, together[k]), (four, k)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ many tasks per query
@pytest.mark.parametrize("task_cost", [None, 4096])
def test_a_set_that_spans_many_tasks(T, dev, worlds, cols, task_cost):
    """The tall corpus (D = 2^21 + 2^17 + 5): sets of a million documents, cut into many tasks (cand_task_cost = 4096: many more) whose workgroups all add into ONE row —
    by `one` every match of a query meets on a single counter, by `window` each task on one or two."""
    w, cl = worlds("tall", 1), cols("tall", 1)
    queries = [(w.c.q(t), 1) for t in F.TALL_QUERIES]
    progs, sets, _ = w.want("facet_tall", queries)
    facets = F.resolve(F.TALL_FACETS, w.c.D)
    with options(dev, **({} if task_cost is None else {"cand_task_cost": task_cost})):
        b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        rows = count(b, cl, facets)
        check(b, cl, facets, rows, sets, task_cost)
        assert max(int(r.max()) for r in rows) > (1 << 20)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ edges
def test_edges(T, dev, worlds, cols):
    """Main corpus: an empty result, one match at docID 1, one at docID D, single-task segments one shorter than, exactly at and one longer than FACET_SHORT_SEGMENT, and
    RESULT_BITMAP queries whose last window is the 37 documents past 4 SPAN_BITS."""
    w, cl = worlds("main", 1), cols("main", 1)
    queries = [(w.c.q(t), 1) for t in F.EDGE_QUERIES]
    progs, sets, _ = w.want("facet_edges", queries)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        # on chip first: the four rows fit the LDS budget together, so the segment's length decides (127: direct; 128, 129: an LDS row) — then every edge direct (a 65 537-counter row)
        for group in (F.EDGE_FACETS_ON_CHIP, F.EDGE_FACETS):
            facets = F.resolve(group, w.c.D)
            assert (sum(nb + 1 for _, nb in facets) <= F.LDS_COUNTERS) == (group is F.EDGE_FACETS_ON_CHIP)
            rows = count(b, cl, facets)
            check(b, cl, facets, rows, sets, ("edges", group))
            assert not rows[0][0].any() and int(rows[0][1].sum()) == 1 and int(rows[0][2].sum()) == 1
        if not OVERRIDDEN:
            assert b.docset_form(6) == 1 and b.docset_form(7) == 1 and b.docset_form(3) == 0, [b.docset_form(i) for i in range(len(progs))]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ the reference's answers
def test_the_references_docsets(T, dev):
    """The DocumentsOnly records of tests/golden/ref_small.json and ref_masked.json: the oracle's sets are pinned to the genuine reference by count and hash, the rows
    equal facet_rows over them (ref_masked: the records' filter installed as the index's masked set)."""
    small = json.load(open(os.path.join(GOLDEN, "ref_small.json")))
    masked = json.load(open(os.path.join(GOLDEN, "ref_masked.json")))
    jobs = [(small["corpus"], None, [r for r in small["results"] if r["cmd"] in ("query", "querysome") and r["flags"] == 1])]
    for name in ("tiny", "dense"):
        for flt in masked["filters"]:
            jobs.append((masked["corpora"][name], flt, [r for r in masked["results"] if r["corpus"] == name and r["filter"] == flt and r["flags"] == 1]))
    seen = 0
    worlds_made = {}
    try:
        for c, flt, recs in jobs:
            key = (c["D"], c["V"], c["slots"], c["seed"])
            if key not in worlds_made:
                w = World(T, dev, *key)
                worlds_made[key] = (w, Cols(T, w.ix, c["D"]))
            w, cl = worlds_made[key]
            with np.errstate(over="ignore"):
                drop = O.masked_docs(c["D"], *flt) if flt else EMPTY
            w.ix.set_masked(drop)
            w.ora.set_masked(drop)
            try:
                progs = [O.parse_query(r["q"], some_min=r["min"] or 1) for r in recs]
                sets = [w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs]
                for r, s in zip(recs, sets):
                    assert len(s) == r["n"] and str(O.fnv1a_docs(s)) == r["fnv"], (flt, r["q"])
                facets = F.resolve([("mod7", 5), ("huge", None), ("low16", None)], c["D"])
                b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
                try:
                    check(b, cl, facets, count(b, cl, facets), sets, (key, flt))
                finally:
                    b.close()
                seen += len(recs)
            finally:
                w.ix.set_masked(EMPTY)
                w.ora.set_masked(EMPTY)
    finally:
        for w, cl in worlds_made.values():
            cl.close()
            w.ix.close()
    assert seen >= 300 + 6 * 85, seen


# ------------------------------------------------------------------------------------------ masks and filters
def test_masked_documents_and_filters_are_not_counted(T, dev, worlds, cols):
    """set_masked, then three filters of both polarities in one batch: the rows equal facet_rows of the sets the batch delivers — which are the expected ones — and
    every row sums to the match count."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    queries = S.stream_docs_queries(w.c)
    progs, full, _ = w.want("docs", queries)
    facets = F.resolve([("mod7", 7), ("mod7", 5), ("window", None), ("huge", None)], w.c.D)
    masked = F.stream_masked(w.c.D)
    drops = F.stream_filter_drops(w.c.D)
    filters = []
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        w.ix.set_masked(masked)
        rows = count(b, cl, facets)
        msets = [s[~np.isin(s, masked)] for s in full]
        flat, offs = b.docsets()
        assert all(np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], s) for i, s in enumerate(msets))
        check(b, cl, facets, rows, msets, "mask")
        w.ix.set_masked(EMPTY)
        filters = [T.Filter(w.ix, ids, keep=keep) for ids, keep in F.stream_filters(w.c.D)]
        b.set_filters(filters, [i % 3 for i in range(len(progs))])
        rows = count(b, cl, facets)
        fsets = [s[~np.isin(s, drops[i % 3])] for i, s in enumerate(full)]
        flat, offs = b.docsets()
        assert all(np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], s) for i, s in enumerate(fsets))
        check(b, cl, facets, rows, fsets, "filters")
        b.set_filters([])
        check(b, cl, facets, count(b, cl, facets), full, "neither")
    finally:
        w.ix.set_masked(EMPTY)
        b.close()
        for f in filters:
            f.close()


# ------------------------------------------------------------------------------------------ the default mode
def test_default_mode_and_a_query_the_planner_left_out(T, dev):
    """A TRI_FLAG_MATCHED_TERMS batch; one of its queries reports 17 terms and is left out (rich_max_terms is 16): its row is all zero."""
    w = World(T, dev, 20000, 2000, 10, 42)
    cl = Cols(T, w.ix, 20000)
    texts = ["t0 t1", "t2 OR t3 OR t5", " OR ".join(f"t{i}" for i in range(20, 37)), '"t0 t1"', "t1 (t2 OR t3) NOT t4", "t1999 t1998"]
    progs = [O.parse_query(t) for t in texts]
    facets = F.resolve([("mod7", 7), ("mod7", 5), ("huge", None), ("low16", None)], 20000)
    try:
        with options(dev, rich_max_terms=16):
            b = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS, allow_unsupported=True)
        try:
            status = b.query_status()
            assert status.tolist() == [0, 0, -3, 0, 0, 0]
            sets = [w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] if st == 0 else EMPTY for p, st in zip(progs, status)]
            rows = count(b, cl, facets)
            check(b, cl, facets, rows, sets, "default mode")
            assert all(not r[2].any() for r in rows) and all(r[0].any() for r in rows)
        finally:
            b.close()
    finally:
        cl.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ lifecycle
def test_lifecycle(T, dev, corpora):
    """The same batch run twice: the same rows (zeroed and recounted, not added up); facets replaced between runs; cleared; the batch's info().launches back at what it
    was before it ever had facets; the columns destroyed only after their batch."""
    c = corpora("stream")
    ix = c.upload(T, dev, 1)
    cl = Cols(T, ix, c.D)
    queries = S.stream_docs_queries(c)
    progs = S.programs(queries)
    sets = [c.evaluate(p) for p in progs]
    first, second = F.resolve([("mod7", 5), ("low16", None)], c.D), F.resolve([("huge", None), ("window", None), ("one", None)], c.D)
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        launches = b.info()["launches"]
        a = count(b, cl, first)
        check(b, cl, first, a, sets, "first run")
        assert b.info()["launches"] == launches + 1
        b.run()
        b.sync()
        again = [b.facets(k) for k in range(len(first))]
        assert all(np.array_equal(x, y) for x, y in zip(a, again))
        us = dev.get_option("facet_last_us")
        assert us > 0
        b.set_facets(cl.spec(second))  # replaced: the rows of the last run are gone with their block
        with pytest.raises(T.TrinityError, match="tri_batch_sync first"):
            b.facets(0)
        b.run()
        b.sync()
        check(b, cl, second, [b.facets(k) for k in range(len(second))], sets, "replaced")
        assert b.info()["launches"] == launches + 1
        b.set_facets([])
        assert b.info()["launches"] == launches
        b.run()
        b.sync()
        with pytest.raises(T.TrinityError, match="no facets are set"):
            b.facets(0)
        assert b.counts().tolist() == [len(s) for s in sets]
        check(b, cl, first, count(b, cl, first), sets, "set again")
    finally:
        b.close()  # the batch first ...
        cl.close()  # ... then its columns ...
        ix.close()  # ... then their index


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(T, dev, corpora):
    """Every refusal of the header: TRI_ERR_INVALID, a message, nothing changed."""
    from trinity_amd.engine import TriFacet, hip_lib

    L = hip_lib()
    c = corpora("stream")
    ix, other = c.upload(T, dev, 1), c.upload(T, dev, 2)
    cl, cl_other = Cols(T, ix, c.D), Cols(T, other, c.D)
    progs = S.programs(S.stream_docs_queries(c))[:6]
    sets = [c.evaluate(p) for p in progs]
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    scored = T.Batch(ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=10)
    good = [("mod7", 7)]

    def refused(rc, *words):
        msg = L.tri_last_error().decode()
        assert rc == TRI_ERR_INVALID and all(x in msg for x in words), (rc, msg, words)

    def set_raw(batch, specs):
        arr = (TriFacet * max(1, len(specs)))()
        for i, (col, nb, res) in enumerate(specs):
            arr[i].column, arr[i].nbuckets, arr[i].reserved = col, nb, res
        return L.tri_batch_set_facets(batch.h, arr, len(specs))

    try:
        vals = cl.values["mod7"]
        out = C.c_void_p()
        for n in (c.D, c.D + 2):
            v = np.zeros(n, dtype=np.uint32)
            refused(L.tri_column_create(ix.h, v.ctypes.data, n, C.byref(out)), "tri_column_create", "docs_cnt")
            assert not out.value
        # an index that holds a docID above its docs_cnt: no column of docs_cnt + 1 values covers it
        short = S.build({"a": (np.array([1, 5, 9], dtype=np.uint32), np.ones(3, dtype=np.uint32))}, docs_cnt=8)
        sx = short.upload(T, dev, 1)
        try:
            v = np.zeros(9, dtype=np.uint32)
            refused(L.tri_column_create(sx.h, v.ctypes.data, 9, C.byref(out)), "tri_column_create", "docID 9", "docs_cnt 8")
            assert not out.value
        finally:
            sx.close()
        col = cl.get("mod7").h
        before = count(b, cl, good)[0]
        refused(set_raw(b, [(None, 7, 0)]), "tri_batch_set_facets", "null")
        refused(set_raw(b, [(cl_other.get("mod7").h, 7, 0)]), "another index")
        refused(set_raw(b, [(col, 7, 0)] * (T.FACETS_MAX + 1)), "5 facets")
        refused(set_raw(b, [(col, 0, 0)]), "nbuckets 0")
        refused(set_raw(b, [(col, T.FACET_MAX_BUCKETS + 1, 0)]), "nbuckets 65537")
        refused(set_raw(b, [(col, 7, 1)]), "reserved")
        refused(set_raw(scored, [(col, 7, 0)]), "TRI_FLAG_ACCUMULATED_SCORE")
        assert np.array_equal(b.facets(0), before)  # nothing changed: the rows of the last run still stand
        buf = np.zeros((len(progs), 8), dtype=np.uint32)
        refused(L.tri_batch_facets(b.h, 1, buf.ctypes.data, buf.size), "facet 1 of 1")
        refused(L.tri_batch_facets(b.h, 0, buf.ctypes.data, buf.size - 1), "counters")
        assert not buf.any()
        b.run()
        refused(L.tri_batch_facets(b.h, 0, buf.ctypes.data, buf.size), "tri_batch_sync first")
        b.sync()
        assert L.tri_batch_facets(b.h, 0, buf.ctypes.data, buf.size) == 0 and np.array_equal(buf, F.facet_rows(sets, vals, 7))
        b.set_facets(cl.spec(good))
        refused(L.tri_batch_facets(b.h, 0, buf.ctypes.data, buf.size), "tri_batch_sync first")
        fresh = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
        try:
            fresh.run()
            fresh.sync()
            refused(L.tri_batch_facets(fresh.h, 0, buf.ctypes.data, buf.size), "no facets")
        finally:
            fresh.close()
    finally:
        scored.close()
        b.close()
        cl.close()
        cl_other.close()
        ix.close()
        other.close()


# ------------------------------------------------------------------------------------------ a batch without facets launches what it always did
def test_a_batch_without_facets_launches_nothing_new(T, dev, worlds, cols):
    w, cl = worlds("stream", 1), cols("stream", 1)
    progs, sets, _ = w.want("docs", S.stream_docs_queries(w.c))
    plain = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        plain.run()
        plain.sync()
        launches = plain.info()["launches"]
        assert b.info()["launches"] == launches
        count(b, cl, [("mod7", 7)])
        assert b.info()["launches"] == launches + 1
        b.set_facets([])
        b.run()
        b.sync()
        assert b.info()["launches"] == launches == plain.info()["launches"]
        assert b.counts().tolist() == plain.counts().tolist() and np.array_equal(b.docset_hashes(), plain.docset_hashes())
    finally:
        b.close()
        plain.close()
