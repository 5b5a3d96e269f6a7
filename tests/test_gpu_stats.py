"""GPU tests of the stats of a column (run with -m gpu on an MI355X): tri_batch_set_stats / tri_batch_stats — per query and bucket the count, sum, min and max of a
value column over the query's docID set, aggregated on the device by csrc/k_stats.hpp at the end of every run.

The reference is tests/stats_cases.py::stats_rows (numpy) over structured.Corpus.evaluate's docID sets — for the reference's own records, over the oracle's sets, which
tests/golden pins to the genuine reference by count and hash.  tests/test_stats_cases.py shows on the CPU that these expected rows tell a right answer from a value
column read one docID off, swapped columns, a 32-bit sum, a zero-initialised min plane, clamped overflow, the unmasked set and a first task left unmerged, and which
regime of the kernel every group takes.  Every comparison is integer equality.

One device handle for the file; every index, column, batch and filter is closed by the test or fixture that made it; nothing sleeps, retries or loops over a timing."""
import json
import os

import numpy as np
import pytest

import facet_cases as F
import oracle_lib as O
import order_cases as OC
import stats_cases as X
import structured as S
from test_gpu_parity import GOLDEN, World, options
from test_gpu_structured import OVERRIDDEN, SWorld, T, corpora, dev, worlds  # noqa: F401  (T, dev, corpora, worlds: fixtures)

pytestmark = pytest.mark.gpu
EMPTY = np.zeros(0, np.uint32)
TRI_ERR_INVALID = -1


class Cols:
    """The named columns of stats_cases over one uploaded index, each created on first use."""

    def __init__(self, T, ix, D):
        self.T, self.ix, self.D, self.values, self.made = T, ix, D, X.columns(D), {}

    def get(self, name):
        if name is None:
            return None
        if name not in self.made:
            self.made[name] = self.T.Column(self.ix, self.values[name])
        return self.made[name]

    def spec(self, stats):
        return [(self.get(g), nb, self.get(v)) for g, nb, v in stats]

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


def aggregate(b, cl, stats):
    """Set the stats, run, sync: [Stats of stat k]."""
    b.set_stats(cl.spec(stats))
    b.run()
    b.sync()
    return [b.stats(k) for k in range(len(stats))]


def check(b, cl, stats, rows, sets, tag):
    counts = b.counts()
    assert counts.tolist() == [len(s) for s in sets], tag
    for (g, nb, v), got in zip(stats, rows):
        want = X.stats_rows(sets, None if g is None else cl.values[g], nb, cl.values[v])
        for plane, a, w in zip(X.Stats._fields, got, want):
            assert a.shape == w.shape and a.dtype == w.dtype, (tag, g, nb, v, plane, a.shape, a.dtype)
            bad = np.flatnonzero((a != w).any(axis=1))
            assert not bad.size, (tag, g, nb, v, plane, bad[:5].tolist(), a[bad[0]][:8].tolist(), w[bad[0]][:8].tolist())
        assert got.counts.sum(axis=1, dtype=np.uint64).tolist() == counts.tolist(), (tag, g, nb, v)
        empty = got.counts == 0
        assert not got.sums[empty].any() and (got.mins[empty] == X.HUGE).all() and not got.maxs[empty].any(), (tag, g, nb, v)


# ------------------------------------------------------------------------------------------ the stream corpus: every matching kernel, both result forms
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("opt", range(len(S.DOCS_OPTION_SETS)))
def test_stream_corpus_under_every_docs_option_set(T, dev, worlds, cols, codec, opt):
    """stream_docs_queries (documents on every window boundary) under each DocumentsOnly option set — the sets come from k_and, k_and_dense, k_psets and k_probe, as docIDs
    and as bitmaps — with one ungrouped stat (hash: sums past 2^32) and one grouped (rev by mod7 at 5 buckets: overflow) together."""
    w, cl = worlds("stream", codec), cols("stream", codec)
    queries = S.stream_docs_queries(w.c)
    progs, sets, _ = w.want("docs", queries)
    opts = S.DOCS_OPTION_SETS[opt][0]
    stats = X.resolve(X.STREAM_STATS, w.c.D)
    with options(dev, **opts):
        b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        rows = aggregate(b, cl, stats)
        check(b, cl, stats, rows, sets, (codec, opts))
        assert int(rows[0].sums.max()) >= 1 << 32
        forms = {b.docset_form(i) for i in range(len(progs))}
        if not OVERRIDDEN and not opts:
            assert forms == {0, 1}, forms  # (both result forms in one batch)
        if "result_bitmaps" in opts:
            assert forms == {0}
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ both sides of the LDS budget; four stats at once; mixed launches
def test_both_sides_of_the_lds_budget_four_stats_at_once_and_mixed_launches(T, dev, worlds, cols):
    """One grouped stat of STATS_LDS_BUCKETS - 1, + 0 and + 1 records (the last takes global atomics), low16 at 65 536 buckets; four stats at once — inside the budget
    together, and beyond it — against each of the four alone; ungrouped stats beside an on-chip and beside a direct one."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    queries = S.stream_docs_queries(w.c)
    progs, sets, _ = w.want("docs", queries)
    assert [X.lds_records([s]) - X.LDS_BUCKETS for s in X.THRESHOLD_STATS[:3]] == [-1, 0, 1] and X.THRESHOLD_STATS[3][1] == T.FACET_MAX_BUCKETS
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        for s in X.THRESHOLD_STATS:
            check(b, cl, [s], aggregate(b, cl, [s]), sets, s)
        for four in (X.FOUR_ON_CHIP, X.FOUR_DIRECT):
            together = aggregate(b, cl, four)
            check(b, cl, four, together, sets, four)
            for k, s in enumerate(four):
                alone = aggregate(b, cl, [s])[0]
                assert X.same(alone, together[k]), (four, k)
        for mixed in (X.MIXED_ON_CHIP, X.MIXED_DIRECT):
            check(b, cl, mixed, aggregate(b, cl, mixed), sets, mixed)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ the four columns as group and as value
def test_one_huge_rev_and_hash_as_group_and_as_value(T, dev, worlds, cols):
    """`one`: every match of a query lands on one record; `huge`: the overflow bucket, sums past 2^32; `rev`: min moves at every step of the walk; `hash`: no locality."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    progs, sets, _ = w.want("docs", S.stream_docs_queries(w.c))
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        for group in (X.AS_GROUPS, X.AS_VALUES):
            stats = X.resolve(group, w.c.D)
            rows = aggregate(b, cl, stats)
            check(b, cl, stats, rows, sets, group)
        huge = rows[1]  # ungrouped over `huge`: a third of a set's documents bring 0xffffffff
        assert int(huge.maxs.max()) == X.HUGE and int(huge.sums.max()) >= 1 << 32
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ many tasks per query
@pytest.mark.parametrize("task_cost", [None, 4096])
def test_a_set_that_spans_many_tasks(T, dev, worlds, cols, task_cost):
    """The tall corpus (D = 2^21 + 2^17 + 5): sets of a million documents, cut into many tasks (cand_task_cost = 4096: many more) whose workgroups all flush into ONE row."""
    w, cl = worlds("tall", 1), cols("tall", 1)
    queries = [(w.c.q(t), 1) for t in X.TALL_QUERIES]
    progs, sets, _ = w.want("facet_tall", queries)
    stats = X.resolve(X.TALL_STATS, w.c.D)
    with options(dev, **({} if task_cost is None else {"cand_task_cost": task_cost})):
        b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        rows = aggregate(b, cl, stats)
        check(b, cl, stats, rows, sets, task_cost)
        assert int(rows[0].counts.max()) > (1 << 20) and int(rows[0].sums.max()) > (1 << 50)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ edges
def test_edges(T, dev, worlds, cols):
    """Main corpus: an empty result, one match at docID 1, one at docID D, single-task segments one shorter than, exactly at and one longer than STATS_SHORT_SEGMENT, and
    RESULT_BITMAP queries whose last window is the 37 documents past 4 SPAN_BITS — with rows that fit the LDS budget, then with one that does not."""
    w, cl = worlds("main", 1), cols("main", 1)
    queries = [(w.c.q(t), 1) for t in X.EDGE_QUERIES]
    progs, sets, _ = w.want("facet_edges", queries)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        for group in (X.EDGE_STATS_ON_CHIP, X.EDGE_STATS_DIRECT):
            stats = X.resolve(group, w.c.D)
            assert (X.lds_records(stats) <= X.LDS_BUCKETS) == (group is X.EDGE_STATS_ON_CHIP)
            rows = aggregate(b, cl, stats)
            check(b, cl, stats, rows, sets, ("edges", group))
            u = rows[0]  # the ungrouped stat: the empty result, docID 1, docID D
            assert (u.counts[0, 0], u.sums[0, 0], u.mins[0, 0], u.maxs[0, 0]) == (0, 0, X.HUGE, 0)
            for q, d in ((1, 1), (2, w.c.D)):
                h = int(cl.values["hash"][d])
                assert (u.counts[q, 0], u.sums[q, 0], u.mins[q, 0], u.maxs[q, 0]) == (1, h, h, h)
        if not OVERRIDDEN:
            assert b.docset_form(6) == 1 and b.docset_form(7) == 1 and b.docset_form(3) == 0, [b.docset_form(i) for i in range(len(progs))]
    finally:
        b.close()


def test_single_task_segments_around_a_wave_and_a_workgroup(T, dev):
    """The ungrouped path: lists of one below, at and one above 64 and 256 documents, each one candidate tile, one task — a partial wave, a full one, one lane of the
    next; a workgroup's first pass, and one document of its second."""
    c = OC.sizes_corpus()
    ix = c.upload(T, dev, 1)
    cl = Cols(T, ix, c.D)
    progs = [O.parse_query(c.q("{n%d}" % n)) for n in X.SIZE_QUERIES]
    sets = [c.evaluate(p) for p in progs]
    assert [len(s) for s in sets] == X.SIZE_QUERIES
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        stats = X.resolve(X.SIZE_STATS, c.D)
        check(b, cl, stats, aggregate(b, cl, stats), sets, "sizes")
    finally:
        b.close()
        cl.close()
        ix.close()


# ------------------------------------------------------------------------------------------ the reference's answers
def test_the_references_docsets(T, dev):
    """The DocumentsOnly records of tests/golden/ref_small.json and ref_masked.json: the oracle's sets are pinned to the genuine reference by count and hash, the rows
    equal stats_rows over them (ref_masked: the records' filter installed as the index's masked set)."""
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
                stats = X.resolve([(None, 0, "hash"), ("mod7", 5, "rev"), ("huge", None, "low16")], c["D"])
                b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
                try:
                    check(b, cl, stats, aggregate(b, cl, stats), sets, (key, flt))
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
def test_masked_documents_and_filters_are_not_aggregated(T, dev, worlds, cols):
    """set_masked, then three filters of both polarities in one batch: the rows equal stats_rows of the sets the batch delivers — which are the expected ones."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    queries = S.stream_docs_queries(w.c)
    progs, full, _ = w.want("docs", queries)
    stats = X.resolve(X.MASK_STATS, w.c.D)
    masked = X.stream_masked(w.c.D)
    drops = X.stream_filter_drops(w.c.D)
    filters = []
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        w.ix.set_masked(masked)
        rows = aggregate(b, cl, stats)
        msets = [s[~np.isin(s, masked)] for s in full]
        flat, offs = b.docsets()
        assert all(np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], s) for i, s in enumerate(msets))
        check(b, cl, stats, rows, msets, "mask")
        w.ix.set_masked(EMPTY)
        filters = [T.Filter(w.ix, ids, keep=keep) for ids, keep in X.stream_filters(w.c.D)]
        b.set_filters(filters, [i % 3 for i in range(len(progs))])
        rows = aggregate(b, cl, stats)
        fsets = [s[~np.isin(s, drops[i % 3])] for i, s in enumerate(full)]
        flat, offs = b.docsets()
        assert all(np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], s) for i, s in enumerate(fsets))
        check(b, cl, stats, rows, fsets, "filters")
        b.set_filters([])
        check(b, cl, stats, aggregate(b, cl, stats), full, "neither")
    finally:
        w.ix.set_masked(EMPTY)
        b.close()
        for f in filters:
            f.close()


# ------------------------------------------------------------------------------------------ the default mode; stats beside facets, an order and a ranker
def test_default_mode_with_a_left_out_query_and_facets_an_order_and_a_ranker_beside_the_stats(T, dev):
    """A TRI_FLAG_MATCHED_TERMS batch; one of its queries reports 17 terms and is left out (rich_max_terms is 16): empty records, min 0xffffffff.  The counts plane equals
    Batch.facets of the same column on the same batch; stats, facets, an order and a ranker on the one batch each yield what they yield alone."""
    w = World(T, dev, 20000, 2000, 10, 42)
    cl = Cols(T, w.ix, 20000)
    texts = ["t0 t1", "t2 OR t3 OR t5", " OR ".join(f"t{i}" for i in range(20, 37)), '"t0 t1"', "t1 (t2 OR t3) NOT t4", "t1999 t1998"]
    progs = [O.parse_query(t) for t in texts]
    stats = X.resolve([(None, 0, "hash"), ("mod7", 5, "rev"), ("huge", None, "low16"), ("low16", None, "hash")], 20000)
    try:
        with options(dev, rich_max_terms=16):
            b = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS, allow_unsupported=True)
        try:
            status = b.query_status()
            assert status.tolist() == [0, 0, -3, 0, 0, 0]
            sets = [w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] if st == 0 else EMPTY for p, st in zip(progs, status)]
            alone = aggregate(b, cl, stats)
            check(b, cl, stats, alone, sets, "default mode")
            for r in alone:
                assert not r.counts[2].any() and not r.sums[2].any() and (r.mins[2] == X.HUGE).all() and not r.maxs[2].any() and r.counts[0].any()
            b.set_stats([])
            b.set_facets([(cl.get("mod7"), 5), (cl.get("huge"), 5)])
            b.run()
            b.sync()
            facets_alone = [b.facets(0), b.facets(1)]
            b.set_facets([])
            b.set_order(cl.get("hash"), 10, True)
            b.run()
            b.sync()
            ordered_alone = b.ordered()
            b.clear_order()
            b.set_ranker(5)
            b.run()
            b.sync()
            ranked_alone = b.ranked()
            b.set_facets([(cl.get("mod7"), 5), (cl.get("huge"), 5)])
            b.set_order(cl.get("hash"), 10, True)
            together = aggregate(b, cl, stats)
            assert all(X.same(x, y) for x, y in zip(together, alone))
            assert np.array_equal(b.facets(0), facets_alone[0]) and np.array_equal(b.facets(1), facets_alone[1])
            assert np.array_equal(together[1].counts, facets_alone[0]) and np.array_equal(together[2].counts, facets_alone[1])  # the counts plane IS the facet row
            assert all(np.array_equal(x, y) for x, y in zip(b.ordered(), ordered_alone))
            assert all(np.array_equal(x, y) for x, y in zip(b.ranked(), ranked_alone))
        finally:
            b.close()
    finally:
        cl.close()
        w.ix.close()


def test_the_counts_plane_equals_the_facets_of_the_same_batch(T, dev, worlds, cols):
    """Every grouped stat's counts against tri_batch_facets of its group column and nbuckets, set on the same batch, integer for integer."""
    w, cl = worlds("stream", 1), cols("stream", 1)
    progs, sets, _ = w.want("docs", S.stream_docs_queries(w.c))
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        for group in (X.FOUR_ON_CHIP, X.FOUR_DIRECT):
            b.set_facets([(cl.get(g), nb) for g, nb, _ in group])
            rows = aggregate(b, cl, group)
            for k in range(len(group)):
                assert np.array_equal(rows[k].counts, b.facets(k)), (group, k)
        b.set_facets([])
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ lifecycle and launches
def test_lifecycle_and_launches(T, dev, corpora):
    """The same batch run twice: the same bits (initialised and aggregated again, not added up); stats replaced between runs; a run queued behind a replacement keeps
    the specs it was launched with; cleared: info().launches back at what it was, the read call refuses; set again; the columns destroyed only after their batch."""
    c = corpora("stream")
    ix = c.upload(T, dev, 1)
    cl = Cols(T, ix, c.D)
    progs = S.programs(S.stream_docs_queries(c))
    sets = [c.evaluate(p) for p in progs]
    first, second, third = X.resolve(X.STREAM_STATS, c.D), X.resolve(X.AS_GROUPS, c.D), X.resolve(X.MIXED_DIRECT, c.D)
    plain = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        plain.run()
        plain.sync()
        launches = b.info()["launches"]
        assert launches == plain.info()["launches"]
        a = aggregate(b, cl, first)
        check(b, cl, first, a, sets, "first run")
        assert b.info()["launches"] == launches + 1
        b.run()
        b.sync()
        assert all(X.same(x, b.stats(k)) for k, x in enumerate(a))
        assert dev.get_option("stats_last_us") > 0
        b.set_stats(cl.spec(second))  # replaced: the rows of the last run are gone with their block
        with pytest.raises(T.TrinityError, match="tri_batch_sync first"):
            b.stats(0)
        b.run()
        b.sync()
        check(b, cl, second, [b.stats(k) for k in range(len(second))], sets, "replaced")
        assert b.info()["launches"] == launches + 1
        b.run()  # a run queued ...
        b.set_stats(cl.spec(third))  # ... and a replacement behind it: the setter waits for the run, which aggregated into the block it was launched with
        b.sync()
        with pytest.raises(T.TrinityError, match="tri_batch_sync first"):
            b.stats(0)
        b.run()
        b.sync()
        check(b, cl, third, [b.stats(k) for k in range(len(third))], sets, "behind a replacement")
        b.set_stats([])
        assert b.info()["launches"] == launches
        b.run()
        b.sync()
        with pytest.raises(T.TrinityError, match="no stats are set"):
            b.stats(0)
        assert b.info()["launches"] == launches == plain.info()["launches"]
        assert b.counts().tolist() == [len(s) for s in sets] and np.array_equal(b.docset_hashes(), plain.docset_hashes())
        check(b, cl, first, aggregate(b, cl, first), sets, "set again")
    finally:
        b.close()  # the batch first ...
        plain.close()
        cl.close()  # ... then its columns ...
        ix.close()  # ... then their index


# ------------------------------------------------------------------------------------------ refusals; NULL outputs
def test_refusals_and_null_outputs(T, dev, corpora):
    """Every refusal of the header: TRI_ERR_INVALID, a message, nothing changed.  A NULL output is skipped; all four NULL is refused."""
    from trinity_amd.engine import TriStat, hip_lib

    L = hip_lib()
    c = corpora("stream")
    ix, other = c.upload(T, dev, 1), c.upload(T, dev, 2)
    cl, cl_other = Cols(T, ix, c.D), Cols(T, other, c.D)
    progs = S.programs(S.stream_docs_queries(c))[:6]
    sets = [c.evaluate(p) for p in progs]
    b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    scored = T.Batch(ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=10)
    good = [("mod7", 7, "hash")]

    def refused(rc, *words):
        msg = L.tri_last_error().decode()
        assert rc == TRI_ERR_INVALID and all(x in msg for x in words), (rc, msg, words)

    def set_raw(batch, specs):
        arr = (TriStat * max(1, len(specs)))()
        for i, (grp, val, nb, res) in enumerate(specs):
            arr[i].group, arr[i].value, arr[i].nbuckets, arr[i].reserved = grp, val, nb, res
        return L.tri_batch_set_stats(batch.h, arr, len(specs))

    def read_raw(batch, k, planes, cap):
        return L.tri_batch_stats(batch.h, k, *[p.ctypes.data if p is not None else None for p in planes], cap)

    try:
        grp, val = cl.get("mod7").h, cl.get("hash").h
        before = aggregate(b, cl, good)[0]
        want = X.stats_rows(sets, cl.values["mod7"], 7, cl.values["hash"])
        assert X.same(before, want)
        refused(L.tri_batch_set_stats(None, None, 0), "tri_batch_set_stats", "null argument")
        refused(L.tri_batch_set_stats(b.h, None, 1), "tri_batch_set_stats", "null argument")
        refused(set_raw(b, [(grp, None, 7, 0)]), "tri_batch_set_stats", "value column is null")
        refused(set_raw(b, [(grp, cl_other.get("hash").h, 7, 0)]), "value column belongs to another index")
        refused(set_raw(b, [(cl_other.get("mod7").h, val, 7, 0)]), "group column belongs to another index")
        refused(set_raw(b, [(grp, val, 7, 0)] * (T.STATS_MAX + 1)), "5 stats")
        refused(set_raw(b, [(grp, val, 0, 0)]), "nbuckets 0")
        refused(set_raw(b, [(grp, val, T.FACET_MAX_BUCKETS + 1, 0)]), "nbuckets 65537")
        refused(set_raw(b, [(None, val, 3, 0)]), "nbuckets 3 without a group column")
        refused(set_raw(b, [(grp, val, 7, 1)]), "reserved")
        refused(set_raw(scored, [(grp, val, 7, 0)]), "TRI_FLAG_ACCUMULATED_SCORE", "keep no docID sets to count")
        assert X.same(b.stats(0), before)  # nothing changed: the rows of the last run still stand
        planes = [np.zeros((len(progs), 8), dt) for dt in (np.uint64, np.uint32, np.uint32, np.uint32)]
        refused(L.tri_batch_stats(None, 0, *[p.ctypes.data for p in planes], 48), "tri_batch_stats", "null argument")
        refused(read_raw(b, 0, [None] * 4, 48), "tri_batch_stats", "null argument")
        refused(read_raw(b, 1, planes, 48), "stat 1 of 1")
        refused(read_raw(b, 0, planes, 47), "records")
        assert not any(p.any() for p in planes)
        # a NULL output is skipped: each plane alone, then all four
        for i in range(4):
            only = [p if j == i else None for j, p in enumerate(planes)]
            assert read_raw(b, 0, only, 48) == 0 and np.array_equal(planes[i], want[i]) and not any(p.any() for j, p in enumerate(planes) if j > i)
        b.run()
        refused(read_raw(b, 0, planes, 48), "tri_batch_sync first")
        b.sync()
        assert read_raw(b, 0, planes, 48) == 0 and X.same(planes, want)
        b.set_stats(cl.spec(good))
        refused(read_raw(b, 0, planes, 48), "tri_batch_sync first")
        fresh = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
        try:
            fresh.run()
            fresh.sync()
            refused(read_raw(fresh, 0, planes, 48), "no stats")
        finally:
            fresh.close()
    finally:
        scored.close()
        b.close()
        cl.close()
        cl_other.close()
        ix.close()
        other.close()
