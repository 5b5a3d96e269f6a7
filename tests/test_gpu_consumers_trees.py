"""GPU tests of the three docID-set consumers — facets (csrc/k_facet.hpp), order (k_order.hpp), stats (k_stats.hpp) — over TASK_TREE queries, the hidden phrase queries
the planner adds for them, multi-task phrase queries and wide records (run with -m gpu on an MI355X).  The other consumer files run conjunctions, unions and CNFs of
terms and single-task phrases only; here a batch holds hidden slots between the callers' (rows are indexed by the caller's query, a hidden task has no row and no
list), hidden queries of up to 11 tasks (after k_tree_gather the first carries the whole list's length), tree queries whose single task is the whole result in chunks
of 65 536 documents — up to 524 325 of them in one workgroup, regions filled exactly —, filters applied at a tree's root only, and records of 1024 nodes.

The reference is facet_cases.facet_rows, order_cases.rows and stats_cases.stats_rows (numpy) over structured.Corpus.evaluate's docID sets — for the default mode and the
collection over the CPU oracle's DocumentsOnly sets — never the engine's own docsets.  tests/test_consumer_tree_cases.py shows on the CPU that the planner makes of
these lists what is said here and that the expected rows tell a right answer from a hidden list counted, rows by slot, a first chunk only, a last document dropped,
a root filter missing and a segment read by capacity.  Every comparison is integer equality.

One device handle for the file; every index, column, batch and filter is closed by the test or fixture that made it; nothing sleeps, retries or loops over a timing."""
import numpy as np
import pytest

import consumer_tree_cases as CT
import facet_cases as F
import oracle_lib as O
import order_cases as OC
import stats_cases as X
import structured as S
import wide_terms_cases as WT
import wide_tree_cases as W
from test_gpu_order import Cols
from test_gpu_parity import World, options
from test_gpu_structured import OVERRIDDEN, T, corpora, dev, worlds  # noqa: F401  (T, dev, corpora, worlds: fixtures)
from test_gpu_wide_tree_limits import Catalogue

pytestmark = pytest.mark.gpu
EMPTY = np.zeros(0, np.uint32)


# ------------------------------------------------------------------------------------------ the references, computed once for both codecs
class Refs:
    def __init__(self, corpora):
        self.corpora, self._lists, self._rows = corpora, {}, {}

    def get(self, name):
        """(queries, programs, numpy docID sets) of a list of consumer_tree_cases.LISTS"""
        if name not in self._lists:
            c = self.corpora(name)
            queries = CT.LISTS[name][0](c)
            progs = S.programs(queries)
            self._lists[name] = (queries, progs, CT.evaluate_all(c, progs))
        return self._lists[name]

    def rows(self, key, sets, values, sp):
        """consumer_rows of a phase (key), computed once"""
        if key not in self._rows:
            self._rows[key] = CT.consumer_rows(sets, values, sp)
        return self._rows[key]


@pytest.fixture(scope="module")
def refs(corpora):
    return Refs(corpora)


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


# ------------------------------------------------------------------------------------------ one consumer at a time, then all three
def set_facets(b, cl, facets):
    b.set_facets([(cl.get(name), nb) for name, nb in facets])


def set_stats(b, cl, stats):
    b.set_stats([(None if g is None else cl.get(g), nb, cl.get(v)) for g, nb, v in stats])


def run(b):
    b.run()
    b.sync()


def bad_rows(got, want):
    """The queries whose rows differ, and the first one's rows."""
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    return (bad[:6].tolist(), np.asarray(got)[bad[0]].ravel()[:10].tolist(), np.asarray(want)[bad[0]].ravel()[:10].tolist()) if bad.size else None


def check_facets(got, want, facets, tag):
    for (name, nb), g, w in zip(facets, got, want):
        assert g.shape == w.shape and g.dtype == np.uint32 and bad_rows(g, w) is None, (tag, "facet", name, nb, bad_rows(g, w))


def check_order(got, want, order, tag):
    for g, w, what in zip(got, want, ("docids", "values", "counts")):
        assert g.shape == w.shape and g.dtype == np.uint32 and bad_rows(g, w) is None, (tag, "order", order, what, bad_rows(g, w))


def check_stats(got, want, stats, tag):
    for s, g, w in zip(stats, got, want):
        for plane, a, x in zip(X.Stats._fields, g, w):
            assert a.shape == x.shape and a.dtype == x.dtype and bad_rows(a, x) is None, (tag, "stat", s, plane, bad_rows(a, x))


def alone(b, cl, sp, want, tag):
    """Facets, order and stats each ALONE on the batch, group by group, against the expected rows -> what each yielded."""
    out = {}
    for key in ("facets_on_chip", "facets_direct"):
        set_facets(b, cl, sp[key])
        run(b)
        out[key] = [b.facets(k) for k in range(len(sp[key]))]
        check_facets(out[key], want[key], sp[key], tag)
    b.set_facets([])
    out["orders"] = []
    for o, w in zip(sp["orders"], want["orders"]):
        b.set_order(cl.get(o[0]), o[1], o[2])
        run(b)
        out["orders"].append(b.ordered())
        check_order(out["orders"][-1], w, o, tag)
    b.clear_order()
    for key in ("stats_on_chip", "stats_direct"):
        set_stats(b, cl, sp[key])
        run(b)
        out[key] = [b.stats(k) for k in range(len(sp[key]))]
        check_stats(out[key], want[key], sp[key], tag)
    b.set_stats([])
    return out


def together(b, cl, sp, want, tag, yielded=None, order=0):
    """All three set on the one batch: each yields the expected rows — and, bit for bit, what it yielded alone.  The consumers stay set."""
    set_facets(b, cl, sp["facets_on_chip"])
    o = sp["orders"][order]
    b.set_order(cl.get(o[0]), o[1], o[2])
    set_stats(b, cl, sp["stats_on_chip"])
    run(b)
    got = ([b.facets(k) for k in range(len(sp["facets_on_chip"]))], b.ordered(), [b.stats(k) for k in range(len(sp["stats_on_chip"]))])
    check_facets(got[0], want["facets_on_chip"], sp["facets_on_chip"], (tag, "together"))
    check_order(got[1], want["orders"][order], o, (tag, "together"))
    check_stats(got[2], want["stats_on_chip"], sp["stats_on_chip"], (tag, "together"))
    if yielded is not None:
        assert CT.same_facets(got[0], yielded["facets_on_chip"]) and CT.same_order(got[1], yielded["orders"][order]) and CT.same_stats(got[2], yielded["stats_on_chip"]), tag
    return got


def clear(b):
    b.set_facets([])
    b.clear_order()
    b.set_stats([])


def check_counts(b, sets, tag):
    assert b.counts().tolist() == [len(s) for s in sets], (tag, b.counts().tolist(), [len(s) for s in sets])


# ------------------------------------------------------------------------------------------ the phrase corpus: hidden slots between the callers'
@pytest.mark.parametrize("codec", [1, 2])
def test_phrase_corpus_hidden_queries_between_the_callers(T, dev, worlds, cols, refs, codec):
    """phrase_queries in one batch: 17 queries in 21 slots, 4 hidden queries, 7 callers in a slot other than their index — a row taken by slot, or a hidden leaf's list
    counted, shows in every query behind the first tree.  Each consumer alone, then all three together."""
    w, cl = worlds("phrase", codec), cols("phrase", codec)
    queries, progs, sets = refs.get("phrase")
    sp = CT.specs(w.c.D)
    want = refs.rows("phrase", sets, cl.values, sp)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        if not OVERRIDDEN:
            assert b.info()["tree_queries"] >= 3, b.info()["tree_queries"]
        yielded = alone(b, cl, sp, want, (codec, "phrase"))
        check_counts(b, sets, (codec, "phrase"))
        together(b, cl, sp, want, (codec, "phrase"), yielded)
        check_counts(b, sets, (codec, "phrase"))
    finally:
        b.close()


def test_launch_accounting_on_the_phrase_batch(T, dev, worlds, cols, refs):
    """An order adds exactly k_order and ONE round of k_order_merge: the hidden queries' tasks belong to no merge group and add no round.  All three consumers cleared: the
    launches of the plain batch."""
    w, cl = worlds("phrase", 1), cols("phrase", 1)
    queries, progs, sets = refs.get("phrase")
    sp = CT.specs(w.c.D)
    plain = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        run(plain)
        launches = b.info()["launches"]
        assert launches == plain.info()["launches"]
        b.set_order(cl.get("hash"), 10, False)
        run(b)
        if not OVERRIDDEN:
            assert b.info()["launches"] == launches + 2, (b.info()["launches"], launches)
        check_order(b.ordered(), OC.rows(sets, cl.values["hash"], 10, False), ("hash", 10, False), "launches")
        set_facets(b, cl, sp["facets_on_chip"])
        set_stats(b, cl, sp["stats_on_chip"])
        run(b)
        if not OVERRIDDEN:
            assert b.info()["launches"] == launches + 4, (b.info()["launches"], launches)  # (k_facet and k_stats: one launch each)
        clear(b)
        assert b.info()["launches"] == launches
        run(b)
        assert b.info()["launches"] == launches == plain.info()["launches"]
        check_counts(b, sets, "cleared")
        assert np.array_equal(b.docset_hashes(), plain.docset_hashes())
    finally:
        b.close()
        plain.close()


# ------------------------------------------------------------------------------------------ the stream corpus: multi-task hidden queries, multi-task phrases, five chunks
@pytest.mark.parametrize("codec", [1, 2])
def test_stream_corpus_plain(T, dev, worlds, cols, refs, codec):
    """stream_queries and the four new tree texts: hidden queries of 5, 2, 11, 11, 5 and 11 tasks, caller phrase queries of 2 .. 11 compacted segments, tree results in
    all five chunks.  Each consumer alone, all three together, and a second run of the same batch: identical rows."""
    w, cl = worlds("stream", codec), cols("stream", codec)
    queries, progs, sets = refs.get("stream")
    sp = CT.specs(w.c.D)
    want = refs.rows("stream", sets, cl.values, sp)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        if not OVERRIDDEN:
            assert b.info()["tree_queries"] >= 5, b.info()["tree_queries"]
        yielded = alone(b, cl, sp, want, (codec, "stream"))
        check_counts(b, sets, (codec, "stream"))
        first = together(b, cl, sp, want, (codec, "stream"), yielded, order=3)
        run(b)  # (nothing changed)
        second = ([b.facets(k) for k in range(len(sp["facets_on_chip"]))], b.ordered(), [b.stats(k) for k in range(len(sp["stats_on_chip"]))])
        assert CT.same_facets(first[0], second[0]) and CT.same_order(first[1], second[1]) and CT.same_stats(first[2], second[2])
    finally:
        b.close()


@pytest.mark.parametrize("codec", [1, 2])
def test_stream_corpus_masked(T, dev, worlds, cols, refs, codec):
    """facet_cases.stream_masked masked — the window edges, which are chunk edges, and every 11th document: the hidden leaves run against the mask."""
    w, cl = worlds("stream", codec), cols("stream", codec)
    queries, progs, full = refs.get("stream")
    sp = CT.specs(w.c.D)
    masked = F.stream_masked(w.c.D)
    msets = CT.without(full, masked)
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        w.ix.set_masked(masked)
        alone(b, cl, sp, refs.rows("stream masked", msets, cl.values, sp), (codec, "masked"))
        check_counts(b, msets, (codec, "masked"))
    finally:
        w.ix.set_masked(EMPTY)
        b.close()


@pytest.mark.parametrize("codec", [1, 2])
def test_stream_corpus_filtered_at_the_root_on_top_of_the_mask_then_neither(T, dev, worlds, cols, refs, codec):
    """On top of the mask, stream_filters with query i on filter i % 3 — tree queries, whose filter is applied at the root only (their hidden leaves ran against the mask
    alone), and plain phrase queries both receive one; then filters and mask gone: the plain rows again."""
    w, cl = worlds("stream", codec), cols("stream", codec)
    queries, progs, full = refs.get("stream")
    sp = CT.specs(w.c.D)
    masked, drops = F.stream_masked(w.c.D), F.stream_filter_drops(w.c.D)
    msets = CT.without(full, masked)
    fsets = CT.without(msets, [drops[i % 3] for i in range(len(full))])
    filters = []
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        w.ix.set_masked(masked)
        filters = [T.Filter(w.ix, ids, keep=keep) for ids, keep in F.stream_filters(w.c.D)]
        b.set_filters(filters, [i % 3 for i in range(len(progs))])
        want = refs.rows("stream filtered", fsets, cl.values, sp)
        yielded = alone(b, cl, sp, want, (codec, "filtered"))
        check_counts(b, fsets, (codec, "filtered"))
        together(b, cl, sp, want, (codec, "filtered"), yielded, order=6)
        b.set_filters([])
        w.ix.set_masked(EMPTY)
        together(b, cl, sp, refs.rows("stream", full, cl.values, sp), (codec, "neither"), order=6)
        check_counts(b, full, (codec, "neither"))
    finally:
        w.ix.set_masked(EMPTY)
        b.close()
        for f in filters:
            f.close()


# ------------------------------------------------------------------------------------------ the main corpus: 524 325 documents in one task, a region filled exactly
def test_main_corpus_nine_and_its_neighbours(T, dev, worlds, cols, refs):
    """NINE: one workgroup walks 524 325 documents of a region filled exactly.  Order by `rev` ascending — the best keys come last, every step beats the threshold —
    and by `one` at K = 256 in both directions (the lowest 256 docIDs); window as a facet and as a group (every match through one workgroup's LDS flush); hash ungrouped
    (the sum passes 2^32)."""
    w, cl = worlds("main", 1), cols("main", 1)
    queries, progs, sets = refs.get("main")
    sp = CT.specs(w.c.D, main=True)
    want = refs.rows("main", sets, cl.values, sp)
    assert len(sets[0]) == w.c.D == 524325
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        if not OVERRIDDEN:
            assert b.info()["tree_queries"] >= 1
        yielded = alone(b, cl, sp, want, "main")
        check_counts(b, sets, "main")
        together(b, cl, sp, want, "main", yielded, order=1)
        rev, up, down = yielded["orders"][1], yielded["orders"][2], yielded["orders"][3]
        assert sp["orders"][1:4] == [("rev", 256, False), ("one", 256, False), ("one", 256, True)]
        assert rev[0][0].tolist() == list(range(w.c.D, w.c.D - 256, -1))  # NINE by rev ascending: the LAST 256 documents of its task, the last one first
        assert up[0][0].tolist() == down[0][0].tolist() == list(range(1, 257))
        assert int(yielded["stats_on_chip"][0].sums[0, 0]) >= 1 << 32 and int(yielded["facets_on_chip"][0][0].max()) == S.SPAN_BITS
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ the wide catalogue
@pytest.fixture(scope="module")
def cat():
    return Catalogue()


@pytest.mark.parametrize("codec", [1, 2])
def test_wide_catalogue_plain_masked_and_filtered(T, dev, cat, codec):
    """wide_tree_cases' records of up to 1024 nodes under tree_max_nodes = 1024 — a chunk that holds its first 65 documents only, an empty chunk, a last chunk of two
    words, allP's region filled exactly — plain, with chunk_edge_mask() masked, and with the drop filter on every second query on top.  deep65 is left out (status -3):
    count 0, empty rows in all three consumers.  allP's last document, D, is the first of an order by rev ascending at K = 1."""
    ix = cat.c.upload(T, dev, codec)
    cl = Cols(T, ix, cat.c.D)
    sp = CT.specs(cat.c.D)
    flt = None
    out = cat.names.index("deep65")
    try:
        for tag, mk, filtered in (("plain", EMPTY, False), ("masked", cat.mask, False), ("masked+filter", cat.mask, True)):
            ix.set_masked(mk)
            sets = [cat.docs(n, "plain" if tag == "plain" else "both" if filtered and i % 2 == 1 else "masked") if cat.status[i] == 0 else EMPTY for i, n in enumerate(cat.names)]
            with options(dev, **W.WIDE):
                b = T.Batch(ix, cat.progs, T.FLAG_DOCUMENTS_ONLY, allow_unsupported=True)
            try:
                assert b.query_status().tolist() == cat.status and cat.status[out] == -3
                if filtered:
                    flt = T.Filter(ix, cat.drop)
                    b.set_filters([flt], [0 if i % 2 == 1 else T.engine.NO_FILTER for i in range(len(cat.progs))])
                want = CT.consumer_rows(sets, cl.values, sp)
                yielded = alone(b, cl, sp, want, (codec, tag))
                check_counts(b, sets, (codec, tag))
                got = together(b, cl, sp, want, (codec, tag), yielded, order=2)
                assert not got[0][0][out].any() and got[1][2][out] == 0 and not got[1][0][out].any() and not got[1][1][out].any()
                u = got[2][0]
                assert (u.counts[out, 0], u.sums[out, 0], u.mins[out, 0], u.maxs[out, 0]) == (0, 0, X.HUGE, 0) and not got[2][1].counts[out].any()
                if tag == "plain":
                    b.set_order(cl.get("rev"), 1, False)
                    run(b)
                    d, v, n = b.ordered()
                    allp = cat.names.index("allP")
                    assert (int(d[allp, 0]), int(v[allp, 0]), int(n[allp])) == (cat.c.D, 0, 1) and len(sets[allp]) == len(W.active_docs())
            finally:
                b.close()
    finally:
        if flt is not None:
            flt.close()
        ix.set_masked(EMPTY)
        cl.close()
        ix.close()


# ------------------------------------------------------------------------------------------ the default mode
def test_default_mode_wide_report_and_narrow_tree_queries(T, dev):
    """One TRI_FLAG_MATCHED_TERMS batch under rich_max_terms = 64: wide-report queries (or64: 64 reportable terms; straddle: 54, two phrase leaves), narrow tree queries
    with a phrase leaf, and plain queries.  The consumers' rows equal those over the oracle's DocumentsOnly sets, and the batch's matched-terms report is byte for byte
    what it is without them."""
    D = WT.WORLDS[1][0]
    w = World(T, dev, *WT.WORLDS[1])
    cl = Cols(T, w.ix, D)
    shapes = {name: (text, mn) for name, text, mn, *_ in WT.SHAPES}
    texts = [shapes["or64"], shapes["straddle"], ('t0 OR "t1 t2"', 1), ('t0 NOT ("t1 t2" t3)', 1), ("t0 t1", 1), ('"t0 t1"', 1), ("t5", 1)]
    progs = [O.parse_query(t, some_min=mn) for t, mn in texts]
    sp = CT.specs(D)
    sp["orders"] = [("hash", 10, False), ("rev", 256, True), ("one", 256, False), ("hash", 256, True)]  # (every run of this batch writes its report again: four orders)

    def report(b):
        counts = b.counts()
        return [(b.docset(q, int(counts[q])),) + tuple(b.matched_terms(q, int(counts[q]))) for q in range(len(progs))]

    try:
        with options(dev, **WT.OPTS):
            b = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS)
        try:
            assert not b.query_status().any()
            if not OVERRIDDEN:
                assert b.info()["tree_queries"] >= 3, b.info()["tree_queries"]
            run(b)
            before = report(b)
            assert len(before[0][1]) == 64 and len(before[1][1]) == 54
            sets = [w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs]
            assert all(np.array_equal(r[0], s) for r, s in zip(before, sets))
            want = CT.consumer_rows(sets, cl.values, sp)
            yielded = alone(b, cl, sp, want, "default mode")
            together(b, cl, sp, want, "default mode", yielded, order=1)
            after = report(b)
            for q, (x, y) in enumerate(zip(before, after)):
                assert all(p.dtype == r.dtype and p.tobytes() == r.tobytes() for p, r in zip(x, y)), texts[q][0]
            check_counts(b, sets, "default mode")
        finally:
            b.close()
    finally:
        cl.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ a collection
def test_collection_of_two_parts_with_tree_queries(T, dev):
    """Two segments (the older one masked where the newer one updates it), each part's batch holding tree queries with phrase leaves — its own hidden slots —: the
    collection's facets are the parts' rows summed, its order order_cases.blend_rows, its stats stats_cases.combine, over the per-part expected rows."""
    old, new = World(T, dev, 20000, 2000, 10, 42), World(T, dev, 6000, 2000, 10, 7)
    worlds2 = (old, new)
    cls = [Cols(T, x.ix, x.D) for x in worlds2]
    texts = ['t0 OR "t1 t2"', 't3 NOT "t0 t1"', WT.SHAPES[7][1], "t0 t1", '"t0 t1"', '"t0 t1" OR "t1 t2" OR "t2 t3"']
    progs = [O.parse_query(t) for t in texts]
    gone = np.arange(1, 6001, dtype=np.uint32)
    facets, stats = [("mod7", 5), ("huge", 5), ("low16", 16)], [(None, 0, "hash"), ("mod7", 5, "rev"), ("huge", 5, "low16")]
    parts, cb = [], None
    try:
        old.ix.set_masked(gone)
        old.ora.set_masked(gone)
        sets = [[x.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs] for x in worlds2]
        assert all(len(s) for s in sets[0]) and all(len(s) for s in sets[1]) and int(sets[0][0].min()) > 6000
        with options(dev, **W.WIDE):
            parts = [T.Batch(x.ix, progs, T.FLAG_DOCUMENTS_ONLY) for x in worlds2]
        if not OVERRIDDEN:
            assert all(p.info()["tree_queries"] >= 4 for p in parts), [p.info()["tree_queries"] for p in parts]
        cb = T.CollectionBatch(parts)
        for p, cl in zip(parts, cls):
            set_facets(p, cl, facets)
            set_stats(p, cl, stats)
        for name, k, desc in (("hash", 10, False), ("rev", 256, True), ("mod7", 10, False)):
            for p, cl in zip(parts, cls):
                p.set_order(cl.get(name), k, desc)
            cb.run()
            cb.sync()
            part_rows = [OC.rows(s, cl.values[name], k, desc) for s, cl in zip(sets, cls)]
            for p, r in zip(parts, part_rows):
                check_order(p.ordered(), r, (name, k, desc), "part")
            got = cb.ordered()
            for g, x, what in zip(got, OC.blend_rows(part_rows, k, desc), ("docids", "values", "counts")):
                assert g.dtype == np.uint32 and np.array_equal(g, x), (name, k, desc, what)
        assert cb.counts().tolist() == [len(a) + len(c) for a, c in zip(*sets)]
        for k, (name, nb) in enumerate(facets):
            want = sum(F.facet_rows(s, cl.values[name], nb).astype(np.uint64) for s, cl in zip(sets, cls))
            got = cb.facets(k)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (name, nb, bad_rows(got, want))
        for k, (g, nb, v) in enumerate(stats):
            want = X.combine([X.stats_rows(s, None if g is None else cl.values[g], nb, cl.values[v]) for s, cl in zip(sets, cls)])
            got = cb.stats(k)
            assert X.same(got, want), (g, nb, v, [bad_rows(a, x) for a, x in zip(got, want)])
    finally:
        if cb is not None:
            cb.close()
        for p in parts:
            p.close()
        old.ora.set_masked(EMPTY)
        old.ix.set_masked(EMPTY)
        for cl in cls:
            cl.close()
        for x in worlds2:
            x.ix.close()
