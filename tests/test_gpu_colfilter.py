"""GPU tests of column predicates as document filters (run with -m gpu on an MI355X): tri_filters_from_columns / tri_filter_bitmap (csrc/k_filter_columns.hpp — one
launch evaluates every predicate of a call over the index's resident columns and writes every word of every drop bitmap).

References: the numpy contract of tests/colfilter_cases.py (tests/test_colfilter_cases.py shows that its cases tell the right answer from nine wrong ones) for the
bitmaps, bit for bit over 1 .. D, on the stream corpus (D = 2 SPAN_BITS + 37) and the tiny fixture corpus (smaller than one chunk of the kernel); for batches, the same
batch under a Filter(index, docids) made from the host evaluation — docID sets, counts and the default mode's matched terms integer for integer, scored top-K through
structured.check_topk against the oracle masked by the same documents.

One device handle for the file; every index, batch, column and filter is closed by the test that made it; nothing sleeps, retries or loops over a timing."""
import ctypes as C

import numpy as np
import pytest

import colfilter_cases as CF
import filter_cases as F
import oracle_lib as O
import structured as S
from test_gpu_filters import DOCS_PATHS, KINDS, SCORED_PATHS, Oracle, Run, check_top, stream  # noqa: F401  (stream: fixture)
from test_gpu_parity import World, options
from test_gpu_structured import OVERRIDDEN, SWorld, T, dev  # noqa: F401  (T, dev: fixtures)

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
EMPTY = np.zeros(0, np.uint32)
BITMAP_KERNEL, CANDIDATE_KERNEL = DOCS_PATHS[2], DOCS_PATHS[3]  # k_and_dense alone (no planes, every list dense enough); k_and (no planes, the planner's density threshold)
assert BITMAP_KERNEL == {"dense_min_postings": 0, "planes": 0} and CANDIDATE_KERNEL == {"planes": 0}


class Cols:
    """The eight named columns of colfilter_cases over one uploaded index (`mod7@2` a second handle over mod7's values)."""

    def __init__(self, T, ix, D):
        self.values = CF.columns(D)
        self.made = {n: T.Column(ix, v) for n, v in self.values.items()}

    def close(self):
        for c in self.made.values():
            c.close()
        self.made = {}


def predicate(T, cols, case, also=None):
    cl = [T.Clause.range(cols.made[c["col"]], c["lo"], c["hi"], c["negate"]) if c["kind"] == "range" else T.Clause.among(cols.made[c["col"]], c["set"], c["negate"]) for c in case.clauses]
    return T.Predicate(cl, any=case.any, also=also[case.also] if case.also else None)


def build(T, ix, cols, cases, also, keep, size=CF.MAX_PREDS):
    """The cases' filters (all of one mode), `size` predicates a call."""
    out = []
    for i in range(0, len(cases), size):
        out += T.Filter.from_columns(ix, [predicate(T, cols, c, also) for c in cases[i : i + size]], keep=keep)
    return out


def words(ix_D):
    return (ix_D // S.SPAN_BITS + 2) * (S.SPAN_BITS // 32)


class Setup:
    """An uploaded corpus with its columns, its two `also` filters (tri_filter_create; tri_filter_from_docset of ALSO_QUERY) and what those drop."""

    def __init__(self, T, dev, name):
        self.name = name
        if name == "stream":
            self.c = S.stream_corpus()
            self.w = SWorld(T, dev, self.c, 1)
            self.D = self.c.D
            prog = S.programs([(self.c.q(CF.ALSO_QUERY[name]), 1)])[0]
            docset = self.c.evaluate(prog)
        else:
            t = CF.TINY
            self.w = World(T, dev, t["D"], t["V"], t["slots"], t["seed"])
            self.D = t["D"]
            prog = O.parse_query(CF.ALSO_QUERY[name])
            docset = self.w.ora.exec(prog, O.FLAG_DOCUMENTS_ONLY)[0]
        self.ix = self.w.ix
        self.cols = Cols(T, self.ix, self.D)
        b = T.Batch(self.ix, [prog], T.FLAG_DOCUMENTS_ONLY)
        b.run()
        b.sync()
        assert np.array_equal(b.docset(0), docset)
        self.also = {"create": T.Filter(self.ix, CF.also_create_ids(self.D)), "docset": T.Filter.from_docset(b, 0, keep=True)}
        b.close()
        self.also_bits = {k: CF.also_bits(k, self.D, docset) for k in self.also}

    def want(self, case):
        return CF.drop_bits(case, self.cols.values, self.D, self.also_bits.get(case.also))

    def close(self):
        for f in self.also.values():
            f.close()
        self.cols.close()
        self.ix.close()


@pytest.fixture(scope="module")
def setups(T, dev):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Setup(T, dev, name)
        return made[name]

    yield get
    for s in made.values():
        s.close()


# ------------------------------------------------------------------------------------------ 1: every case's bitmap, bit for bit
@pytest.mark.parametrize("corpus", ["stream", "tiny"])
def test_bitmaps_equal_the_contract_bit_for_bit(T, setups, corpus):
    s = setups(corpus)
    cases = CF.cases(s.D)
    checked = 0
    for keep in (True, False):
        mine = [c for c in cases if c.keep == keep]
        filters = build(T, s.ix, s.cols, mine, s.also, keep)
        try:
            assert len(filters) == len(mine)
            for c, f in zip(mine, filters):
                w = f.bitmap()
                assert w.dtype == np.uint32 and w.size == words(s.D), (c, w.size)
                got, want = CF.bits_of(w, s.D), s.want(c)
                if not np.array_equal(got, want):
                    bad = np.nonzero(got != want)[0]
                    raise AssertionError((corpus, c.name, len(bad), bad[:10].tolist(), got[bad[:10]].tolist()))
                checked += 1
        finally:
            for f in filters:
                f.close()
    assert checked == len(cases) == 2 * len(CF.predicates(s.D)) >= 78  # (39 predicates on every corpus, more where the chunk's and the windows' multiples fall inside it; both modes)
    # a filter made by tri_filter_create reads back too: tri_filter_bitmap works for any filter
    assert np.array_equal(CF.bits_of(s.also["create"].bitmap(), s.D), s.also_bits["create"]) and np.array_equal(CF.bits_of(s.also["docset"].bitmap(), s.D), s.also_bits["docset"])


# ------------------------------------------------------------------------------------------ 2: however the predicates are cut into calls
def test_one_call_of_1_of_2_of_256_and_each_alone_give_identical_bitmaps(T, setups):
    s = setups("stream")
    base = [c for c in CF.cases(s.D) if c.keep]
    preds = [base[i % len(base)] for i in range(CF.MAX_PREDS)]
    assert len(base) >= 64 and {c.also for c in preds} == {None, "create", "docset"} and len({cl["col"] for c in preds for cl in c.clauses}) == CF.MAX_COLUMNS
    made = []
    try:
        full = build(T, s.ix, s.cols, preds, s.also, True, size=CF.MAX_PREDS)
        made += full
        ref = [f.bitmap() for f in full]
        one = build(T, s.ix, s.cols, preds[:1], s.also, True)
        two = build(T, s.ix, s.cols, preds[:2], s.also, True)
        made += one + two
        assert np.array_equal(one[0].bitmap(), ref[0]) and np.array_equal(two[0].bitmap(), ref[0]) and np.array_equal(two[1].bitmap(), ref[1])
        alone = build(T, s.ix, s.cols, preds, s.also, True, size=1)
        made += alone
        assert len(alone) == CF.MAX_PREDS
        for i, f in enumerate(alone):
            assert np.array_equal(f.bitmap(), ref[i]), (i, preds[i])
        for i in (0, 7, 100):
            assert np.array_equal(CF.bits_of(ref[i], s.D), s.want(preds[i]))
    finally:
        for f in made:
            f.close()


# ------------------------------------------------------------------------------------------ 3: filtered batches = the same batch under a docID-list filter
BATCH_CASES = ["two_all/keep", "eight_columns_any/drop", "also_docset/keep", "set_chunk_edges/drop", "astride_span_%d/drop" % S.SPAN_BITS, "also_create_any/keep", "full_range/drop", "docs_mid_to_D/keep"]


@pytest.fixture(scope="module")
def batches(T, setups, stream):
    """The stream queries, query q under filter q % n, and per filter the documents it drops by the host evaluation."""
    s = setups("stream")
    by_name = {c.name: c for c in CF.cases(s.D)}
    cases = [by_name[n] for n in BATCH_CASES]
    drops = [np.nonzero(s.want(c))[0].astype(np.uint32) for c in cases]
    assert any(len(d) == s.D for d in drops) and all(len(d) for d in drops)
    foq = [i % len(cases) for i in range(len(stream.progs))]
    return s, cases, drops, foq


def two_runs(T, s, cases, drops, progs, foq, flags, topk, opts, dev):
    """(the batch under the column filters, the batch under Filter(index, docids) of the host evaluation); the caller closes both and the filters."""
    cf = []
    for keep in (True, False):
        cf += zip([c.name for c in cases if c.keep == keep], build(T, s.ix, s.cols, [c for c in cases if c.keep == keep], s.also, keep))
    cf = dict(cf)
    col = [cf[c.name] for c in cases]
    ids = [T.Filter(s.ix, d) for d in drops]
    runs = []
    for fl in (col, ids):
        with options(dev, **opts):
            b = T.Batch(s.ix, progs, {1: T.FLAG_DOCUMENTS_ONLY, 2: T.FLAG_ACCUMULATED_SCORE, 0: T.FLAG_MATCHED_TERMS}[flags], topk=topk)
        b.set_filters(fl, foq)
        runs.append(Run(T, s.ix, progs, flags, batch=b))
    return runs, col + ids


@pytest.mark.parametrize("opts", [BITMAP_KERNEL, CANDIDATE_KERNEL], ids=["bitmap_kernel", "candidate_kernel"])
def test_documents_only_batches_equal_the_docid_filtered_ones(T, dev, batches, stream, opts):
    s, cases, drops, foq = batches
    runs, filters = two_runs(T, s, cases, drops, stream.progs, foq, 1, 0, opts, dev)
    try:
        a, b = runs
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.hashes, b.hashes)
        differs = 0
        for i in range(len(stream.progs)):
            assert np.array_equal(a.sets[i], b.sets[i]), (opts, stream.queries[i][0], cases[foq[i]])
            full = stream.want[i]
            exp = full[~np.isin(full, drops[foq[i]])]
            assert np.array_equal(a.sets[i], exp), (opts, stream.queries[i][0], cases[foq[i]])  # (and both are numpy's set minus the dropped documents)
            differs += len(exp) != len(full)
        assert differs > len(stream.progs) // 2
        if not OVERRIDDEN:
            kind = "dense_queries" if opts is BITMAP_KERNEL else "cand_queries"
            assert int(a.info[kind]) > 0 and int(b.info[kind]) > 0, (kind, {k: int(a.info[k]) for k in ("dense_queries", "cand_queries", "pset_queries")})
    finally:
        for x in runs + filters:
            x.close()


@pytest.mark.parametrize("opts", [SCORED_PATHS[2], SCORED_PATHS[0]], ids=["bitmap_kernel", "candidate_kernel"])
def test_scored_top_k_equals_the_docid_filtered_batch_under_check_topk(T, dev, batches, stream, opts):
    s, cases, drops, foq = batches
    sel = sorted(set(range(0, len(stream.progs), 3)) | set(range(len(stream.progs) - len(F.STREAM_EXTRA), len(stream.progs))))  # (every third query, and the rare-lead / tree / phrase extras)
    progs, sfoq = [stream.progs[i] for i in sel], [foq[i] for i in sel]
    runs, filters = two_runs(T, s, cases, drops, progs, sfoq, 2, F.K, opts, dev)
    try:
        a, b = runs
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.top[2], b.top[2])
        if not OVERRIDDEN:  # which kernels the filtered queries ran in: the window-word kernel (k_fused: a bitmap of the window per term) / the candidate-tile kernels (k_and, k_probe)
            ran = {k: int(a.info[k]) for k in KINDS}
            assert {k: int(b.info[k]) for k in KINDS} == ran
            assert (ran["fused_queries"] > 0) if opts is SCORED_PATHS[2] else (ran["cand_queries"] + ran["probe_queries"] > 0), (opts, ran)
        setwise, scored = [0, 0], 0
        for j, i in enumerate(sel):
            docs, scores = stream.ora.get("colfilter:" + cases[sfoq[j]].name, drops[sfoq[j]], progs[j], O.FLAG_ACCUM_SCORE)
            for k, run in enumerate((a, b)):
                setwise[k] += check_top(run, j, docs, scores, F.K, s.w.ora, (opts, stream.queries[i][0], cases[sfoq[j]]))
            scored += len(docs) > 0
        # (check_topk's rule is the whole criterion; which cases it decides set-wise depends on the oracle's scores alone, so it is the same for both runs — and it is
        #  not what decides most of them)
        assert setwise[0] == setwise[1] and 2 * setwise[0] < scored, (setwise, scored)
    finally:
        for x in runs + filters:
            x.close()


@pytest.mark.parametrize("opts", [BITMAP_KERNEL, CANDIDATE_KERNEL], ids=["bitmap_kernel", "candidate_kernel"])
def test_default_mode_matched_terms_equal_the_docid_filtered_batch(T, dev, batches, stream, opts):
    s, cases, drops, foq = batches
    c = s.c
    rq = [(c.q("{r1} {h3}"), 1), (c.q("{r2} {h0} {h1}"), 1), (c.q("{r0} OR {r1}"), 1), (c.q("{r2} {h3}"), 1), (c.q("{r0} OR {r2}"), 1), (c.q("{r1} {h0}"), 1)]
    progs = S.programs(rq)
    rfoq = [(0, 1, 3, 5, 7, 2)[i] for i in range(len(progs))]
    runs, filters = two_runs(T, s, cases, drops, progs, rfoq, 0, 0, opts, dev)
    try:
        a, b = runs
        assert np.array_equal(a.counts, b.counts)
        if not OVERRIDDEN:
            ran = {k: int(a.info[k]) for k in KINDS}
            assert {k: int(b.info[k]) for k in KINDS} == ran
            assert ran["dense_queries" if opts is BITMAP_KERNEL else "cand_queries"] > 0, (opts, ran)
        some = 0
        for i in range(len(progs)):
            assert len(a.rich[i]) == len(b.rich[i]) == 5
            for x, y in zip(a.rich[i], b.rich[i]):
                assert np.array_equal(x, y), (opts, rq[i], cases[rfoq[i]])
            full = c.evaluate(progs[i])
            assert np.array_equal(a.rich[i][0], full[~np.isin(full, drops[rfoq[i]])])
            some += len(a.rich[i][0]) > 0
        assert some >= 3
    finally:
        for x in runs + filters:
            x.close()


# ------------------------------------------------------------------------------------------ 4: facets over a column-filtered batch
def test_a_facet_row_over_a_column_filtered_batch_sums_to_the_match_count(T, batches, stream):
    s, cases, drops, foq = batches
    filters = build(T, s.ix, s.cols, [c for c in cases if c.keep], s.also, True)
    foq = [i % len(filters) for i in range(len(stream.progs))]
    b = T.Batch(s.ix, stream.progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        b.set_filters(filters, foq)
        b.set_facets([(s.cols.made["mod7"], 7), (s.cols.made["window"], 2)])
        b.run()
        b.sync()
        counts = b.counts()
        kept = [c for c in cases if c.keep]
        for k, (name, nb) in enumerate((("mod7", 7), ("window", 2))):
            rows = b.facets(k)
            assert np.array_equal(rows.sum(axis=1).astype(np.uint64), counts)
            for q in range(len(stream.progs)):
                full = stream.want[q]
                exp = full[~s.want(kept[foq[q]])[full]]
                assert np.array_equal(rows[q], np.bincount(np.minimum(s.cols.values[name][exp], nb), minlength=nb + 1)), (name, q)
        assert counts.sum() > 0
    finally:
        b.close()
        for f in filters:
            f.close()


# ------------------------------------------------------------------------------------------ 5: collections
def test_collection_parts_each_carry_their_own_column_filter(T, dev):
    old, new = World(T, dev, 20000, 2000, 10, 42), World(T, dev, 6000, 2000, 10, 7)
    made, parts, cb = [], [], None
    try:
        texts = ["t0 t1", "t0 OR t1 OR t2 OR t3", "t5", "t3 t5 NOT t1", "t0 t1 (t2 OR t3 OR t4)", "t7 OR t9"]
        progs = [O.parse_query(t) for t in texts]
        want = []
        for w, case in ((old, CF.Case("old", [CF.R("mod7", 1, 5), CF.IN("low16", range(0, 65536, 3), negate=True)], keep=True)), (new, CF.Case("new", [CF.R("rev", 100, 3000), CF.R("huge", CF.HUGE, CF.HUGE)], any=True, keep=False))):
            cols = Cols(T, w.ix, w.D)
            made.append(cols)
            f = build(T, w.ix, cols, [case], {}, case.keep)[0]
            made.append(f)
            bits = CF.drop_bits(case, cols.values, w.D)
            assert 0 < bits.sum() < w.D and np.array_equal(CF.bits_of(f.bitmap(), w.D), bits)
            p = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
            p.set_filters([f], [0] * len(progs))
            parts.append(p)
            sets = [w.ora.exec(q, O.FLAG_DOCUMENTS_ONLY)[0] for q in progs]
            want.append([x[~bits[x]] for x in sets])
        cb = T.CollectionBatch(parts)
        cb.run()
        cb.sync()
        counts = cb.counts()
        for i, t in enumerate(texts):
            docs = np.concatenate([want[0][i], want[1][i]])
            assert int(counts[i]) == len(docs) and np.array_equal(cb.docset(i, len(docs)), docs), t
        assert counts.sum() > 0
    finally:
        if cb is not None:
            cb.close()
        for x in parts + made[::-1]:
            x.close()
        old.ix.close()
        new.ix.close()


# ------------------------------------------------------------------------------------------ 6: lifetime, refusals, the pool
def test_a_filter_survives_the_destruction_of_its_columns(T, setups):
    s = setups("tiny")
    cols = Cols(T, s.ix, s.D)
    case = CF.Case("gone", [CF.R("mod7", 2, 4), CF.IN("hash", [1, 2, 3], negate=True)], keep=True)
    f = build(T, s.ix, cols, [case], {}, True)[0]
    b = None
    try:
        cols.close()
        bits = CF.drop_bits(case, s.cols.values, s.D)
        assert np.array_equal(CF.bits_of(f.bitmap(), s.D), bits)
        prog = O.parse_query("t0 OR t1 OR t2")
        b = T.Batch(s.ix, [prog], T.FLAG_DOCUMENTS_ONLY)
        b.set_filters([f], [0])
        b.run()
        b.sync()
        full = s.w.ora.exec(prog, O.FLAG_DOCUMENTS_ONLY)[0]
        assert np.array_equal(b.docset(0), full[~bits[full]]) and 0 < int(b.counts()[0]) < len(full)
    finally:
        if b is not None:
            b.close()
        f.close()


def test_refusals_leave_out_untouched_and_the_pool_gets_its_bytes_back(T, dev, setups):
    from trinity_amd.engine import TriClause, TriPredicate, hip_lib

    L = hip_lib()
    s = setups("stream")  # (its bitmaps are 64 KB each: buffers of the handle's pool, which the pool's byte count sees)
    other = World(T, dev, 2000, 200, 10, 7)
    live = []
    try:
        start = dev.memory()["pool_in_use_bytes"]
        ocols = Cols(T, other.ix, 2000)
        extra = T.Column(s.ix, s.cols.values["one"])  # a ninth column handle of this index
        foreign = T.Filter(other.ix, np.array([1, 2, 3], dtype=np.uint32))
        live += [ocols, extra, foreign]
        mine = s.cols.made
        SENTINEL = 0x5A5A5A5A5A5A
        out = (C.c_void_p * 4)(*[SENTINEL] * 4)
        keepalive = []

        def clause(col, kind=0, lo=1, hi=2, values=None, reserved=0, negate=0):
            c = TriClause()
            c.column, c.kind, c.negate, c.lo, c.hi, c.reserved = (col.h if col is not None else None), kind, negate, lo, hi, reserved
            if values is not None:
                v = np.asarray(values, dtype=np.uint32)
                keepalive.append(v)
                c.set, c.nset = v.ctypes.data, v.size
            return c

        def pred(clauses, nclauses=None, also=None, reserved=0):
            arr = (TriClause * max(1, len(clauses)))(*clauses)
            keepalive.append(arr)
            p = TriPredicate()
            p.clauses, p.nclauses, p.any, p.also, p.reserved = arr, len(clauses) if nclauses is None else nclauses, 0, (also.h if also is not None else None), reserved
            return p

        def call(preds, np_=None, mode=1, ix=s.ix.h, out=out):
            arr = (TriPredicate * max(1, len(preds)))(*preds)
            return L.tri_filters_from_columns(ix, arr, len(preds) if np_ is None else np_, mode, out)

        def refused(rc, *msg):
            text = L.tri_last_error().decode()
            assert rc == -1 and all(x == SENTINEL for x in out), (rc, text)
            assert "tri_filters_from_columns" in text and all(m in text for m in msg), text

        good = pred([clause(mine["mod7"])])
        refused(call([good], ix=None), "null argument")
        refused(L.tri_filters_from_columns(s.ix.h, None, 1, 1, out), "null argument")
        refused(call([good], np_=0), "0 predicates")
        refused(call([good] * 257), "257 predicates")
        refused(call([good], mode=2), "mode 2")
        refused(call([good, pred([clause(ocols.made["mod7"])])]), "predicate 1 clause 0", "another index")
        refused(call([good, pred([clause(mine["mod7"])], also=foreign)]), "predicate 1", "also", "another index")
        refused(call([pred([clause(c) for c in mine.values()]), pred([clause(mine["mod7"]), clause(extra)])]), "predicate 1 clause 1", "distinct columns")
        refused(call([good, pred([clause(mine["mod7"])], nclauses=0)]), "predicate 1", "0 clauses")
        refused(call([good, pred([clause(mine["mod7"])] * 8, nclauses=9)]), "predicate 1", "9 clauses")
        refused(call([good, pred([clause(mine["mod7"]), clause(mine["mod7"], kind=2)])]), "predicate 1 clause 1", "unknown kind 2")
        refused(call([good, pred([clause(mine["mod7"], kind=1, values=[1, 65536])])]), "predicate 1 clause 0", "set value 65536")
        refused(call([good, pred([clause(mine["mod7"], reserved=1)])]), "predicate 1 clause 0", "reserved")
        refused(call([good, pred([clause(mine["mod7"])], reserved=1)]), "predicate 1", "reserved")
        refused(call([good, pred([clause(None)])]), "predicate 1 clause 0", "null argument")
        with pytest.raises(T.TrinityError, match="rc=-1"):
            T.Filter.from_columns(s.ix, [])
        assert dev.memory()["pool_in_use_bytes"] == start  # nothing was allocated
        # the limits themselves are accepted: eight distinct columns, eight clauses, 256 predicates
        ok = T.Filter.from_columns(s.ix, [T.Predicate([T.Clause.range(c, 0, 5) for c in mine.values()])] * CF.MAX_PREDS, keep=False)
        live += ok
        assert len(ok) == CF.MAX_PREDS and dev.memory()["pool_in_use_bytes"] > start
        # tri_filter_bitmap: a capacity below the extent writes nothing and leaves the extent
        n = C.c_size_t()
        small = np.full(8, 0xABCDEF01, dtype=np.uint32)
        assert L.tri_filter_bitmap(ok[0].h, small.ctypes.data, small.size, C.byref(n)) == -1 and n.value == words(s.D) and (small == 0xABCDEF01).all()
        assert L.tri_filter_bitmap(ok[0].h, None, 0, C.byref(n)) == -1 and L.tri_filter_bitmap(ok[0].h, small.ctypes.data, small.size, None) == -1
        for x in live:
            x.close()
        live = []
        assert dev.memory()["pool_in_use_bytes"] == start
    finally:
        for x in live:
            x.close()
        other.ix.close()
