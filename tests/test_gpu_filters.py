"""GPU tests of the per-query document filters (run with -m gpu on an MI355X): tri_filter_create / tri_filter_from_docset / tri_batch_set_filters — ONE batch, many
filters, every query naming one (IndexDocumentsFilter, matches.h:190-201, selected per query on the device: csrc/k_filter.hpp).

References: the genuine reference's records with a rule-backed IndexDocumentsFilter (tests/golden/ref_masked.json: until now they reached the GPU one filter at a time,
through the index-wide mask); structured.Corpus.evaluate minus the filter for docID sets on the stream corpus (three SPAN_BITS windows); the oracle with the filter
installed as its masked set for scores, top-K lists and the default mode's records.

Top-K comparison on the stream corpus as in test_gpu_structured.py (structured.check_topk).  Measured on the oracle by
tests/test_filters_abi.py::test_filtered_top_k_stays_inside_the_tie_cap for exactly these queries and filters: the set-wise rule decides 12 of the 140 scored (query,
filter) cases, 8.6 % (bound: 10 %); the smallest relative gap between distinct scores is 2.45e-06.

One device handle for the file; every index, batch and filter is closed by the test that made it; nothing sleeps, retries or loops over a timing."""
import json
import os

import numpy as np
import pytest

import filter_cases as F
import oracle_lib as O
import structured as S
from test_gpu_parity import GOLDEN, World, options, rich_flat
from test_gpu_structured import OVERRIDDEN, SWorld, T, dev  # noqa: F401  (T, dev: fixtures)

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
EMPTY = np.zeros(0, np.uint32)
KINDS = ("dense_queries", "cand_queries", "pset_queries", "probe_queries", "fused_queries", "planes_queries", "tree_queries")


# ------------------------------------------------------------------------------------------ helpers
def complement(ids, D):
    return np.setdiff1d(np.arange(1, D + 1, dtype=np.uint32), ids).astype(np.uint32)


class Run:
    """One batch with filters, run and read: .counts, and by mode .sets / .hashes (DocumentsOnly), .top = (docs, scores, counts) (top-K), .rich (default mode)."""

    def __init__(self, T, ix, progs, flags, topk=0, filters=(), foq=None, batch=None):
        self.b = batch or T.Batch(ix, progs, {1: T.FLAG_DOCUMENTS_ONLY, 2: T.FLAG_ACCUMULATED_SCORE, 0: T.FLAG_MATCHED_TERMS}[flags], topk=topk)
        self.flags, self.n = flags, len(progs)
        if batch is None and len(filters):
            self.b.set_filters(filters, foq)
        self.read()

    def read(self):
        b = self.b
        b.run()
        b.sync()
        self.counts = b.counts()
        self.info = b.info()
        if self.flags == 1:
            flat, offs = b.docsets()
            self.sets = [flat[int(offs[i]) : int(offs[i + 1])] for i in range(self.n)]
            self.hashes = b.docset_hashes()
        elif self.flags == 2:
            self.top = b.topk_results()
        else:
            self.rich = []
            for i in range(self.n):
                docs = b.docset(i, int(self.counts[i]))
                self.rich.append((docs,) + b.matched_terms(i, len(docs)))
        return self

    def close(self):
        self.b.close()


class Oracle:
    """The oracle's answers under a masked set, computed once per (set, program, mode)."""

    def __init__(self, ora):
        self.ora, self.memo = ora, {}

    def get(self, key, drop, prog, flags):
        k = (key, prog.tobytes(), flags)
        if k not in self.memo:
            self.ora.set_masked(drop)
            try:
                self.memo[k] = self.ora.exec_rich(prog) if flags == 0 else self.ora.exec(prog, flags)
            finally:
                self.ora.set_masked(EMPTY)
        return self.memo[k]


def check_docs(run, i, want, tag, fnv=None):
    assert int(run.counts[i]) == len(want), (tag, int(run.counts[i]), len(want))
    assert np.array_equal(run.sets[i], want), tag
    assert int(run.hashes[i]) == (O.fnv1a_docs(want) if fnv is None else fnv), tag


def check_top(run, i, docs, scores, k, ora, tag):
    """counts, then the top-K through structured.check_topk; returns 1 when its set-wise rule decided."""
    d, s, c = run.top
    assert int(run.counts[i]) == len(docs) and int(c[i]) == min(k, len(docs)), (tag, int(run.counts[i]), len(docs), int(c[i]))
    return int(S.check_topk(d[i, : int(c[i])], s[i, : int(c[i])], docs, scores, k, ora, tag))


def check_rich(run, i, want, tag):
    wdocs, wflat, _, _ = want
    docs, terms, present, freq, pos = run.rich[i]
    assert np.array_equal(docs, wdocs), tag
    assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), tag


# ------------------------------------------------------------------------------------------ 1 + 2: the reference's records, many filters in one batch, both polarities
@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "ref_masked.json")))


@pytest.mark.parametrize("keep", [False, True], ids=["drop", "keep"])
@pytest.mark.parametrize("corpus", ["tiny", "dense"])
def test_reference_records_many_filters_in_one_batch(T, dev, golden, corpus, keep):
    """Per mode ONE batch holds the records of all three filters (5 %, 30 %, 90 % dropped), interleaved, every fourth query unfiltered; each query names its filter and
    no index mask is set.  keep: every filter handed over as its complement in 1 .. D with TRI_FILTER_KEEP — the same records."""
    c = golden["corpora"][corpus]
    w = World(T, dev, c["D"], c["V"], c["slots"], c["seed"])
    filters = []
    try:
        for fs, pm in golden["filters"]:
            with np.errstate(over="ignore"):
                ids = O.masked_docs(c["D"], fs, pm)
            filters.append(T.Filter(w.ix, complement(ids, c["D"]) if keep else ids, keep=keep))
        seen = 0
        for flags in (1, 2, 0):
            per = [[r for r in golden["results"] if r["corpus"] == corpus and r["filter"] == f and r["flags"] == flags] for f in golden["filters"]]
            assert len({len(x) for x in per}) == 1 and all(a["q"] == b["q"] for a, b in zip(per[0], per[2]))
            recs, foq = [], []
            for i in range(len(per[0])):
                for j in range(3):
                    recs.append(per[j][i])
                    foq.append(j)
                recs.append(None)  # the same query, unfiltered: against the oracle without a mask
                foq.append(NONE)
            progs = [O.parse_query(per[0][i // 4]["q"], some_min=per[0][i // 4]["min"] or 1) for i in range(len(recs))]
            for opts in ({}, {"dense_min_postings": 0}) if flags == 2 else ({},):
                with options(dev, **opts):
                    b = T.Batch(w.ix, progs, {1: T.FLAG_DOCUMENTS_ONLY, 2: T.FLAG_ACCUMULATED_SCORE, 0: T.FLAG_MATCHED_TERMS}[flags], topk=10 if flags == 2 else 0)
                b.set_filters(filters, foq)
                run = Run(T, w.ix, progs, flags, batch=b)
                try:
                    for i, (r, p) in enumerate(zip(recs, progs)):
                        tag = (corpus, keep, flags, opts, i, per[0][i // 4]["q"], foq[i])
                        if flags == 1:
                            if r is None:
                                check_docs(run, i, w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0], tag)
                            else:
                                assert len(run.sets[i]) == r["n"] == int(run.counts[i]) and str(O.fnv1a_docs(run.sets[i])) == r["fnv"] == str(int(run.hashes[i])), tag
                        elif flags == 2:
                            d, s, cnt = run.top
                            if r is None:
                                docs, scores = w.ora.exec(p, O.FLAG_ACCUM_SCORE)
                                top = list(zip(*[x.tolist() for x in w.ora.topk(docs, scores, 10)]))
                                n = len(docs)
                            else:
                                top, n = r.get("top", []), r["n"]
                            assert int(run.counts[i]) == n and int(cnt[i]) == len(top), tag
                            assert d[i, : len(top)].tolist() == [x[0] for x in top], tag
                            np.testing.assert_allclose(s[i, : len(top)], [x[1] for x in top], rtol=1e-5, atol=0, err_msg=str(tag))
                        else:
                            docs, terms, present, freq, pos = run.rich[i]
                            if r is None:
                                check_rich(run, i, w.ora.exec_rich(p), tag)
                            else:
                                assert len(docs) == r["n"] and int(freq.sum()) == r["hits_total"], tag
                                assert int(sum(bin(int(x)).count("1") for x in present)) == r["terms_total"], tag
                                assert str(O.fnv1a_u32_stream(rich_flat(docs, terms, present, freq, pos))) == r["rich_fnv"], tag
                finally:
                    run.close()
            seen += len(recs)
        assert seen >= 4 * (85 + 85 + 84)
    finally:
        for f in filters:
            f.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ 3: filter ∪ mask, taken at run time
@pytest.mark.parametrize("flags", [1, 2], ids=["docs", "top10"])
def test_filter_and_mask_are_combined_when_the_batch_runs(T, dev, golden, flags):
    """Index mask = filter A's documents, the queries name B: A ∪ B is dropped.  The mask cleared, the SAME batch run again: B alone.  Another assignment between two
    runs; then nf = 0: the results of a batch that never had filters."""
    c = golden["corpora"]["dense"]
    w = World(T, dev, c["D"], c["V"], c["slots"], c["seed"])
    with np.errstate(over="ignore"):
        A, B, Cc = (O.masked_docs(c["D"], fs, pm) for fs, pm in golden["filters"])
    texts = sorted({(r["q"], r["min"] or 1) for r in golden["results"] if r["corpus"] == "dense" and r["flags"] == flags})
    progs = [O.parse_query(q, some_min=mn) for q, mn in texts]
    ora = Oracle(w.ora)
    oflags = O.FLAG_DOCUMENTS_ONLY if flags == 1 else O.FLAG_ACCUM_SCORE
    fb, fc = T.Filter(w.ix, B), T.Filter(w.ix, Cc)
    run = plain = None

    def check(run, drops, step):
        for i, p in enumerate(progs):
            key, drop = drops[i]
            docs, scores = ora.get(key, drop, p, oflags)
            if flags == 1:
                check_docs(run, i, docs, (step, texts[i]))
            else:
                check_top(run, i, docs, scores, 10, w.ora, (step, texts[i]))

    try:
        w.ix.set_masked(A)
        run = Run(T, w.ix, progs, flags, topk=10 if flags == 2 else 0, filters=[fb], foq=[0] * len(progs))
        check(run, [("A|B", np.union1d(A, B).astype(np.uint32))] * len(progs), "mask A, filter B")
        w.ix.set_masked(EMPTY)
        check(run.read(), [("B", B)] * len(progs), "mask cleared, the same batch")
        run.b.set_filters([fb, fc], [(1, NONE, 0)[i % 3] for i in range(len(progs))])
        check(run.read(), [(("C", Cc), ("none", EMPTY), ("B", B))[i % 3] for i in range(len(progs))], "another assignment")
        run.b.set_filters([])
        run.read()
        plain = Run(T, w.ix, progs, flags, topk=10 if flags == 2 else 0)
        assert np.array_equal(run.counts, plain.counts)
        if flags == 1:
            assert np.array_equal(run.hashes, plain.hashes) and all(np.array_equal(a, b) for a, b in zip(run.sets, plain.sets))
        else:
            assert all(np.array_equal(a, b) for a, b in zip(run.top, plain.top))
        check(plain, [("none", EMPTY)] * len(progs), "never filtered")
    finally:
        w.ix.set_masked(EMPTY)
        for x in (run, plain, fb, fc):
            if x is not None:
                x.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ 4 + 5: boundaries, every kernel
@pytest.fixture(scope="module")
def stream():
    class Ref:
        pass

    r = Ref()
    r.c = S.stream_corpus()
    r.queries = F.stream_queries(r.c)
    r.progs = S.programs(r.queries)
    r.want = [r.c.evaluate(p) for p in r.progs]  # unfiltered, once
    r.filters = F.stream_filters()
    r.drops = {n: F.dropped(f, r.c.D) for n, f in r.filters.items()}
    r.drops["none"] = EMPTY
    r.ora = Oracle(r.c.oracle())
    r.expect = {}  # (query, filter) -> (numpy's set minus the filter, its FNV): worked out once, shared by every batch that holds the pair
    return r


def expected(stream, qi, name):
    if (qi, name) not in stream.expect:
        full = stream.want[qi]
        exp = full[~np.isin(full, stream.drops[name])] if len(stream.drops[name]) else full
        stream.expect[qi, name] = (exp, O.fnv1a_docs(exp))
    return stream.expect[qi, name]


DOCS_PATHS = [{}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}, {"planes": 0}, {"plane_div": S.ALL_PLANES, "probe_max_blocks": 1 << 20}]
SCORED_PATHS = [{}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}, {"dense_min_postings": 0, "planes": 0, "fused_halfwords": 0}, {"dense_min_postings": 0, "fused": 0}]


@pytest.mark.parametrize("codec", [1, 2])
def test_boundary_filters_through_every_kernel(T, dev, stream, codec):
    """The stream corpus, every query under every filter of filter_cases.stream_filters and unfiltered in ONE batch, the batch planned under the option sets that force
    each matching kernel: docID sets = numpy minus the filter; top-10 = the oracle with the filter as its mask.  Info counters say that filtered queries ran in every
    kind (k_and_dense, k_and, k_psets, k_probe, k_fused, k_planes, the tree kernels)."""
    w = SWorld(T, dev, stream.c, codec)
    names = list(stream.filters) + ["none"]
    filters = [T.Filter(w.ix, ids, keep=keep) for ids, keep in stream.filters.values()]
    progs, foq, which = [], [], []
    for qi, p in enumerate(stream.progs):
        for j, n in enumerate(names):
            progs.append(p)
            foq.append(NONE if n == "none" else j)
            which.append((qi, n))
    ran = dict.fromkeys(KINDS, 0)
    setwise = scored = 0
    try:
        for opts in DOCS_PATHS:
            with options(dev, **opts):
                b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
            b.set_filters(filters, foq)
            run = Run(T, w.ix, progs, 1, batch=b)
            try:
                for i, (qi, n) in enumerate(which):
                    exp, fnv = expected(stream, qi, n)
                    check_docs(run, i, exp, (codec, opts, stream.queries[qi][0], n), fnv)
                    assert n != "all" or int(run.counts[i]) == 0
                for k in KINDS:
                    ran[k] = max(ran[k], int(run.info[k]))
            finally:
                run.close()
        for opts in SCORED_PATHS:
            with options(dev, **opts):
                b = T.Batch(w.ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=F.K)
            b.set_filters(filters, foq)
            run = Run(T, w.ix, progs, 2, batch=b)
            try:
                for i, (qi, n) in enumerate(which):
                    docs, scores = stream.ora.get(n, stream.drops[n], stream.progs[qi], O.FLAG_ACCUM_SCORE)
                    assert len(docs) == len(expected(stream, qi, n)[0])
                    setwise += check_top(run, i, docs, scores, F.K, w.ora, (codec, opts, stream.queries[qi][0], n))
                    scored += len(docs) > 0
                    assert n != "all" or (int(run.counts[i]) == 0 and int(run.top[2][i]) == 0)
                for k in KINDS:
                    ran[k] = max(ran[k], int(run.info[k]))
            finally:
                run.close()
        assert setwise <= 0.10 * scored, (setwise, scored)
        if not OVERRIDDEN:
            assert all(ran[k] > 0 for k in KINDS), ran
    finally:
        for f in filters:
            f.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ 6: a filter made of a batch's docset, on the device
def test_filter_from_docset_in_both_forms(T, dev, stream):
    """A DocumentsOnly batch holds a head-term union (kept as a bitmap) and a rare conjunction (kept as docIDs); KEEP filters are made of each and the batch is closed.
    A scored top-10 batch and a default-mode batch of other queries, restricted to them, equal the oracle masked by the complement of its own docset for the filter
    query — the scores are the query's alone."""
    c = stream.c
    w = SWorld(T, dev, c, 1)
    fprogs = S.programs([(c.q("{h0} OR {h1}"), 1), (c.q("{r2} {h3}"), 1)])
    filters = []
    try:
        with options(dev, result_bitmaps=1):
            fb = T.Batch(w.ix, fprogs, T.FLAG_DOCUMENTS_ONLY)
        fb.run()
        fb.sync()
        if not OVERRIDDEN:
            assert fb.docset_form(0) == 1 and fb.docset_form(1) == 0
        filters = [T.Filter.from_docset(fb, 0), T.Filter.from_docset(fb, 1, keep=True)]
        drop0 = T.Filter.from_docset(fb, 1, keep=False)
        filters.append(drop0)
        fb.close()
        fsets = [w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in fprogs]
        drops = [("keep0", complement(fsets[0], c.D)), ("keep1", complement(fsets[1], c.D)), ("drop1", fsets[1])]
        qs = [q for q in F.stream_queries(c) if q[0] not in (c.q("{h0} OR {h1}"), c.q("{r2} {h3}"))][::3]
        progs = S.programs(qs)
        foq = [i % 3 for i in range(len(progs))]
        run = Run(T, w.ix, progs, 2, topk=F.K, filters=filters, foq=foq)
        try:
            for i, p in enumerate(progs):
                docs, scores = stream.ora.get(drops[foq[i]][0], drops[foq[i]][1], p, O.FLAG_ACCUM_SCORE)
                check_top(run, i, docs, scores, F.K, w.ora, ("scored", qs[i][0], foq[i]))
        finally:
            run.close()
        # the default mode, on small sets: every query restricted to the rare conjunction's documents; the rare-lead queries also to the union's
        rq = [(q, 1) for q, _ in qs[:6]] + [(c.q("{r1} {h3}"), 0), (c.q("{r2} {h0} {h1}"), 0), (c.q("{r0} OR {r1}"), 0)]
        rprogs = S.programs([(q, 1) for q, _ in rq])
        rfoq = [f for _, f in rq]
        run = Run(T, w.ix, rprogs, 0, filters=filters, foq=rfoq)
        try:
            for i, p in enumerate(rprogs):
                check_rich(run, i, stream.ora.get(drops[rfoq[i]][0], drops[rfoq[i]][1], p, 0), ("rich", rq[i]))
        finally:
            run.close()
    finally:
        for f in filters:
            f.close()
        w.ix.close()


# ------------------------------------------------------------------------------------------ 7: collections
def test_collection_parts_carry_their_own_filters(T, dev):
    """A tri_cbatch of two parts, each with its own filters (and the older index its mask): counts add up to the two oracles', ONE top-10 merges."""
    old = World(T, dev, 20000, 2000, 10, 42)
    new = World(T, dev, 6000, 2000, 10, 7)
    made = []
    try:
        old.ix.set_masked(np.arange(1, 6001, dtype=np.uint32))
        rng = np.random.default_rng(11)
        fo = [np.unique(rng.integers(1, 20001, 7000)).astype(np.uint32), np.arange(6001, 20001, 2, dtype=np.uint32)]
        fn = [np.unique(rng.integers(1, 6001, 1500)).astype(np.uint32), np.arange(3000, 6001, dtype=np.uint32)]
        texts = ["t0 t1", "t0 OR t1 OR t2 OR t3", "t5", "[t0, t1, t2]", "t3 t5 NOT t1", "t0 t1 (t2 OR t3 OR t4)", '"t0 t1" t2', "t2 OR (t0 t1)", "t7 OR t9", "t1 t2 t3"]
        progs = [O.parse_query(t, some_min=2) for t in texts]
        foq_o = [(0, 1, NONE)[i % 3] for i in range(len(progs))]
        foq_n = [(1, NONE, 0)[i % 3] for i in range(len(progs))]
        made += [T.Filter(old.ix, x) for x in fo] + [T.Filter(new.ix, x) for x in fn]
        want = []
        for i, p in enumerate(progs):
            old.ora.set_masked(np.union1d(np.arange(1, 6001), fo[foq_o[i]] if foq_o[i] != NONE else EMPTY).astype(np.uint32))
            new.ora.set_masked(fn[foq_n[i]] if foq_n[i] != NONE else EMPTY)
            do, so = old.ora.exec(p, O.FLAG_ACCUM_SCORE)
            dn, sn = new.ora.exec(p, O.FLAG_ACCUM_SCORE)
            want.append((np.concatenate([do, dn]), np.concatenate([so, sn])))
        old.ora.set_masked(EMPTY)
        new.ora.set_masked(EMPTY)
        for mode, topk in ((T.FLAG_DOCUMENTS_ONLY, 0), (T.FLAG_ACCUMULATED_SCORE, 10)):
            parts = [T.Batch(w.ix, progs, mode, topk=topk) for w in (old, new)]
            parts[0].set_filters(made[:2], foq_o)
            parts[1].set_filters(made[2:], foq_n)
            cb = T.CollectionBatch(parts)
            try:
                cb.run()
                cb.sync()
                counts = cb.counts()
                for i, (docs, scores) in enumerate(want):
                    assert int(counts[i]) == len(docs), (texts[i], int(counts[i]), len(docs))
                    if topk:
                        d, s, cn = cb.topk_results()
                        assert int(cn[i]) == min(10, len(docs))
                        S.check_topk(d[i, : int(cn[i])], s[i, : int(cn[i])], docs, scores, 10, old.ora, texts[i])
                    else:
                        assert np.array_equal(cb.docset(i, len(docs)), docs), texts[i]
            finally:
                cb.close()
                for b in parts:
                    b.close()
    finally:
        for f in made:
            f.close()
        old.ix.close()
        new.ix.close()


# ------------------------------------------------------------------------------------------ 8: refusals, and the pool
def test_refusals_change_nothing_and_the_pool_gets_its_bytes_back(T, dev, stream):
    c = stream.c
    w = SWorld(T, dev, c, 1)
    other = World(T, dev, 2000, 200, 10, 42)
    qs = F.stream_queries(c)[:12]
    progs = S.programs(qs)
    live = []
    try:
        warm = Run(T, w.ix, progs, 1)  # (the index's plane cache — plane 0 and, with the first scored batch, the high parts — is in place before the pool is read)
        base_sets = warm.sets
        warm.close()
        Run(T, w.ix, progs, 2, topk=10).close()
        start = dev.memory()["pool_in_use_bytes"]
        span, _ = stream.filters["span"]
        f = T.Filter(w.ix, span)
        foreign = T.Filter(other.ix, np.array([1, 2, 3], dtype=np.uint32))
        live += [f, foreign]
        assert dev.memory()["pool_in_use_bytes"] > start
        run = Run(T, w.ix, progs, 1, filters=[f], foq=[0] * len(progs))
        live.append(run)
        first = [s.copy() for s in run.sets]
        with pytest.raises(T.TrinityError, match="rc=-1"):  # a filter of another index
            run.b.set_filters([f, foreign], [0] * len(progs))
        with pytest.raises(T.TrinityError, match="rc=-1"):  # filter_of_query[q] = nf
            run.b.set_filters([f], [0] * (len(progs) - 1) + [1])
        run.read()
        assert all(np.array_equal(a, b) for a, b in zip(run.sets, first))  # nothing changed
        assert any(len(a) != len(b) for a, b in zip(first, base_sets))  # (and the filter does drop documents of these queries)
        scored = T.Batch(w.ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=10)
        live.append(scored)
        scored.run()
        scored.sync()
        with pytest.raises(T.TrinityError, match="rc=-1"):  # a filter is made of a DocumentsOnly batch
            T.Filter.from_docset(scored, 0)
        for x in live:
            x.close()
        live = []
        assert dev.memory()["pool_in_use_bytes"] == start
    finally:
        for x in live:
            x.close()
        w.ix.close()
        other.ix.close()
