"""GPU tests on STRUCTURED segments (run with -m gpu on an MI355X): the matching, scoring, phrase, delivery and top-K kernels on the corpora of tests/structured.py —
documents exactly on every window boundary, lists empty for whole windows, dense lists whose deferred blocks overflow k_and_dense's LDS list, frequencies on the plane
levels and the fused fields' caps, scores that rise with the docID, results where everything ties — instead of the i.i.d. corpus every other GPU test reads.

The reference for docID sets and counts is structured.Corpus.evaluate (numpy over the postings arrays: no codec involved; tests/test_structured.py shows it equals the
oracle); for scores and the default mode's records it is the oracle over the GOOGLE bytes of the same postings, also for the LUCENE-coded upload (the relation
test_gpu_parity.World relies on).

Top-K comparison (structured.check_topk): scores position by position at rtol = 1e-5; docIDs exactly wherever all distinct oracle scores within ranks 1 .. K + 1 differ by
more than that tolerance, else as sets per group of scores within tolerance.  Measured on the oracle by tests/test_structured.py::test_score_gap_condition: 5.0 % of
the scored (query, K, similarity) cases fall under the set-wise rule (bound: 10 %); the smallest relative gap between distinct scores is 3.1e-11 — sums of the same
addends in another order.

One device handle for the file; every uploaded index is closed by its fixture; nothing retries."""
import os

import numpy as np
import pytest

import oracle_lib as O
import structured as S
from test_gpu_parity import options, rich_flat, run_docs_only, run_rich, run_scored

pytestmark = pytest.mark.gpu
OVERRIDDEN = bool(os.environ.get("TRINITY_TEST_OPTIONS", "").strip())  # (a run-wide option set may force other paths: info() counters are asserted only without one)


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


class SWorld:
    """A structured corpus uploaded in one codec: .T / .ix as test_gpu_parity's helpers want them, .c the corpus, .ora the oracle over its GOOGLE bytes."""

    def __init__(self, T, dev, corpus, codec):
        self.T, self.dev, self.c, self.codec = T, dev, corpus, codec
        self.ora = corpus.oracle()
        self.ix = corpus.upload(T, dev, codec)
        self._want, self._scores = {}, {}

    def want(self, key, queries):
        """(programs, numpy docID sets, their FNV hashes) of a query list, evaluated once."""
        if key not in self._want:
            progs = S.programs(queries)
            sets = [self.c.evaluate(p) for p in progs]
            self._want[key] = (progs, sets, [O.fnv1a_docs(s) for s in sets])
        return self._want[key]

    def scores(self, key, progs, sim=0, masked=None):
        """The oracle's (docs, scores) of a program list under a similarity (and a masked set), computed once."""
        if key not in self._scores:
            self.ora.set_similarity(sim)
            self.ora.set_masked(masked if masked is not None else np.zeros(0, np.uint32))
            try:
                self._scores[key] = [self.ora.exec(p, O.FLAG_ACCUM_SCORE) for p in progs]
            finally:
                self.ora.set_similarity(0)
                self.ora.set_masked(np.zeros(0, np.uint32))
        return self._scores[key]


@pytest.fixture(scope="module")
def corpora():
    made = {}

    def get(name):
        if name not in made:
            made[name] = S.main_corpus(docs_cnt=S.D_MAIN + 2 * S.SPAN_BITS) if name == "main_wide" else S.CORPORA[name]()
        return made[name]

    return get


@pytest.fixture(scope="module")
def worlds(T, dev, corpora):
    made = {}

    def get(name, codec):
        if (name, codec) not in made:
            made[name, codec] = SWorld(T, dev, corpora(name), codec)
        return made[name, codec]

    yield get
    for w in made.values():
        w.ix.close()


def check_docsets(w, queries, progs, want, hashes, opts, masked=None):
    with options(w.dev, **opts):
        sets, got_h, info = run_docs_only(w, progs)
    total = 0
    for (text, mn), got, h, full, fh in zip(queries, sets, got_h, want, hashes):
        exp = full if masked is None else full[~np.isin(full, masked)]
        assert np.array_equal(got, exp), (w.codec, opts, text, mn, len(got), len(exp))
        assert int(h) == (fh if masked is None else O.fnv1a_docs(exp)), (w.codec, opts, text)
        total += len(exp)
    assert info["matches"] == total and info["unsupported_queries"] == 0, (opts, info["matches"], total)
    return info


def check_scored(w, key, queries, progs, counts_want, k, opts, sim=0, masked=None):
    """One scored top-K batch under an option set: match counts against numpy, top-K against the oracle.  Returns (info-free) the number of set-wise comparisons."""
    ref = w.scores((key, sim, masked is not None), progs, sim, masked)
    with options(w.dev, **opts):
        d, s, c, counts = run_scored(w, progs, k, similarity=sim)
    setwise = 0
    for i, (text, mn) in enumerate(queries):
        docs, scores = ref[i]
        assert int(counts[i]) == counts_want[i] == len(docs), (w.codec, opts, k, sim, text, int(counts[i]), counts_want[i])
        assert int(c[i]) == min(k, len(docs)), (w.codec, opts, k, sim, text)
        setwise += S.check_topk(d[i, : int(c[i])], s[i, : int(c[i])], docs, scores, k, w.ora, (w.codec, opts, k, sim, text))
    return setwise


# ------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", ["main", "freq", "tall", "phrase"])
def test_decode_equals_the_postings(worlds, name, codec):
    """decode_terms of every list of every corpus == the postings that were encoded (frequencies 0 and 300, two- to four-byte deltas, lists of 1 .. D documents)."""
    w = worlds(name, codec)
    c = w.c
    docs, freqs, offs = w.ix.decode_terms(np.arange(len(c.names), dtype=np.uint32), c.df())
    assert np.array_equal(offs, c.term_first)
    assert np.array_equal(docs, c.docs), [n for t, n in enumerate(c.names) if not np.array_equal(docs[int(offs[t]) : int(offs[t + 1])], c.lists[n][0])]
    assert np.array_equal(freqs, c.freqs), [n for t, n in enumerate(c.names) if not np.array_equal(freqs[int(offs[t]) : int(offs[t + 1])], c.lists[n][1])]


# ------------------------------------------------------------------------------------------ DocumentsOnly
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", ["main", "main_wide"])
def test_docsets_match_numpy(worlds, name, codec):
    """Sets, counts and docset hashes of every catalogue query — ordered pairs as AND / OR / NOT, triples and CNFs, optional forms, matchsome at 1 .. 3, a nine-term
    tree — under the option sets that send them through k_and (candidate tiles), k_and_dense (rows decoded: the deferred-block overflow, the single-lane block,
    the sparse flag's two sides), k_psets (planes) and both result forms.  `main_wide`: docs_cnt = D + 2 SPAN_BITS, the trailing documents have no postings."""
    w = worlds(name, codec)
    queries = S.main_queries(w.c)
    progs, want, hashes = w.want("main", queries)
    seen = {"dense_queries": 0, "cand_queries": 0, "pset_queries": 0, "bitmap_queries": 0, "tree_queries": 0, "fused_queries": 0}
    sets = S.DOCS_OPTION_SETS if name == "main" else S.DOCS_OPTION_SETS[:3]
    for opts, _ in sets:
        info = check_docsets(w, queries, progs, want, hashes, opts)
        for k in seen:
            seen[k] += info[k]
        if not OVERRIDDEN and opts == {"dense_min_postings": 0, "planes": 0}:
            assert info["dense_queries"] > 300 and info["pset_queries"] == 0, info
    if not OVERRIDDEN:
        assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", ["main", "main_wide"])
def test_result_bitmaps_bit_by_bit(worlds, name, codec):
    """RESULT_BITMAP results through k_psets and k_and_dense, word by word: bit j of word i is document first + 32 i + j and nothing else — no bit for docID 0, none
    above docs_cnt (main_wide: none above the last posting either), every word of a window the lead group skips (`holes`, `lastwin`, `firstwin`, `midwin`) zero."""
    w = worlds(name, codec)
    c = w.c
    texts = ["{all} OR {odd}", "{all} {odd}", "{all} OR {edges}", "{odd} OR {holes}", "{all} NOT {lastwin}", "{holes} OR {stub}", "{holes} {all}", "{lastwin} OR {stub}", "{lastwin} {all}", "{firstwin} OR {first1}",
             "{firstwin} {odd}", "{midwin} OR {last1}", "{midwin} {all}", "{all} NOT {all}", "{all} NOT {odd}", "({all} OR {odd}) ({holes} OR {lastwin})", "{dense_many_slow} OR {firstwin}", "{dense_many_slow} {all}",
             "{rnd3} OR {rnd10}", "{all} {edges}", "{all} OR {last1}", "{odd} OR {first1} OR {last1}"]  # fmt: skip
    queries = [(c.q(t), 1) for t in texts]
    progs, want, _ = w.want("bitmaps", queries)
    nbm = 0
    for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}, {"plane_div": S.ALL_PLANES}):
        with options(w.dev, **opts):
            b = w.T.Batch(w.ix, progs, w.T.FLAG_DOCUMENTS_ONLY)
        b.run()
        b.sync()
        counts = b.counts()
        for i, (text, _) in enumerate(queries):
            assert int(counts[i]) == len(want[i]), (opts, texts[i])
            bm = b.docset_bitmap(i)
            if bm is None:
                assert np.array_equal(b.docset(i, len(want[i])), want[i]), (opts, texts[i])
                continue
            nbm += 1
            first, words = bm
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")
            got = np.nonzero(bits)[0].astype(np.int64) + first
            assert first % 32 == 0 and (first > 0 or bits[0] == 0), (opts, texts[i])
            assert got.size == 0 or (got[0] >= 1 and got[-1] <= c.D <= c.docs_cnt), (opts, texts[i], got[:1], got[-1:])
            assert np.array_equal(got.astype(np.uint32), want[i]), (opts, texts[i], got.size, len(want[i]))
            span = np.arange(first // S.SPAN_BITS, (first + 32 * words.size + S.SPAN_BITS - 1) // S.SPAN_BITS)
            empty = np.setdiff1d(span, np.unique(want[i] // S.SPAN_BITS))
            for win in empty.tolist():  # (implied by the equality above; named, because a skipped window's words are written by a path of their own)
                lo, hi = max(win * S.SPAN_BITS - first, 0) // 32, max(min((win + 1) * S.SPAN_BITS - first, 32 * words.size), 0) // 32
                assert not words[lo:hi].any(), (opts, texts[i], win)
        b.close()
    if not OVERRIDDEN:
        assert nbm >= 3 * len(texts) // 2, nbm


@pytest.mark.parametrize("codec", [1, 2])
def test_mixed_delivery_after_odd_counts(worlds, codec):
    """k_deliver_docsets, both entry points: docID-form results of 1, 2 and 3 (mod 4) documents each directly before a bitmap-form result, so that the bitmap's
    words land at word offsets of the flat buffer that are not multiples of four."""
    w = worlds("main", codec)
    queries = S.mixed_queries(w.c)
    progs, want, _ = w.want("mixed", queries)
    b = w.T.Batch(w.ix, progs, w.T.FLAG_DOCUMENTS_ONLY)
    try:
        for rep in range(2):
            b.run()
            b.sync()
            flat, offs = b.docsets()
            assert offs.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist()
            for i, (text, _) in enumerate(queries):
                assert np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], want[i]), (rep, text)
            mflat, moffs, forms = b.docsets_mixed()
            if not OVERRIDDEN:
                assert forms.tolist() == [0, 1] * (len(queries) // 2) and {int(moffs[i]) % 4 for i in range(1, len(queries), 2)} >= {1, 2, 3}, (forms, moffs)
            for i, (text, _) in enumerate(queries):
                part = mflat[int(moffs[i]) : int(moffs[i + 1])]
                if forms[i]:
                    bits = np.unpackbits(part.view(np.uint8), bitorder="little")
                    assert np.array_equal(np.nonzero(bits)[0].astype(np.uint32), want[i]), (rep, text)
                else:
                    assert np.array_equal(part, want[i]), (rep, text)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ scored top-K
@pytest.mark.parametrize("codec", [1, 2])
def test_scored_topk_on_frequency_patterns(worlds, codec):
    """BM25 top-K for K in {1, 10, 255, 256} over the frequency corpus: the cycle through f = 0, the plane levels and the fused fields' natural caps (no fused_freq_cap:
    6 / 14 / 30 / 254 saturate on 7, 15 / 16, 31 / 32, 255 / 256, 300), constant 1 (all ties: docID ascending decides), scores rising and falling with the docID, the best
    three on the last documents of the last task; lists of K - 1, K, K + 1 documents.  One option set per kernel variant."""
    w = worlds("freq", codec)
    queries = S.freq_queries(w.c)
    progs, want, _ = w.want("freq", queries)
    counts_want = [len(x) for x in want]
    assert {len(x) for x in want} >= {k + s for k in S.K_VALUES for s in (-1, 0, 1)} - {0}
    setwise = cases = 0
    for opts, kinds in S.SCORED_OPTION_SETS:
        for k in S.K_VALUES:
            setwise += check_scored(w, "freq", queries, progs, counts_want, k, opts)
            cases += len(queries)
        if not OVERRIDDEN and opts:
            with options(w.dev, **opts):
                b = w.T.Batch(w.ix, progs, w.T.FLAG_ACCUMULATED_SCORE, topk=10)
            b.run()
            b.sync()
            info = b.info()
            b.close()
            assert (info["planes_queries"] > 20) == ("n_planes" in kinds) and (info["fused_queries"] > 20) == ("n_fused" in kinds or "n_fused16" in kinds), (opts, info)
    assert setwise <= cases // 10, (setwise, cases)


@pytest.mark.parametrize("sim", ["bm25", "tfidf", "trivial"])
@pytest.mark.parametrize("codec", [1, 2])
def test_scored_topk_where_everything_ties(worlds, codec, sim):
    """Constant-frequency lists: every match of a query has the same score under BM25, TF-IDF and Trivial, so the top K are the K smallest docIDs — through the pruned
    candidate buffers (PLK_CAP / FUS_CAP) and k_topk_merge, whose running threshold no later document beats."""
    w = worlds("freq", codec)
    simid = {"bm25": O.SIM_BM25, "tfidf": O.SIM_TFIDF, "trivial": O.SIM_TRIVIAL}[sim]
    queries = S.tie_queries(w.c)
    progs, want, _ = w.want("ties", queries)
    for opts, _ in S.SCORED_OPTION_SETS:
        for k in S.K_VALUES:
            assert check_scored(w, "ties", queries, progs, [len(x) for x in want], k, opts, sim=simid) == 0
            with options(w.dev, **opts):
                d, s, c, _ = run_scored(w, progs, k, similarity=simid)
            for i in range(len(queries)):  # said outright: the K smallest docIDs, one score
                assert d[i, : int(c[i])].tolist() == want[i][:k].tolist() and len(set(s[i, : int(c[i])].tolist())) == 1, (opts, k, sim, queries[i][0])


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", ["main", "tall", "phrase"])
def test_scored_topk_on_structure(worlds, name, codec):
    """Scored top-K on the boundary lists, the tall corpus' unions and the phrase corpus: counts against numpy, top-K against the oracle — the planner's choice, the
    one-pass kernels forced (planes, then window words), match-then-score forced."""
    w = worlds(name, codec)
    qf, ks = S.SCORED_CASES[name]
    queries = qf(w.c)
    progs, want, _ = w.want("scored", queries)
    for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}, {"dense_min_postings": 0, "fused": 0}):
        for k in ks:
            check_scored(w, "scored", queries, progs, [len(x) for x in want], k, opts)


# ------------------------------------------------------------------------------------------ the default mode
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", ["freq", "phrase"])
def test_rich_mode_reports_what_the_oracle_reports(worlds, name, codec):
    """Matched terms, frequencies and positions: frequencies 0 and 300 of the cycle, the phrase corpus' repeated positions and positions up to 65535."""
    w = worlds(name, codec)
    queries = S.rich_freq_queries(w.c) if name == "freq" else S.phrase_queries(w.c)
    progs, want, _ = w.want("rich", queries)
    freqs_seen = set()
    for (text, mn), p, exp, (docs, terms, present, freq, pos) in zip(queries, progs, want, run_rich(w, progs)):
        wdocs, wflat, tt, ht = w.ora.exec_rich(p)
        assert np.array_equal(docs, exp) and np.array_equal(docs, wdocs), (text, len(docs), len(exp))
        assert int(freq.sum()) == ht and int(sum(bin(int(x)).count("1") for x in present)) == tt, text
        assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), text
        freqs_seen |= set(freq.ravel().tolist())
    if name == "freq":
        assert {0, 7, 256, 300} <= freqs_seen
    else:
        assert int(max(freqs_seen)) >= 70


# ------------------------------------------------------------------------------------------ phrases
@pytest.mark.parametrize("codec", [1, 2])
def test_phrases_at_position_edges(worlds, codec):
    """Two- and three-term phrases starting at positions 1, 62 .. 65, 127, 128, 65533, 65534; near misses (a gap of 2, one position for two terms, reversed order);
    repeated positions; frequencies 6, 7, 8 and 70 around k_phrase's INLINE_MAX — DocumentsOnly against numpy, on both codecs (the Lucene block walk)."""
    w = worlds("phrase", codec)
    queries = S.phrase_queries(w.c)
    progs, want, hashes = w.want("phrase", queries)
    assert sum(len(x) > 0 for x in want) >= 12
    for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}):
        info = check_docsets(w, queries, progs, want, hashes, opts)
        if not OVERRIDDEN:
            assert info["phrase_queries"] > 0


# ------------------------------------------------------------------------------------------ masked documents
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("which", ["edges", "window"])
def test_masked_boundaries_and_a_whole_window(worlds, which, codec):
    """Exactly the boundary documents masked, then every document of one SPAN_BITS window: DocumentsOnly against numpy (the unmasked result minus the masked set) and
    scored against the oracle with the same set installed — the planner's choice and the bitmap windows forced."""
    w = worlds("main", codec)
    masked = w.c.lists["edges"][0] if which == "edges" else np.arange(S.SPAN_BITS, 2 * S.SPAN_BITS, dtype=np.uint32)
    queries = S.main_queries(w.c)
    progs, want, hashes = w.want("main", queries)
    squeries = S.main_scored_queries(w.c)
    sprogs, swant, _ = w.want("scored", squeries)
    scounts = [int((~np.isin(x, masked)).sum()) for x in swant]
    w.ix.set_masked(masked)
    try:
        for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}):
            check_docsets(w, queries, progs, want, hashes, opts, masked=masked)
        for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}, {"dense_min_postings": 0, "fused": 0}):
            check_scored(w, "scored_" + which, squeries, sprogs, scounts, 10, opts, masked=masked)
    finally:
        w.ix.set_masked(np.zeros(0, np.uint32))
    check_docsets(w, queries[:60], progs[:60], want[:60], hashes[:60], {})  # (cleared again)


# ------------------------------------------------------------------------------------------ tall
@pytest.mark.parametrize("codec", [1, 2])
def test_tall_corpus_docsets(worlds, codec):
    """D = 2^21 + 2^17 + 5: three- and four-byte deltas, a list that lives beyond 2^21 only, `dense_tail3` (a block of more than 64 delta bytes in a list k_and_dense
    takes the static path for) — single lists and every ordered pair as AND / OR / NOT; the planner's choice, the bitmap windows forced, then with every row decoded."""
    w = worlds("tall", codec)
    queries = S.tall_queries(w.c)
    progs, want, hashes = w.want("tall", queries)
    for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}):
        info = check_docsets(w, queries, progs, want, hashes, opts)
        if not OVERRIDDEN and "planes" in opts:
            assert info["dense_queries"] > 50, info
