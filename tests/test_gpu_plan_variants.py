"""GPU tests of the planner and launch options no other test sets (run with -m gpu on an MI355X): a batch's results do not depend on how plan_batch cuts a query into
tasks (phrase_task_div, dense_window_cost), on the kernel and result form a union gets (scatter_bitmap_slack), on the order of sched[] / unit_sched[] (pset_order,
planes_order) or on the streams the matching kernels run on (overlap, overlap_dense_wgs / overlap_cand_wgs) — and tree_max_bytes refuses below the documented need only.

The variants, the corpus / query list / mode / base options each is run on, and the claim that makes each non-vacuous are tests/plan_variants.py's;
tests/test_plan_variants.py shows on the CPU that every claim holds there and fails without the option, that the lists have matches on both sides of the variants'
seams, and that the consumers' batches meet run_matching's fork conditions.  The options are set with test_gpu_parity.options around the batch's creation AND its
runs (the overlap* ones are read by tri_batch_run) and restored by it.

References, none from the engine: structured.Corpus.evaluate (numpy over the postings) for docID sets, counts and FNV hashes; the oracle over the GOOGLE bytes for
scores and the default mode's records, in both codecs; structured.check_topk for top-K (rtol 1e-5; the set-wise rule's 10 % cap is asserted per test from the returned
count and the measured share printed); facet_cases / order_cases / stats_cases / rank_cases for the consumers and the ranker.  Integer results are also compared
with the default-option run of the same world: they must be identical.

One device handle for the file; corpora, worlds, columns and references are module fixtures built once; nothing sleeps, retries or loops on a failure."""
import os

import numpy as np
import pytest

import consumer_tree_cases as CT
import facet_cases as F
import oracle_lib as O
import order_cases as OC
import plan_variants as V
import rank_cases as R
import stats_cases as X
import structured as S
from test_gpu_order import Cols
from test_gpu_parity import options, rich_flat, run_docs_only, run_rich, run_scored
from test_gpu_structured import T, corpora, dev, worlds  # noqa: F401  (T, dev, corpora, worlds: fixtures — this module's own instances)

pytestmark = pytest.mark.gpu
OVERRIDDEN = bool(os.environ.get("TRINITY_TEST_OPTIONS", "").strip())  # (a run-wide option set may force other paths: info() counters are asserted only without one)
RANK_K, RANK_CAP, RANK_ADJ = 10, 3, 4.0
FACET, ORDER, STAT = ("mod7", 7), ("hash", 10, False), ("mod7", 5, "rev")  # facets on one column, an order (K = 10, ascending), one grouped stat


# ------------------------------------------------------------------------------------------ the references, computed once for both codecs
class Refs:
    def __init__(self, corpora):
        self.corpora, self._lists, self._scores, self._rich, self._ora, self._sets = corpora, {}, {}, {}, {}, {}

    def ora(self, name):
        if name not in self._ora:
            self._ora[name] = self.corpora(name).oracle()
        return self._ora[name]

    def get(self, name, key):
        """(queries, programs, numpy docID sets, their FNV hashes) of plan_variants.QUERY_LISTS[key] over a corpus"""
        if (name, key) not in self._lists:
            c = self.corpora(name)
            queries = V.QUERY_LISTS[key](c)
            progs = S.programs(queries)
            sets = [self.evaluate(name, c, p) for p in progs]
            self._lists[name, key] = (queries, progs, sets, [O.fnv1a_docs(s) for s in sets])
        return self._lists[name, key]

    def evaluate(self, name, c, prog):
        """(a program that several lists hold — a phrase over the stream corpus takes numpy seconds — is evaluated once)"""
        k = (name, prog.tobytes())
        if k not in self._sets:
            self._sets[k] = c.evaluate(prog)
        return self._sets[k]

    def scores(self, name, key):
        """the oracle's (docs, BM25 scores) of the list"""
        if (name, key) not in self._scores:
            self._scores[name, key] = [self.ora(name).exec(p, O.FLAG_ACCUM_SCORE) for p in self.get(name, key)[1]]
        return self._scores[name, key]

    def rich(self, name, key):
        """the oracle's default-mode answers (docs, flat records, matched terms, hits) of the list"""
        if (name, key) not in self._rich:
            self._rich[name, key] = [self.ora(name).exec_rich(p) for p in self.get(name, key)[1]]
        return self._rich[name, key]


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
    for c in made.values():  # (a column is destroyed before its index)
        c.close()


@pytest.fixture(scope="module")
def defaults():
    """results of the default-option runs, kept for the comparisons with the variants' runs"""
    return {}


@pytest.fixture(scope="module")
def shares():
    """(variant, codec) -> [set-wise comparisons, scored cases]"""
    made = {}
    yield made
    for (name, codec), (n, cases) in sorted(made.items()):
        print(f"[plan-variants] set-wise share {name} codec {codec}: {n} of {cases} ({100.0 * n / max(1, cases):.1f} %)")


# ------------------------------------------------------------------------------------------ runs
def docs_run(w, progs, opts):
    """One DocumentsOnly batch created and run under an option set -> (flat docIDs, offsets, hashes, counts, mixed words, mixed offsets, forms, info)."""
    with options(w.dev, **opts):
        b = w.T.Batch(w.ix, progs, w.T.FLAG_DOCUMENTS_ONLY)
        try:
            b.run()
            b.sync()
            flat, offs = b.docsets()
            mflat, moffs, forms = b.docsets_mixed()
            return flat, offs, b.docset_hashes(), b.counts(), mflat, moffs, forms, b.info()
        finally:
            b.close()


def check_docs(w, ref, opts, base=None, tag=None):
    """Sets, counts and hashes against numpy; every bitmap-form result word by word; -> the run (for the comparison with the default run)."""
    queries, progs, want, hashes = ref
    got = docs_run(w, progs, dict(base or {}, **opts))
    flat, offs, hs, counts, mflat, moffs, forms, info = got
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist(), (tag, opts)
    for i, (text, mn) in enumerate(queries):
        assert int(counts[i]) == len(want[i]) and int(hs[i]) == hashes[i], (tag, opts, text, int(counts[i]), len(want[i]))
        assert np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], want[i]), (tag, opts, text)
        if forms[i]:  # bit j of word i is document 32 i + j and nothing else: no bit for docID 0, none past docs_cnt
            words = mflat[int(moffs[i]) : int(moffs[i + 1])]
            docs = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little"))
            assert docs.size == 0 or (docs[0] >= 1 and docs[-1] <= w.c.docs_cnt), (tag, opts, text, docs[:1], docs[-1:])
            assert np.array_equal(docs.astype(np.uint32), want[i]), (tag, opts, text, docs.size, len(want[i]))
    assert info["matches"] == sum(len(x) for x in want) and info["unsupported_queries"] == 0, (tag, opts)
    return got


def same_docs(a, b):
    """Two runs' expanded sets, counts and hashes, bit for bit (the forms may differ: scatter_bitmap_slack changes them)."""
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def check_scored(w, ref, scores, k, opts, tag):
    """One scored top-K batch under an option set: match counts against numpy, top-K against the oracle -> (set-wise comparisons, cases)."""
    queries, progs, want, _ = ref
    with options(w.dev, **opts):
        d, s, c, counts = run_scored(w, progs, k)
    setwise = 0
    for i, (text, mn) in enumerate(queries):
        docs, sc = scores[i]
        assert int(counts[i]) == len(want[i]) == len(docs), (tag, opts, k, text, int(counts[i]), len(want[i]))
        assert int(c[i]) == min(k, len(docs)), (tag, opts, k, text)
        setwise += S.check_topk(d[i, : int(c[i])], s[i, : int(c[i])], docs, sc, k, w.ora, (tag, opts, k, text))
    return setwise, len(queries)


def check_rich(w, ref, rich, opts, tag):
    """The default mode's matched terms, frequencies and positions against the oracle's records."""
    queries, progs, want, _ = ref
    with options(w.dev, **opts):
        got = run_rich(w, progs)
    for (text, mn), exp, (wdocs, wflat, tt, ht), (docs, terms, present, freq, pos) in zip(queries, want, rich, got):
        assert np.array_equal(docs, exp) and np.array_equal(docs, wdocs), (tag, opts, text, len(docs), len(exp))
        assert int(freq.sum()) == ht and int(sum(bin(int(x)).count("1") for x in present)) == tt, (tag, opts, text)
        assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), (tag, opts, text)


def add_share(shares, name, codec, setwise, cases):
    at = shares.setdefault((name, codec), [0, 0])
    at[0], at[1] = at[0] + setwise, at[1] + cases


def fork_condition(info):
    """run_matching puts k_and on the second stream (options overlap*) when the batch holds window or plane-set queries AND candidate-tile queries."""
    return info["dense_queries"] + info["pset_queries"] > 0 and info["cand_queries"] > 0


# ------------------------------------------------------------------------------------------ DocumentsOnly, every variant
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", V.PLAN_VARIANTS + V.LAUNCH_VARIANTS)
def test_docsets_do_not_depend_on_the_variant(worlds, refs, defaults, name, codec):
    """The full main catalogue and the scatter unions, D = 4 x 131072 + 37: sets, counts and hashes equal numpy's and, bit for bit, the default-option run's; every
    bitmap-form result word by word.  The scatter variants also under plane_div = 4096, where unions sit on both sides of the rule at every slack."""
    w = worlds("main", codec)
    ref = refs.get("main", "main+unions")
    if ("main", codec) not in defaults:
        defaults["main", codec] = check_docs(w, ref, {}, tag="default")
    base = defaults["main", codec]
    got = check_docs(w, ref, V.OPTIONS[name], tag=name)
    assert same_docs(got, base), name
    info, info0 = got[7], base[7]
    if name.startswith("scatter"):
        small = refs.get("main", "unions")
        key = ("unions", codec)
        if key not in defaults:
            defaults[key] = check_docs(w, small, {}, base={"plane_div": V.SCATTER_PLANE_DIV}, tag="default")
        g2 = check_docs(w, small, V.OPTIONS[name], base={"plane_div": V.SCATTER_PLANE_DIV}, tag=name)
        assert same_docs(g2, defaults[key]), name
        if not OVERRIDDEN:
            more = V.OPTIONS[name]["scatter_bitmap_slack"] > 4
            for a, b in ((got, base), (g2, defaults[key])):  # the forms flipped in the variant's direction only
                gained, lost = int(((a[6] == 1) & (b[6] == 0)).sum()), int(((a[6] == 0) & (b[6] == 1)).sum())
                assert (gained > 0 and lost == 0) if more else (lost > 0 and gained == 0), (name, gained, lost)
    elif not OVERRIDDEN:
        assert np.array_equal(got[6], base[6]), name  # (no other variant changes a result's form)
        assert info["bitmap_queries"] == info0["bitmap_queries"] > 0
    if not OVERRIDDEN:
        assert fork_condition(info) and info["pset_queries"] > 0 and info["dense_queries"] > 0, info


# ------------------------------------------------------------------------------------------ phrases
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", V.PHRASE_VARIANTS)
def test_phrase_corpus_in_all_three_modes(worlds, refs, shares, name, codec):
    """Phrases at the position edges under the phrase_task_div, stream-layout and combined variants: DocumentsOnly against numpy, scored top-K at K = 10 and 256
    against the oracle, the default mode's matched terms, frequencies and positions against the oracle."""
    w = worlds("phrase", codec)
    ref = refs.get("phrase", "phrase")
    opts = V.OPTIONS[name]
    for base in ({}, {"dense_min_postings": 0}, V.ALL_WINDOWS):
        got = check_docs(w, ref, opts, base=base, tag=name)
        if not OVERRIDDEN:
            assert got[7]["phrase_queries"] > 0
    setwise = cases = 0
    for k in (10, 256):
        n, m = check_scored(w, ref, refs.scores("phrase", "phrase"), k, opts, name)
        setwise, cases = setwise + n, cases + m
    add_share(shares, name, codec, setwise, cases)
    assert setwise <= cases // 10, (setwise, cases)
    check_rich(w, ref, refs.rich("phrase", "phrase"), opts, name)


STREAM_DOCS_CASES = [(n, "mix") for n in V.PHRASE_VARIANTS] + [(n, "windows") for n in V.PHRASE_VARIANTS if n not in V.LAUNCH_VARIANTS]
STREAM_BASES = {"mix": V.PHRASE_MIX, "windows": V.ALL_WINDOWS}
PHRASE_CUTS = [n for n in V.PHRASE_VARIANTS if n not in V.LAUNCH_VARIANTS]


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name,bname", STREAM_DOCS_CASES)
def test_phrase_tasks_of_several_windows_and_tiles(worlds, refs, defaults, name, bname, codec):
    """The stream corpus (three windows, leads of up to five tiles).  `mix`: plan_variants.PHRASE_MIX, where one plan holds phrase queries as plane-set windows, bitmap
    windows and candidate tiles and the phrase_task_div variants really cut them 1 x, 2 x and 8 x; `windows`: every phrase query as bitmap windows, seams at the window
    boundaries the head terms all hold documents on.  DocumentsOnly against numpy and, bit for bit, the default cut's run.  (k_phrase's span is its longest task: a batch
    of this corpus — up to 300 hits a document — runs about a second at the default cut and two uncut; each case is one batch.)"""
    w = worlds("stream", codec)
    ref = refs.get("stream", "stream")
    base = STREAM_BASES[bname]
    key = ("stream", bname, codec)
    if key not in defaults:
        defaults[key] = check_docs(w, ref, {}, base=base, tag="default")
    got = check_docs(w, ref, V.OPTIONS[name], base=base, tag=name)
    assert same_docs(got, defaults[key]), (name, bname)
    if not OVERRIDDEN and bname == "mix":
        assert fork_condition(got[7]) and got[7]["phrase_queries"] > 0, got[7]


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", PHRASE_CUTS)
def test_phrase_tasks_of_several_windows_scored(worlds, refs, shares, name, codec):
    """... the same plan scored, top-K at K = 10 against the oracle."""
    w = worlds("stream", codec)
    setwise, cases = check_scored(w, refs.get("stream", "stream"), refs.scores("stream", "stream"), 10, dict(V.PHRASE_MIX, **V.OPTIONS[name]), name)
    add_share(shares, name, codec, setwise, cases)
    assert setwise <= cases // 10, (setwise, cases)


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", PHRASE_CUTS)
def test_phrase_tasks_of_several_windows_in_the_default_mode(worlds, refs, name, codec):
    """... and its phrase queries in the default mode: matched terms, frequencies and positions against the oracle (k_rich walks the same tasks)."""
    w = worlds("stream", codec)
    check_rich(w, refs.get("stream", "stream_phrases"), refs.rich("stream", "stream_phrases"), dict(V.PHRASE_MIX, **V.OPTIONS[name]), name)


# ------------------------------------------------------------------------------------------ scored
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", V.SCORED_VARIANTS)
def test_scored_topk_does_not_depend_on_the_order_or_the_streams(worlds, refs, shares, name, codec):
    """freq_queries (K = 10 and 256) and main_scored_queries (K = 10) under the scored option sets that reach k_planes, both word widths of k_fused and
    match-then-score (k_psets + k_and + k_and_dense): counts against numpy, top-K through check_topk.  A k_planes query's ranges share one threshold: a wrong order shows
    as a lost document."""
    opts = V.OPTIONS[name]
    setwise = cases = 0
    for corpus, key, ks in (("freq", "freq", (10, 256)), ("main", "main_scored", (10,))):
        w = worlds(corpus, codec)
        ref = refs.get(corpus, key)
        for base in V.SCORED_BASES:
            for k in ks:
                n, m = check_scored(w, ref, refs.scores(corpus, key), k, dict(base, **opts), name)
                setwise, cases = setwise + n, cases + m
    add_share(shares, name, codec, setwise, cases)
    assert setwise <= cases // 10, (setwise, cases)


# ------------------------------------------------------------------------------------------ tall
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", V.TALL_VARIANTS)
def test_tall_corpus_one_task_over_all_windows_and_one_window_a_task(worlds, refs, defaults, shares, name, codec):
    """D = 2^21 + 2^17 + 5, the corpus where a query spans 17 windows: dense_window_cost = 0 (a union of rare lists is ONE task over all of them), 1 << 20 (every
    window a task of its own, on lists that end inside the last window) and phrase_task_div = 1 (the corpus holds no phrase: the cut a large batch gets must leave
    it alone) — DocumentsOnly, the planner's choice and every row decoded, and scored at K = 10."""
    w = worlds("tall", codec)
    ref = refs.get("tall", "tall")
    opts = V.OPTIONS[name]
    for bname, base in (("", {}), ("windows", V.ALL_WINDOWS)):
        key = ("tall", bname, codec)
        if key not in defaults:
            defaults[key] = check_docs(w, ref, {}, base=base, tag="default")
        got = check_docs(w, ref, opts, base=base, tag=name)
        assert same_docs(got, defaults[key]), (name, bname)
        if not OVERRIDDEN and bname:
            assert got[7]["dense_queries"] > 50, got[7]
    # scored as match-then-score: the bases under which the one-pass kernels run hold no window tasks for the option to cut
    setwise, cases = check_scored(w, refs.get("tall", "tall_scored"), refs.scores("tall", "tall_scored"), 10, dict(V.MATCH_THEN_SCORE, **opts), name)
    add_share(shares, name, codec, setwise, cases)
    assert setwise <= cases // 10, (setwise, cases)


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", ["dense_window_cost=0", "dense_window_cost=1M"])
def test_dense_window_cost_in_the_default_mode(worlds, refs, name, codec):
    """k_rich walks the same TASK_DENSE tasks: the tall corpus' rare-list unions and conjunctions as one task over 17 .. 18 windows and as a task a window, and —
    1 << 20, which cuts the main corpus' five windows too — the main corpus' default-mode list: matched terms, frequencies and positions against the oracle."""
    for corpus, key in [c[:2] for c in V.CLAIM_CASES[name] if c[2] == "rich"]:
        w = worlds(corpus, codec)
        ref = refs.get(corpus, key)
        with options(w.dev, **V.OPTIONS[name]):
            b = w.T.Batch(w.ix, ref[1], w.T.FLAG_MATCHED_TERMS)
            info = b.info()
            b.close()
        if not OVERRIDDEN:
            assert info["dense_queries"] > 0, info
        check_rich(w, ref, refs.rich(corpus, key), V.OPTIONS[name], name)


# ------------------------------------------------------------------------------------------ the consumers and the ranker under the stream layouts
def set_consumers(b, cl):
    b.set_facets([(cl.get(FACET[0]), FACET[1])])
    b.set_order(cl.get(ORDER[0]), ORDER[1], ORDER[2])
    b.set_stats([(cl.get(STAT[0]), STAT[1], cl.get(STAT[2]))])


def consumer_rows(sets, values):
    return F.facet_rows(sets, values[FACET[0]], FACET[1]), OC.rows(sets, values[ORDER[0]], ORDER[1], ORDER[2]), X.stats_rows(sets, values[STAT[0]], STAT[1], values[STAT[2]])


def check_consumers(b, sets, hashes, rows, tag):
    """After sync(): counts, hashes, facet rows, ordered rows and stats of a batch against the expected ones — integer equality throughout."""
    assert b.counts().tolist() == [len(s) for s in sets] and (hashes is None or b.docset_hashes().tolist() == hashes), tag
    f, o, st = rows
    got = b.facets(0)
    assert got.dtype == np.uint32 and np.array_equal(got, f), (tag, "facets")
    for g, x, what in zip(b.ordered(), o, ("docids", "values", "counts")):
        assert g.dtype == np.uint32 and np.array_equal(g, x), (tag, "order", what)
    assert X.same(b.stats(0), st), (tag, "stats")


@pytest.fixture(scope="module")
def consumer_refs(refs, corpora):
    made = {}

    def get(key):
        if key not in made:
            ref = refs.get("main", key)
            made[key] = (ref, consumer_rows(ref[2], OC.columns(corpora("main").D)))
        return made[key]

    return get


@pytest.mark.parametrize("codec", [1, 2])
def test_consumers_read_the_results_after_the_join(T, worlds, cols, consumer_refs, codec):
    """One DocumentsOnly batch of window, plane-set and candidate-tile queries with facets, an order and a grouped stat set at once, created and run under the four
    stream layouts: the consumers and the delivery read d_out / d_counts only after k_and's stream has joined."""
    w, cl = worlds("main", codec), cols("main", codec)
    (queries, progs, sets, hashes), rows = consumer_refs("consumers")
    for layout in V.LAYOUTS:
        with options(w.dev, **layout):
            b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
            try:
                if not OVERRIDDEN:
                    assert fork_condition(b.info()), b.info()
                set_consumers(b, cl)
                for rep in range(2):  # (the second run: tickets, counts and the consumers' rows are reset behind the same fork)
                    b.run()
                    b.sync()
                    check_consumers(b, sets, hashes, rows, (layout, rep))
                flat, offs = b.docsets()
                assert all(np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], sets[i]) for i in range(len(sets))), layout
            finally:
                b.close()


@pytest.mark.parametrize("codec", [1, 2])
def test_default_mode_ranker_and_consumers_under_the_stream_layouts(T, worlds, cols, refs, codec):
    """The default mode with a ranker, facets, an order and a grouped stat on one batch of bitmap-window and candidate-tile queries, under the four layouts: the ranked
    lists equal rank_cases' restatement bit for bit, the consumers' rows the numpy ones, the matched-terms report the oracle's."""
    w, cl = worlds("main", codec), cols("main", codec)
    ref = refs.get("main", "rich")
    queries, progs, sets, hashes = ref
    rich = refs.rich("main", "rich")
    rows = consumer_rows(sets, cl.values)
    w3 = lambda k: 1 + k % 3  # noqa: E731
    weights = R.token_weights(progs, w3)
    want = [R.rows(R.records(r[1]), p, RANK_CAP, RANK_ADJ, R.token_weights([p], w3))[:RANK_K] for r, p in zip(rich, progs)]
    assert any(x[2] for rws in want for x in rws)  # (some listed document scores an adjacent pair: the ranker read positions, not only frequencies)
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tolist()  # noqa: E731
    for layout in V.LAYOUTS:
        with options(w.dev, **layout):
            b = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS)
            try:
                if not OVERRIDDEN:
                    assert fork_condition(b.info()), b.info()
                b.set_ranker(RANK_K, RANK_CAP, RANK_ADJ, weights)
                set_consumers(b, cl)
                b.run()
                b.sync()
                check_consumers(b, sets, None, rows, layout)
                d, s, c = b.ranked()
                for qi, rws in enumerate(want):
                    n = len(rws)
                    assert int(c[qi]) == n and d[qi, :n].tolist() == [x[0] for x in rws] and bits(s[qi, :n]) == bits([x[1] for x in rws]), (layout, queries[qi][0])
                    assert not d[qi, n:].any() and not s[qi, n:].any(), (layout, queries[qi][0])
                counts = b.counts()
                for qi, ((text, mn), (wdocs, wflat, tt, ht)) in enumerate(zip(queries, rich)):
                    docs = b.docset(qi, int(counts[qi]))
                    terms, present, freq, pos = b.matched_terms(qi, int(counts[qi]))
                    assert np.array_equal(docs, wdocs) and np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), (layout, text)
            finally:
                b.close()


@pytest.mark.parametrize("codec", [1, 2])
def test_forked_prep_and_forked_k_and_share_the_fork_and_join_events(T, worlds, cols, consumer_refs, codec):
    """Batches that hold scatter unions beside bitmap-window queries AND candidate tiles: k_psets_prep forks onto the second stream in the default layout, k_and in the
    others, over the device's one pair of fork / join events.  Two such batches run back to back without a sync between, under each layout — and once with the first
    in the default layout and the second under overlap = 1 —, then both are synced and checked, consumers included."""
    w, cl = worlds("main", codec), cols("main", codec)
    (queries, progs, sets, hashes), rows = consumer_refs("consumers+scatter")
    back = list(range(len(progs)))[::-1]
    rprogs, rsets, rhashes = [progs[i] for i in back], [sets[i] for i in back], [hashes[i] for i in back]
    rrows = consumer_rows(rsets, cl.values)
    a = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    b = T.Batch(w.ix, rprogs, T.FLAG_DOCUMENTS_ONLY)
    try:
        if not OVERRIDDEN:
            assert fork_condition(a.info()) and fork_condition(b.info()) and a.info()["bitmap_queries"] >= 4, a.info()
        set_consumers(a, cl)
        set_consumers(b, cl)
        for first, second in [(x, x) for x in V.LAYOUTS] + [({}, {"overlap": 1}), ({"overlap": 1}, {})]:
            with options(w.dev, **first):
                a.run()
            with options(w.dev, **second):
                b.run()
            a.sync()
            b.sync()
            check_consumers(a, sets, hashes, rows, (first, second, "a"))
            check_consumers(b, rsets, rhashes, rrows, (first, second, "b"))
            for x, ss in ((a, sets), (b, rsets)):
                flat, offs = x.docsets()
                assert all(np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], ss[i]) for i in range(len(ss))), (first, second)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ tree_max_bytes
@pytest.mark.parametrize("codec", [1, 2])
def test_tree_max_bytes_on_the_device(T, dev, worlds, corpora, refs, codec):
    """A create one byte below the documented need fails with TRI_ERR_NOMEM and leaves the pool's bytes in use where they were; a create at exactly the need runs and
    answers the oracle."""
    w = worlds("stream", codec)
    c = corpora("stream")
    queries = CT.stream_list(c)
    progs = S.programs(queries)
    plain = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    need = plain.info()["tree_scratch_bytes"]
    trees = plain.info()["tree_queries"]
    plain.close()
    if not OVERRIDDEN:  # the documented formula over the host plan's own counters
        hi = c.host_index(codec)
        p = V.host_plan(hi, queries, "docs", {})
        assert need == (p.s["n_tree_terms"] * V.PL_PLANES + p.s["n_tree_hidden"] + p.s["tree_queries"]) * p.s["plw"] * 4 and trees == p.s["tree_queries"] >= 5, (need, p.s)
        p.close()
        hi.close()
    assert need > 0
    dev.sync()
    before = dev.memory()["pool_in_use_bytes"]
    with options(dev, tree_max_bytes=need - 1):
        with pytest.raises(T.engine.TrinityError, match=r"rc=-5: .*tree_max_bytes"):  # TRI_ERR_NOMEM
            T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    dev.sync()
    assert dev.memory()["pool_in_use_bytes"] == before
    ora = refs.ora("stream")
    with options(dev, tree_max_bytes=need):
        sets, _, info = run_docs_only(w, progs)
    assert info["tree_scratch_bytes"] == need and info["unsupported_queries"] == 0
    for (text, mn), p, got in zip(queries, progs, sets):
        assert np.array_equal(got, ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0]), text
