"""GPU tests of the wide tree kernels AT THE RECORD'S LIMITS and the chunk edges (run with -m gpu on an MI355X): k_tree_eval_wide / k_tree_leaves_wide
(csrc/k_tree_wide.hpp) and the fold they share with the percolator (csrc/tree_fold.hpp) on the catalogue of tests/wide_tree_cases.py — a 1024-node OR (all 32
words of bits[][], the root on bit 31 of the last), matchsomes of 300 and 1020 children at thresholds on both sides of a byte and of the ninth and tenth counter
plane, a 64-level alternation and a chain of nested matchsomes that use every word of stk[64] and cnt[64], a union whose matches fill its region exactly, wide
excluded and optional sides — over a corpus with a busy chunk, a chunk that holds its first 65 documents only, an empty chunk, a chunk with a head and a tail, a
last chunk of two words and three chunks of row padding behind it.  tests/test_wide_tree_cases.py shows on the CPU that the planner lowers every case as the
record meant, that numpy, the oracle and a replay of the fold agree on it, and that four deliberately wrong folds (an 8-bit threshold, eight counter planes, a
32-word stack, 64 nodes) each change a named case's answer.

References: docID sets, counts and hashes — structured.Corpus.evaluate (numpy over the postings arrays); scores and the default mode's records — the oracle over
the GOOGLE bytes of the same postings, for the LUCENE-coded upload too.  Scores at structured.RTOL (1e-5); top-10 through structured.check_topk: measured on the
oracle (tests/test_wide_tree_cases.py::test_score_gap_condition), 0 of the 19 scored (case, similarity) runs fall under its set-wise rule (bound: 10 %), the
smallest relative gap between distinct scores within ranks 1 .. 11 is 2.7e-3.

One device handle for the file, one upload per codec; every batch and filter is closed by the test that opened it; nothing retries."""
import os

import numpy as np
import pytest

import oracle_lib as O
import structured as S
import wide_tree_cases as W
from test_gpu_parity import options, rich_flat
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
OVERRIDDEN = bool(os.environ.get("TRINITY_TEST_OPTIONS", "").strip())  # (a run-wide option set may force other paths: info() counters are asserted only without one)
NONE = np.zeros(0, np.uint32)


class Catalogue:
    """The corpus, its oracle and the reference answers, computed once for both codecs."""

    def __init__(self):
        self.c = W.corpus()
        self.ora = self.c.oracle()
        self.cases, self.left = W.cases(), W.left_out()
        self.names = W.NAMES + list(self.left)
        self.progs = [self.cases[n][0] for n in W.NAMES] + [p for p, _, _ in self.left.values()]
        self.status = [0] * len(W.NAMES) + [st for _, st, _ in self.left.values()]
        self.mask, self.drop = W.chunk_edge_mask(), W.filter_drop()
        self.both = np.union1d(self.mask, self.drop).astype(np.uint32)
        self._sets, self._scores, self._rich = {}, {}, {}

    def docs(self, name, key="plain"):
        """evaluate() of a case without `plain` / `masked` / `both` (the mask and the filter's documents)."""
        if (name, key) not in self._sets:
            gone = {"plain": None, "masked": self.mask, "both": self.both}[key]
            self._sets[name, key] = self.c.evaluate(self.cases[name][0], masked=gone)
        return self._sets[name, key]

    def scores(self, name, sim):
        if (name, sim) not in self._scores:
            self.ora.set_similarity(sim)
            try:
                self._scores[name, sim] = self.ora.exec(self.cases[name][0], O.FLAG_ACCUM_SCORE)
            finally:
                self.ora.set_similarity(O.SIM_BM25)
        return self._scores[name, sim]

    def rich(self, name):
        if name not in self._rich:
            self._rich[name] = self.ora.exec_rich(self.cases[name][0])
        return self._rich[name]


@pytest.fixture(scope="module")
def cat():
    return Catalogue()


@pytest.fixture(scope="module")
def indexes(T, dev, cat):
    made = {}

    def get(codec):
        if codec not in made:
            made[codec] = cat.c.upload(T, dev, codec)
        return made[codec]

    yield get
    for ix in made.values():
        ix.close()


def docs_only_batch(T, dev, cat, ix):
    with options(dev, **W.WIDE):
        b = T.Batch(ix, cat.progs, T.FLAG_DOCUMENTS_ONLY, allow_unsupported=True)
    assert b.query_status().tolist() == cat.status, b.query_status().tolist()  # 0 for every case, -3 for deep65
    info = b.info()
    if not OVERRIDDEN:  # (opt_wide is a conjunction with an optional group to the planner: every other lowered case is a tree query)
        assert info["tree_queries"] == len(W.TREE_NAMES) == len(W.NAMES) - 1 and info["unsupported_queries"] == len(cat.left), info
    return b


def check_docs_only(b, cat, key_of, tag):
    counts, hashes = b.counts(), b.docset_hashes()
    for i, name in enumerate(cat.names):
        want = cat.docs(name, key_of(i)) if cat.status[i] == 0 else NONE
        assert int(counts[i]) == len(want), (tag, name, int(counts[i]), len(want))
        got = b.docset(i, len(want))
        assert np.array_equal(got, want), (tag, name, np.setxor1d(got, want)[:8])
        if cat.status[i] == 0:
            assert int(hashes[i]) == O.fnv1a_docs(want), (tag, name)


# ------------------------------------------------------------------------------------------ DocumentsOnly
@pytest.mark.parametrize("codec", [1, 2])
def test_docsets_are_exact_plain_masked_and_filtered(T, dev, cat, indexes, codec):
    """Every case in ONE batch: statuses, counts, docsets and docset hashes against numpy — plain; with the chunk-edge documents {1, 31, 32, C - 1, C, C + 1, 3C,
    4C - 1, 4C, D} and every seventh active document masked; and with a TRI_FILTER_DROP filter on every second query on top of the mask.  allP's matches fill its
    region exactly (out_cap == matches: k_tree_expand's last store) while the mask is off."""
    ix = indexes(codec)
    flt = None
    try:
        for tag, mk, filtered in (("plain", NONE, False), ("masked", cat.mask, False), ("masked+filter", cat.mask, True)):
            ix.set_masked(mk)
            b = docs_only_batch(T, dev, cat, ix)
            try:
                if filtered:
                    flt = T.Filter(ix, cat.drop)
                    b.set_filters([flt], [0 if i % 2 == 1 else T.engine.NO_FILTER for i in range(len(cat.progs))])
                b.run()
                b.sync()
                check_docs_only(b, cat, lambda i: "plain" if tag == "plain" else "both" if filtered and i % 2 == 1 else "masked", (codec, tag))
            finally:
                b.close()
        assert len(cat.docs("allP")) == len(W.active_docs()) > len(cat.docs("allP", "masked")) > len(cat.docs("allP", "both")) > 0
    finally:
        if flt is not None:
            flt.close()
        ix.set_masked(NONE)


@pytest.mark.parametrize("codec", [1, 2])
def test_a_second_run_answers_as_the_first(T, dev, cat, indexes, codec):
    """The chunk counts and the match bitmaps are rebuilt per run — over the empty chunk and the padding chunks too."""
    b = docs_only_batch(T, dev, cat, indexes(codec))
    try:
        for rep in range(2):
            b.run()
            b.sync()
            check_docs_only(b, cat, lambda i: "plain", (codec, "run", rep))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ AccumulatedScore
@pytest.mark.parametrize("sim", ["bm25", "tfidf"])
@pytest.mark.parametrize("codec", [1, 2])
def test_scores_match_the_oracle(T, dev, cat, indexes, codec, sim):
    """Top-10 (structured.check_topk) and the full stream (topk = 0: docIDs exact, every score at RTOL) — BM25 on every case, TF-IDF on or1023 and some1020_511.  A
    document with h = 60 sums 1023 leaves' scores from all 32 node words; the ladder's frequencies 0 and 16 go through k_tree_leaves_wide's lookup."""
    simid = {"bm25": O.SIM_BM25, "tfidf": O.SIM_TFIDF}[sim]
    names = W.NAMES if sim == "bm25" else list(W.SCORED_TFIDF)
    progs = [cat.cases[n][0] for n in names]
    ix = indexes(codec)
    for k in (10, 0):
        with options(dev, **W.WIDE):
            b = T.Batch(ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=k, similarity=simid)
        try:
            assert not b.query_status().any()
            b.run()
            b.sync()
            counts = b.counts()
            tk = b.topk_results() if k else None
            for i, name in enumerate(names):
                docs, scores = cat.scores(name, simid)
                assert np.array_equal(docs, cat.docs(name)) and int(counts[i]) == len(docs), (codec, sim, k, name, int(counts[i]), len(docs))
                if k:
                    n = int(tk[2][i])
                    assert n == min(k, len(docs)), (codec, sim, name)
                    S.check_topk(tk[0][i, :n], tk[1][i, :n], docs, scores, k, cat.ora, (codec, sim, name))
                else:
                    assert np.array_equal(b.docset(i, len(docs)), docs), (codec, sim, name)
                    np.testing.assert_allclose(b.scores(i, len(docs)), scores, rtol=S.RTOL, atol=0, err_msg=str((codec, sim, name)))
        finally:
            b.close()


# ------------------------------------------------------------------------------------------ the default mode
@pytest.mark.parametrize("codec", [1, 2])
def test_matched_terms_match_the_oracle(T, dev, cat, indexes, codec):
    """The flat record stream (doc, matched terms, per term its frequency and positions) against oracle.exec_rich: deep64 at the default rich_max_terms (12 reportable
    terms, cnt[] 64 deep); or1023 and some300_260 at rich_max_terms = 64 (60 reportable terms: rep_hi filled from records of 1024 and 301 nodes)."""
    ix = indexes(codec)
    for names, opts in ((W.RICH_DEFAULT, W.WIDE), (W.RICH_WIDE, dict(W.WIDE, rich_max_terms=64))):
        with options(dev, **opts):
            b = T.Batch(ix, [cat.cases[n][0] for n in names], T.FLAG_MATCHED_TERMS)
        try:
            assert not b.query_status().any() and (OVERRIDDEN or b.info()["tree_queries"] == len(names))
            b.run()
            b.sync()
            counts = b.counts()
            for j, name in enumerate(names):
                wdocs, wflat, tt, ht = cat.rich(name)
                docs = b.docset(j, int(counts[j]))
                terms, present, freq, pos = b.matched_terms(j, len(docs))
                assert np.array_equal(docs, wdocs) and np.array_equal(docs, cat.docs(name)), (codec, name)
                assert len(terms) == (12 if name in W.RICH_DEFAULT else 60), (codec, name, len(terms))
                assert int(freq.sum()) == ht and int(sum(bin(int(x)).count("1") for x in present)) == tt, (codec, name)
                assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), (codec, name)
        finally:
            b.close()
