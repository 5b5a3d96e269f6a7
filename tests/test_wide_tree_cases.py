"""CPU checks of the wide-tree catalogue (tests/wide_tree_cases.py) the GPU file tests/test_gpu_wide_tree_limits.py and the percolator's
test_the_wide_fold_at_its_limits read: the planner lowers every named case as the wide record the table says (node count, stack words, depth, the root's
planes / threshold / children), three independent answers agree on every case — numpy over the postings arrays, the oracle's iterator trees, a replay of
csrc/tree_fold.hpp over the planner's record —, the matchsomes equal their closed form, the deep cases fill all 64 stack words, each of four deliberately
wrong folds is told apart by the case named for it, and the oracle's scores are the sums over the leaves k_tree_leaves_wide's rule reaches.

The score-gap condition (test_score_gap_condition prints it): of the 19 scored (case, similarity) runs at K = 10, 0 fall under structured.check_topk's
set-wise rule (bound: 10 %); the smallest relative gap between distinct oracle scores within ranks 1 .. 11 is 2.7e-3."""
import numpy as np
import pytest

import oracle_lib as O
import perc_cases as PC
import structured as S
import trinity_amd as T
import wide_tree_cases as W
from trinity_amd import hostplan as HP


class Ctx:
    def __init__(self):
        T.build.build_host()
        self.c = W.corpus()
        self.ora = self.c.oracle()
        self.act = W.active_docs()
        self.cases, self.left = W.cases(), W.left_out()
        self.progs = [p for p, _, _ in self.cases.values()] + [p for p, _, _ in self.left.values()]
        self.leaf = {t: W.bits_of(self.c.lists[n][0], self.act) for t, n in enumerate(self.c.names)}
        self.plans, self._want = {}, {}

    def plan(self, codec):
        if codec not in self.plans:
            hi = self.c.host_index(codec)
            self.plans[codec] = (HP.HostPlan(hi, self.progs, T.FLAG_DOCUMENTS_ONLY, options=W.WIDE), hi)
        return self.plans[codec][0]

    def record(self, name, codec=1):
        p = self.plan(codec)
        return p.tree_nodes_wide(int(p.slot_of_query[W.NAMES.index(name)]))

    def want(self, name):
        if name not in self._want:
            self._want[name] = self.c.evaluate(self.cases[name][0])
        return self._want[name]

    def close(self):
        for p, hi in self.plans.values():
            p.close()
            hi.close()


@pytest.fixture(scope="module")
def w():
    x = Ctx()
    yield x
    x.close()


def test_the_corpus_is_what_the_catalogue_says(w):
    c, act = w.c, w.act
    assert c.D == W.D == 4 * W.C + 37 and W.C == 65536 and len(act) == 4392
    chunks = np.unique(act // W.C).tolist()
    assert chunks == [0, 1, 3, 4] and (act[act // W.C == 1] - W.C).max() == 64 and act[-1] == W.D and (W.D >> 5) - 4 * S.TREE_CHUNK_WORDS == 1  # (chunk 4: words 0 and 1)
    held = np.zeros(W.D + 1, dtype=np.int64)
    for i in range(W.NLADDER):
        held[c.lists[f"L{i}"][0]] += 1
    assert np.array_equal(held[act], W.h_of(act)) and set(W.h_of(act).tolist()) == set(range(61)) and held.sum() == sum(c.lists[f"L{i}"][0].size for i in range(W.NLADDER))
    assert {int(f) for i in range(W.NLADDER) for f in c.lists[f"L{i}"][1]} == set(W.LADDER_FREQS) and 0 in W.LADDER_FREQS and S.PL_NESTED in W.LADDER_FREQS and max(W.LADDER_FREQS) > S.PL_NESTED
    parts = np.concatenate([c.lists[f"P{i}"][0] for i in range(W.NPART)])
    assert np.array_equal(np.sort(parts), act) and all(np.all(c.lists[f"P{i}"][0] % 64 == i) for i in range(W.NPART))
    mask = W.chunk_edge_mask()
    assert np.isin([1, 31, 32, W.C - 1, W.C, W.C + 1, 3 * W.C, 4 * W.C - 1, 4 * W.C, W.D], mask).all() and np.isin(mask, act).all() and np.isin(W.filter_drop(), act).all()


@pytest.mark.parametrize("codec", [1, 2])
def test_every_case_is_lowered_as_the_table_says(w, codec):
    """tree_max_nodes = 1024: status 0 and a WIDE record with exactly the table's header [nnodes, kind, stack words, depth] and root cbits / thr / nkids; deep65 is left
    out for its stack; allP's region is exactly its matches; opt_wide is lowered, but not as a tree (wide_tree_cases.cases says why)."""
    p = w.plan(codec)
    n = len(W.NAMES)
    assert p.qstatus[: n + 1].tolist() == [0] * n + [-3] and p.s["unsupported_queries"] == 1 and W.STACK_REASON in p.last_unsupported and "it needs 65" in p.last_unsupported
    assert p.s["tree_queries"] == len(W.TREE_NAMES) == n - 1 and p.s["plw"] % S.TREE_CHUNK_WORDS == 0 and p.s["plw"] // S.TREE_CHUNK_WORDS >= 5
    for i, (name, (prog, hdr, root)) in enumerate(w.cases.items()):
        sl = int(p.slot_of_query[i])
        kind = int(p.tasks["kind"][int(p.plan["first_task"][sl])])
        if hdr is None:
            assert kind != HP.TASK_TREE, name
            continue
        assert kind == HP.TASK_TREE and p.tree_kind(sl) == (HP.TREE_KIND_WIDE, hdr[0]), name
        assert p.tree_header(sl)[:4].tolist() == [hdr[0], HP.TREE_KIND_WIDE, hdr[1], hdr[2]], (name, p.tree_header(sl)[:4].tolist())
        nd = p.tree_nodes_wide(sl)
        assert (int(nd["cbits"][-1]), int(nd["thr"][-1]), int(nd["nkids"][-1])) == root and int(nd["parent"][-1]) == HP.TREE_NO_PARENT, name
        leaves = nd[nd["op"] == O.OP_TERM]
        assert sorted(leaves["arg"].tolist()) == sorted((prog[prog >> 28 == O.OP_TERM] & 0x0FFFFFFF).tolist()), name  # (a leaf's arg is its term: what replay() looks up)
    allp = int(p.slot_of_query[W.NAMES.index("allP")])
    assert int(p.plan["out_cap"][allp]) == len(w.want("allP")) == len(w.act)
    nd = w.record("or1023", codec)
    assert len(nd) - 1 == 1023 == 31 * 32 + 31 and np.all(nd["parent"][:-1] == 1023)  # the root: word 31, bit 31 — every leaf's parent bit lies in the LAST word


@pytest.mark.parametrize("codec", [1, 2])
def test_three_answers_agree(w, codec):
    """Corpus.evaluate (numpy over the postings arrays) == the oracle's iterator tree (DocumentsOnly) == the fold replayed over the planner's record."""
    for name, (prog, hdr, _) in w.cases.items():
        want = w.want(name)
        assert len(want) > 0, name
        if codec == 1:
            assert np.array_equal(w.ora.exec(prog, O.FLAG_DOCUMENTS_ONLY)[0], want), name
        if hdr is not None:
            bits, _ = W.replay(w.record(name, codec), w.leaf)
            assert np.array_equal(W.docs_of(bits, w.act), want), name
    mask = W.chunk_edge_mask()
    w.ora.set_masked(mask)
    try:
        for name in ("or1023", "allP", "deep64"):
            assert np.array_equal(w.ora.exec(w.cases[name][0], O.FLAG_DOCUMENTS_ONLY)[0], w.c.evaluate(w.cases[name][0], masked=mask)), name
    finally:
        w.ora.set_masked(np.zeros(0, np.uint32))


def test_closed_forms(w):
    """A matchsome of m leaves per ladder list counts m h(d): it holds iff h(d) >= ceil(thr / m).  255 and 256 differ, 256 and 260 do not; the other forms by hand."""
    for name, least in W.CLOSED.items():
        assert np.array_equal(w.want(name), w.act[W.h_of(w.act) >= least].astype(np.uint32)), name
    assert [W.CLOSED[f"some300_{t}"] for t in (255, 256, 260, 300)] == [51, 52, 52, 60] and [W.CLOSED[f"some1020_{t}"] for t in (1, 510, 511, 1020)] == [1, 30, 31, 60]
    a, b, c = (w.want(f"some300_{t}") for t in (255, 256, 260))
    assert not np.array_equal(a, b) and np.array_equal(b, c)
    assert np.array_equal(w.want("not_wide"), w.act[W.h_of(w.act) == 1].astype(np.uint32)) and np.array_equal(w.want("allP"), w.act.astype(np.uint32))


def test_the_deep_cases_fill_the_stack(w):
    """The highest stack pointer of the fold is 64 — slot 63 written — for the alternation and for the chain of matchsomes (whose pushes are seven planes each); the parser
    sorts an AND's children by cost, so this is a property of the corpus too."""
    for name in ("deep64", "deep64_inner", "somechain", "somechain_inner"):
        assert W.replay(w.record(name), w.leaf)[1] == 64, name
    assert W.replay(w.record("some1020_511"), w.leaf)[1] == 10 and W.replay(w.record("some300_260"), w.leaf)[1] == 9


CAUGHT_BY = {"thr_byte": "some300_256", "planes8": "some300_255", "stack32": "deep64", "nodes64": "or1023"}


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_each_wrong_fold_is_caught_by_its_case(w, mutant):
    """A case that fails to tell its mutant apart is a failure of the catalogue."""
    name = CAUGHT_BY[mutant]
    nd = w.record(name)
    right, _ = W.replay(nd, w.leaf)
    wrong, _ = W.replay(nd, w.leaf, mutant)
    assert np.array_equal(W.docs_of(right, w.act), w.want(name)) and wrong != right, (mutant, name)
    caught = [n for n in W.TREE_NAMES if W.replay(w.record(n), w.leaf, mutant)[0] != W.replay(w.record(n), w.leaf)[0]]
    print(f"{mutant}: caught by {caught}")
    if mutant == "planes8":
        assert {"some300_255", "some1020_510", "some1020_511", "some1020_1020"} <= set(caught)  # the ninth plane and the tenth
    if mutant == "stack32":
        assert {"deep64", "somechain", "somechain_inner"} <= set(caught)


def test_or1023_scores_are_the_sum_of_its_leaves(w):
    """What "reached" means for k_tree_leaves_wide, without a second evaluator: the oracle's score of a match of or1023 is the sum, over the 1023 leaves, of the single-term
    scores of the terms that hold it — every one of the 32 node words contributes to a document with h = 60."""
    prog = w.cases["or1023"][0]
    docs, scores = w.ora.exec(prog, O.FLAG_ACCUM_SCORE)
    total = np.zeros(W.D + 1, dtype=np.float64)
    times = np.bincount(prog[:-1] & 0x0FFFFFFF, minlength=W.NLADDER)
    assert times.sum() == 1023 and times.min() == 17
    for t in range(W.NLADDER):
        d, s = w.ora.exec(np.array([O.tok(O.OP_TERM, t)], dtype=np.uint32), O.FLAG_ACCUM_SCORE)
        total[d] += int(times[t]) * s
    assert np.array_equal(docs, w.want("or1023")) and (W.h_of(docs) == 60).sum() == 72
    np.testing.assert_allclose(scores, total[docs], rtol=S.RTOL, atol=0)


def test_every_case_scores_the_leaves_the_reached_rule_names(w):
    """wide_tree_cases.reached restates k_tree_leaves_wide's two passes (values leaves-up; root-down in place: every child of an AND, the holding children of an OR /
    matchsome, NOT's required side, OPT's main side and its optional side where it holds).  On every tree case the oracle's score of a match is the sum of the single-term
    scores of the leaves the rule reaches — and with a parent's bit read from the word below its own, or1023's sums are no longer the oracle's."""
    term_score = np.zeros((len(w.c.names), len(w.act)), dtype=np.float64)
    rows = {}
    for t in range(len(w.c.names)):
        d, s = w.ora.exec(np.array([O.tok(O.OP_TERM, t)], dtype=np.uint32), O.FLAG_ACCUM_SCORE)
        at = np.searchsorted(w.act, d)
        term_score[t, at] = s
        rows[t] = np.zeros(len(w.act), dtype=bool)
        rows[t][at] = True

    def sums(name, mutant=None):
        nd = w.record(name)
        total = np.zeros(len(w.act), dtype=np.float64)
        for n, r in W.reached(nd, rows, mutant).items():
            total += np.where(r, term_score[int(nd["arg"][n])], 0.0)
        return total

    for name in W.TREE_NAMES:
        docs, scores = w.ora.exec(w.cases[name][0], O.FLAG_ACCUM_SCORE)
        np.testing.assert_allclose(sums(name)[np.searchsorted(w.act, docs)], scores, rtol=S.RTOL, atol=0, err_msg=name)
    docs, scores = w.ora.exec(w.cases["or1023"][0], O.FLAG_ACCUM_SCORE)
    wrong = sums("or1023", "parent_word")[np.searchsorted(w.act, docs)]
    assert not np.allclose(wrong, scores, rtol=S.RTOL, atol=0)


def scored_runs():
    return [(n, O.SIM_BM25) for n in W.NAMES] + [(n, O.SIM_TFIDF) for n in W.SCORED_TFIDF]


def test_score_gap_condition(w):
    """structured.check_topk compares top-10 docID lists exactly wherever the oracle's distinct scores within ranks 1 .. 11 differ by more than RTOL; at most 10 % of the
    scored runs (the project's cap, tests/test_structured.py) may need its set-wise rule — or the frequency pattern has to change, not the cap."""
    runs = scored_runs()
    setwise, smallest = 0, np.inf
    try:
        for name, sim in runs:
            w.ora.set_similarity(sim)
            docs, scores = w.ora.exec(w.cases[name][0], O.FLAG_ACCUM_SCORE)
            exact, gap = S.score_gaps(scores, 10)
            setwise += not exact
            smallest = min(smallest, gap)
    finally:
        w.ora.set_similarity(O.SIM_BM25)
    print(f"score-gap condition: {setwise} of {len(runs)} scored runs under the set-wise rule; smallest relative gap between distinct scores {smallest:.3g}")
    assert len(runs) == len(W.NAMES) + 2 and setwise <= 0.10 * len(runs), (setwise, len(runs))


def test_the_percolators_restatement_gives_the_closed_forms():
    """The same programs as stored queries over 60 terms, document j holding terms 0 .. j % 61 - 1: perc_cases.match_batch answers h(j) >= the closed form's least h."""
    progs, docs = W.perc_programs(), W.perc_docs()
    assert len(docs) == W.PERC_NDOCS == 130 and [len(d) for d in docs] == [j % 61 for j in range(130)]
    assert {"or1023", "deep64", "somechain"} | set(W.SOME_CASES) <= set(W.PERC_CASES)
    bits = PC.match_batch(progs, docs)
    for name, b in zip(W.PERC_CASES, bits):
        assert b == sum(1 << j for j in range(130) if j % 61 >= W.CLOSED[name]) and b, name
        assert all(PC.match_one(progs[W.PERC_CASES.index(name)], docs[j]) == bool((b >> j) & 1) for j in (0, 1, 2, 30, 31, 51, 52, 60, 61, 129)), name
