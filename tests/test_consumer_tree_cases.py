"""The yardstick of tests/test_gpu_consumers_trees.py, checked on the CPU (tests/consumer_tree_cases.py): through HostPlan the conditions the GPU tests rest on — so
that a planner change cannot silently empty them — and, for each of six wrong implementations of the consumers' walk over a batch's tasks, a named case whose expected
rows (facet_cases.facet_rows, order_cases.rows, stats_cases.stats_rows over structured.Corpus.evaluate's docID sets) it changes, for facets, order and stats alike:
  hidden_counted      a hidden leaf's list consumed into its owner's row: stream `"h2 h3" OR r0` (the leaf of five tasks) and phrase `pad NOT "a b"`;
  by_slot             rows indexed by plan slot: the phrase list, every query behind the first hidden slot;
  first_chunk_only    a tree query's list cut at 32 TREE_CHUNK_WORDS documents: the four new stream trees, NINE, allP;
  last_dropped        the last document of a tree query's region: NINE and allP, whose regions are filled exactly, and every other tree;
  root_filter_missing a tree query consumed without its filter: every stream tree under filter i % 3 on top of the mask;
  capacity_not_count  a multi-task caller phrase query read by capacity: `"h0 h1"` (11 tasks) and `"h1 h2" h0` (7 tasks).
No GPU here."""
import time

import numpy as np
import pytest

import consumer_tree_cases as CT
import facet_cases as F
import order_cases as OC
import structured as S
import trinity_amd as T
import wide_tree_cases as W


class Lists:
    """Corpora, lists, sets and facts, each made once."""

    def __init__(self):
        T.build.build_host()
        self._c, self._l, self._sets, self._facts, self._hidden, self.seconds = {}, {}, {}, {}, {}, {}

    def corpus(self, name):
        if name not in self._c:
            self._c[name] = W.corpus() if name == "wide" else S.CORPORA[name]()
        return self._c[name]

    def get(self, name):
        """(queries or names, programs, indices of the listed tree texts)"""
        if name not in self._l:
            c = self.corpus(name)
            if name == "wide":
                names, progs, _ = CT.wide_progs()
                self._l[name] = (names, progs, [names.index(n) for n in W.TREE_NAMES])
            else:
                make, trees = CT.LISTS[name]
                queries = make(c)
                self._l[name] = (queries, S.programs(queries), CT.tree_indices(c, queries, trees))
        return self._l[name]

    def sets(self, name):
        if name not in self._sets:
            t0 = time.time()
            self._sets[name] = CT.evaluate_all(self.corpus(name), self.get(name)[1])
            self.seconds[name] = time.time() - t0
        return self._sets[name]

    def facts(self, name, codec=1):
        if (name, codec) not in self._facts:
            hi = self.corpus(name).host_index(codec)
            try:
                self._facts[name, codec] = CT.Facts(hi, self.get(name)[1], options=W.WIDE if name == "wide" else None)
            finally:
                hi.close()
        return self._facts[name, codec]

    def hidden_sets(self, name):
        """{hidden slot: the docID set of the phrase it runs}"""
        if name not in self._hidden:
            fx = self.facts(name)
            self._hidden[name] = dict(zip(fx.hidden, CT.evaluate_all(self.corpus(name), [fx.hidden_prog[h] for h in fx.hidden])))
        return self._hidden[name]

    def cols(self, name):
        return OC.columns(self.corpus(name).D)

    def text(self, name, i):
        q = self.get(name)[0][i]
        return q if isinstance(q, str) else q[0]


@pytest.fixture(scope="module")
def L():
    return Lists()


# ------------------------------------------------------------------------------------------ the conditions the GPU tests rest on
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", ["phrase", "stream", "main", "wide"])
def test_every_listed_tree_text_is_a_tree_query(L, name, codec):
    fx = L.facts(name, codec)
    _, progs, trees = L.get(name)
    assert trees and all(fx.tree[i] and fx.ntasks[i] == 1 for i in trees), (name, [L.text(name, i) for i in trees if not fx.tree[i]])
    assert fx.tree_queries == int(fx.tree.sum()) >= len(trees), (name, fx.tree_queries, len(trees))
    print(f"{name} (codec {codec}): {fx.nq} queries in {fx.n_plan} slots, {fx.tree_queries} tree queries, {len(fx.hidden)} hidden queries of {[int(fx.slot_tasks[h]) for h in fx.hidden]} tasks")
    if name == "main":  # (when this was written the planner made a tree record for NINE alone of main_queries' last three texts)
        print("main: tree queries", [L.text(name, i) for i in range(fx.nq) if fx.tree[i]])


@pytest.mark.parametrize("codec", [1, 2])
def test_the_phrase_list_has_hidden_queries_between_the_callers(L, codec):
    fx = L.facts("phrase", codec)
    assert fx.nq == 17 and fx.tree_queries >= 3 and len(fx.hidden) >= 4
    moved = [i for i in range(fx.nq) if fx.slot[i] != i]
    assert len(moved) >= 1 and fx.n_plan == fx.nq + len(fx.hidden)
    print(f"phrase (codec {codec}): {len(moved)} queries in a slot other than their index")  # (7 when this was written)
    assert all(fx.leaves[i] for i in L.get("phrase")[2]) and sum(len(v) for v in fx.leaves.values()) == len(fx.hidden)
    # pad NOT "a b": the longest single task of the list, in a region of D documents it does not fill
    i = L.get("phrase")[2][0]
    assert len(L.sets("phrase")[i]) == 6913 < int(fx.out_cap[i]) <= L.corpus("phrase").D == 6957


@pytest.mark.parametrize("codec", [1, 2])
def test_the_stream_list_has_multi_task_hidden_queries_and_multi_task_phrases(L, codec):
    """A hidden query of at least 2 tasks: its first task carries the gathered list's whole length, the others 0.  A caller phrase query of 2 or more tasks: compacted
    segments."""
    fx = L.facts("stream", codec)
    tasks = [int(fx.slot_tasks[h]) for h in fx.hidden]
    assert max(tasks) >= 2 and fx.tree_queries >= 5 and all(fx.leaves[i] for i in L.get("stream")[2]), tasks  # (5, 2, 11, 11, 5 and 11 tasks when this was written)
    multi = fx.multi_task_phrases()
    assert len(multi) >= 1, [int(fx.ntasks[i]) for i in range(fx.nq) if fx.nphrases[i]]
    print(f"stream (codec {codec}): hidden queries of {tasks} tasks, caller phrase queries of {sorted(int(fx.ntasks[i]) for i in multi)} tasks")
    assert {i % 3 for i in L.get("stream")[2]} == {0, 1, 2}  # (under filter i % 3 the tree queries meet all three filters)


def test_stream_tree_results_lie_in_every_chunk_and_on_chunk_edges(L):
    """Five chunks of 32 TREE_CHUNK_WORDS documents, the last two words long.  The stream corpus has NO posting on C - 1 (shown here): its lists all hold 2C - 1, 2C and
    2C + 1, so that is the chunk edge a stream tree result can straddle — C - 1, C and C + 1 themselves are NINE's and the wide catalogue's (below)."""
    c, sets = L.corpus("stream"), L.sets("stream")
    assert c.D == S.D_STREAM == 4 * CT.C + 37 and (c.D >> 5) - 4 * S.TREE_CHUNK_WORDS == 1
    assert not np.isin(CT.C - 1, c.docs) and S.SPAN_BITS == 2 * CT.C
    full = [i for i in L.get("stream")[2] if np.unique(sets[i] // CT.C).tolist() == [0, 1, 2, 3, 4] and np.isin([2 * CT.C - 1, 2 * CT.C, 2 * CT.C + 1, 4 * CT.C, c.D], sets[i]).all()]
    assert len(full) >= 1, [np.unique(sets[i] // CT.C).tolist() for i in L.get("stream")[2]]
    print("stream trees in all five chunks and on 2C - 1, 2C, 2C + 1, 4C, D:", [L.text("stream", i) for i in full])
    every = [i for i in L.get("stream")[2] if np.unique(sets[i] // CT.C).tolist() == [0, 1, 2, 3, 4]]
    assert len(every) == 5  # (all five tree texts of the list)
    print("numpy reference over the stream list: %.1f s" % L.seconds["stream"])


@pytest.mark.parametrize("codec", [1, 2])
def test_nine_and_allp_fill_their_regions_exactly(L, codec):
    for name, i in (("main", 0), ("wide", W.NAMES.index("allP"))):
        fx, s = L.facts(name, codec), L.sets(name)[i]
        assert fx.tree[i] and int(fx.out_cap[i]) == len(s), (name, int(fx.out_cap[i]), len(s))
        assert np.isin([CT.C - 1, CT.C, CT.C + 1, L.corpus(name).D], s).all() and s[-1] == L.corpus(name).D
    assert len(L.sets("main")[0]) == S.D_MAIN == 524325 and np.unique(L.sets("main")[0] // CT.C).size == 9
    fx = L.facts("wide", codec)
    names, _, status = CT.wide_progs()
    assert fx.status.tolist() == status and status[-1] == -3 and fx.slot[-1] == -1 and not fx.hidden


# ------------------------------------------------------------------------------------------ wrong answers
def rows_at(L, name, sets, i):
    """consumer_rows of ONE query's docID (multi)set."""
    D = L.corpus(name).D
    return CT.consumer_rows([sets[i]], L.cols(name), CT.specs(D, main=name == "main"))


def assert_told(L, name, right, wrong, cases, tag):
    for i in cases:
        t = CT.told(rows_at(L, name, right, i), rows_at(L, name, wrong, i))
        assert all(t.values()), (tag, name, L.text(name, i), t)


def test_hidden_counted_changes_its_cases(L):
    for name, text in (("stream", '"{h2} {h3}" OR {r0}'), ("phrase", '{pad} NOT "{a} {b}"')):
        c = L.corpus(name)
        i = [t for t, _ in L.get(name)[0]].index(c.q(text))
        fx, sets = L.facts(name), L.sets(name)
        wrong = CT.hidden_counted(sets, fx, L.hidden_sets(name))
        assert len(wrong[i]) > len(sets[i]) and fx.leaves[i]
        assert_told(L, name, sets, wrong, [i], "hidden_counted")
        assert all(np.array_equal(wrong[j], sets[j]) for j in range(fx.nq) if not fx.tree[j])
    fx = L.facts("stream")
    i = [t for t, _ in L.get("stream")[0]].index(L.corpus("stream").q('"{h2} {h3}" OR {r0}'))
    assert all(int(fx.slot_tasks[h]) >= 2 for h in fx.leaves[i])  # (a leaf whose gathered list is longer than its first task's segment: 5 tasks when this was written)
    assert_told(L, "stream", L.sets("stream"), CT.hidden_counted(L.sets("stream"), fx, L.hidden_sets("stream")), L.get("stream")[2], "hidden_counted")


def test_by_slot_changes_the_phrase_list(L):
    fx, sets = L.facts("phrase"), L.sets("phrase")
    wrong = CT.by_slot(sets, fx, L.hidden_sets("phrase"))
    moved = [i for i in range(fx.nq) if fx.slot[i] != i]
    differ = [i for i in moved if not np.array_equal(wrong[i], sets[i])]
    assert len(differ) >= 5, (moved, differ)  # ("a b" <c> and "a b" hold the same documents: slot order cannot tell those apart)
    assert_told(L, "phrase", sets, wrong, differ, "by_slot")
    assert all(np.array_equal(wrong[i], sets[i]) for i in range(fx.nq) if i not in moved)


def test_first_chunk_only_and_last_dropped_change_every_tree_with_documents_past_the_first_chunk(L):
    for name in ("stream", "main", "wide"):
        fx, sets = L.facts(name), L.sets(name)
        trees = [i for i in L.get(name)[2] if len(sets[i])]
        wrong = CT.first_chunk_only(sets, fx)
        past = [i for i in trees if sets[i][-1] >= CT.C]
        assert past and (name != "stream" or len(past) == 5), (name, past)
        assert_told(L, name, sets, wrong, past if name != "wide" else [W.NAMES.index("allP"), W.NAMES.index("or1023")], "first_chunk_only")
        wrong = CT.last_dropped(sets, fx)
        assert_told(L, name, sets, wrong, trees if name != "wide" else [W.NAMES.index("allP"), W.NAMES.index("or1023")], "last_dropped")
    fx, sets = L.facts("phrase"), L.sets("phrase")
    assert_told(L, "phrase", sets, CT.last_dropped(sets, fx), L.get("phrase")[2], "last_dropped")


def test_root_filter_missing_changes_every_stream_tree(L):
    c, fx, full = L.corpus("stream"), L.facts("stream"), L.sets("stream")
    masked, drops = F.stream_masked(c.D), F.stream_filter_drops(c.D)
    msets = CT.without(full, masked)
    fsets = CT.without(msets, [drops[i % 3] for i in range(len(full))])
    wrong = CT.root_filter_missing(msets, fx, fsets)
    trees = L.get("stream")[2]
    assert all(0 < len(fsets[i]) < len(msets[i]) < len(full[i]) for i in trees)
    assert_told(L, "stream", fsets, wrong, trees, "root_filter_missing")
    assert_told(L, "stream", msets, full, trees, "unmasked")
    assert all(np.array_equal(wrong[i], fsets[i]) for i in range(fx.nq) if not fx.tree[i])
    # the wide catalogue's mask and drop filter (every second query): the same discipline
    wfx, wfull = L.facts("wide"), L.sets("wide")
    wm = CT.without(wfull, W.chunk_edge_mask())
    wf = CT.without(wm, [W.filter_drop() if i % 2 == 1 else CT.NONE for i in range(len(wfull))])
    odd = [i for i in L.get("wide")[2] if i % 2 == 1 and len(wf[i])]
    assert len(odd) >= 5
    assert_told(L, "wide", wf, CT.root_filter_missing(wm, wfx, wf), odd, "root_filter_missing")


def test_capacity_not_count_changes_the_multi_task_phrases(L):
    c, fx, sets = L.corpus("stream"), L.facts("stream"), L.sets("stream")
    multi = fx.multi_task_phrases()
    cand = {i: c.evaluate(CT.conjunction_of(L.get("stream")[1][i])) for i in multi}
    wrong = CT.capacity_not_count(sets, fx, cand)
    texts = [t for t, _ in L.get("stream")[0]]
    named = [texts.index(c.q('"{h0} {h1}"')), texts.index(c.q('"{h1} {h2}" {h0}'))]
    assert set(named) <= set(multi), [int(fx.ntasks[i]) for i in named]  # (11 and 7 tasks when this was written)
    assert all(len(cand[i]) > len(sets[i]) and np.isin(sets[i], cand[i]).all() for i in multi)
    assert_told(L, "stream", sets, wrong, multi, "capacity_not_count")
    assert all(np.array_equal(wrong[i], sets[i]) for i in range(fx.nq) if i not in multi)


def test_the_specs_lie_on_both_sides_of_both_lds_budgets(L):
    for name in ("phrase", "stream", "main", "wide"):
        sp = CT.specs(L.corpus(name).D, main=name == "main")
        assert len(sp["facets_on_chip"]) <= F.FACETS_MAX and sp["facets_direct"][0][0] == "low16" and sp["facets_direct"][0][1] + 1 > F.LDS_COUNTERS
        assert any(g is None for g, _, _ in sp["stats_on_chip"]) and any(g is not None for g, _, _ in sp["stats_on_chip"])
    assert {(n, k, d) for n, k, d in CT.ORDERS} == {(n, k, d) for n in ("hash", "rev", "one") for k in (10, 256) for d in (False, True)}
