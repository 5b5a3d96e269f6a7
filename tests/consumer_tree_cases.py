"""Facets, order and stats over TASK_TREE queries, their hidden phrase queries and wide records (a helper module, imported by tests/test_consumer_tree_cases.py — CPU —
and tests/test_gpu_consumers_trees.py): the query lists, the consumer specs, the planner's facts about a list and six wrong implementations of "a workgroup per task
over every task of the batch".

The three consumers (csrc/k_facet.hpp, k_order.hpp, k_stats.hpp) walk every task of a batch.  A TASK_TREE query brings tasks none of the other consumer tests hold:
  * hidden queries — the phrase leaves of a tree, planned as queries of their own with qid 0xffffffff: the consumers skip them, and index their rows by the caller's
    query, not by plan slot (the hidden slots sit between the callers');
  * a hidden query of several tasks: after k_tree_gather its first task carries the length of the whole gathered list, the others 0;
  * the tree query itself: ONE task whose segment is the whole result, written by k_tree_expand in chunks of C = 32 TREE_CHUNK_WORDS documents, possibly filling its
    region exactly (out_cap == matches); its filter is applied at the root only;
  * a caller's phrase query of several tasks, whose segments are compacted: counts[task] documents of a region laid out for every candidate.

The lists (corpora of tests/structured.py and tests/wide_tree_cases.py; nothing here is generated anew):
  phrase   structured.phrase_queries as it stands: 17 queries in 21 plan slots, 3 tree queries, 4 hidden queries, 7 queries in a slot other than their index;
  stream   structured.stream_queries and STREAM_TREE_TEXTS: 58 queries in 64 slots, 5 tree queries, 6 hidden queries of 5, 2, 11, 11, 5 and 11 tasks, 13 caller phrase
           queries of which 12 have 2 .. 11 tasks; all five tree results have documents in all five chunks;
  main     NINE — one task of 524 325 matches in a region of 524 325 — and three neighbours.  Of main_queries' three last texts only NINE is a TASK_TREE query: the
           planner lowers `{edges} NOT ({all} {odd})` and `{lastwin} OR ({all} {edges})` without a tree record (test_consumer_tree_cases.py prints their kinds);
  wide     wide_tree_cases.cases() under tree_max_nodes = 1024, deep65 left out with status -3.
The stream corpus holds no posting on C - 1 = 65 535 (test_consumer_tree_cases.py asserts it): every list of it holds 2C - 1, 2C, 2C + 1 (SPAN_BITS - 1 .. + 1), 4C and D,
so the chunk edge a stream tree result straddles is the one between chunks 1 and 2; C - 1, C and C + 1 themselves are held by NINE and by the wide catalogue's cases.

structured.Corpus.evaluate over the stream list takes 5 s on the machine this was written on (one core; 14 s without the memo of evaluate_all: "h0 h1" alone is 3 s
and four texts hold it), over the phrase list 0.01 s, over the main list 0.05 s; tests/test_consumer_tree_cases.py prints the stream figure."""
import numpy as np

import facet_cases as F
import oracle_lib as O
import order_cases as OC
import stats_cases as X
import structured as S
import wide_tree_cases as W

C = S.TREE_CHUNK_WORDS * 32  # documents k_tree_expand writes per chunk
HIDDEN = 0xFFFFFFFF
NONE = np.zeros(0, np.uint32)

# ---- the lists ------------------------------------------------------------------------------------------------------------------------------------
PHRASE_TREE_TEXTS = ['{pad} NOT "{a} {b}"', '"{a} {b}" OR "{b} {c}"', '{c} OR "{a} {b}"']
# stream: phrase leaves that are hidden queries of several tasks, results in every chunk.  [text, matchsome minimum]
STREAM_TREE_TEXTS = [('{h0} NOT "{h0} {h1}"', 1), ('{h11} OR ("{h0} {h1}" {h2})', 1), ('"{h2} {h3}" OR {r0}', 1), ('["{h0} {h1}", {h6}, {r2}]', 2)]
STREAM_OLD_TREE = '"{h2} {h3}" OR "{h4} {h5}"'  # (the one tree text stream_phrase_queries holds)
MAIN_TREE_TEXTS = [S.NINE]
MAIN_TEXTS = [S.NINE, "{edges} NOT ({all} {odd})", "{lastwin} OR ({all} {edges})", "{all} OR {odd}"]


def phrase_list(c):
    return S.phrase_queries(c)


def stream_list(c):
    return S.stream_queries(c) + [(c.q(t), mn) for t, mn in STREAM_TREE_TEXTS]


def main_list(c):
    return [(c.q(t), 1) for t in MAIN_TEXTS]


def tree_indices(c, queries, texts):
    """Where the listed tree texts sit in a list."""
    at = {t: i for i, (t, _) in enumerate(queries)}
    return [at[c.q(t)] for t in texts]


LISTS = {"phrase": (phrase_list, PHRASE_TREE_TEXTS), "stream": (stream_list, [STREAM_OLD_TREE] + [t for t, _ in STREAM_TREE_TEXTS]), "main": (main_list, MAIN_TREE_TEXTS)}


def evaluate_all(c, progs, masked=None):
    """structured.Corpus.evaluate of every program, with the phrase check of a term sequence made once per list (numpy's phrase check is slow and the tree texts repeat
    the plain phrase texts' leaves): the reference itself is untouched, its _phrase is looked up in a table first."""
    memo, phrase = {}, c._phrase

    def once(terms, sets):
        key = tuple(terms)
        if key not in memo:
            memo[key] = phrase(terms, sets)
        return memo[key]

    c._phrase = once  # (an instance attribute in front of the method, taken away again below)
    try:
        return [c.evaluate(p, masked=masked) for p in progs]
    finally:
        del c._phrase


def without(sets, gone):
    """Every set minus the documents `gone` (one array for all, or one per set)."""
    per = gone if isinstance(gone, list) else [gone] * len(sets)
    return [s[~np.isin(s, g)] if len(g) else s for s, g in zip(sets, per)]


# ---- the consumer specs ------------------------------------------------------------------------------------------------------------------------------
FACETS_ON_CHIP = [("mod7", 7), ("window", None), ("huge", None)]
FACETS_DIRECT = [("low16", None)]  # one row past FACET_LDS_COUNTERS: global atomics
ORDERS = [(name, k, desc) for name in ("hash", "rev", "one") for k in (10, 256) for desc in (False, True)]
STATS_ON_CHIP = list(X.STREAM_STATS)  # (None, 0, hash): registers; (mod7, 5, rev): on chip, mod7 overflows 5 buckets
STATS_DIRECT = [X.MIXED_DIRECT[1]]  # (low16, STATS_LDS_BUCKETS, rev): one record past the budget
# the main corpus: one workgroup, 524 325 documents — `rev` ascending (the best keys come last: every step beats the threshold), `one` at K = 256 in both directions
# (the lowest 256 docIDs), window as facet and as group (every match through one LDS flush), hash ungrouped (the sum passes 2^32)
MAIN_ORDERS = [("rev", 10, False), ("rev", 256, False), ("one", 256, False), ("one", 256, True), ("hash", 10, True)]
MAIN_FACETS = [("window", None), ("mod7", 7)]
MAIN_STATS = [(None, 0, "hash"), ("window", None, "hash"), ("mod7", 5, "rev")]


def specs(D, main=False):
    """{group: spec} for a corpus of D documents, bucket counts resolved; the two sides of both LDS budgets are asserted here."""
    out = {"facets_on_chip": F.resolve(MAIN_FACETS if main else FACETS_ON_CHIP, D), "facets_direct": F.resolve(FACETS_DIRECT, D), "orders": list(MAIN_ORDERS if main else ORDERS),
           "stats_on_chip": X.resolve(MAIN_STATS if main else STATS_ON_CHIP, D), "stats_direct": X.resolve(STATS_DIRECT, D)}  # fmt: skip
    assert sum(nb + 1 for _, nb in out["facets_on_chip"]) <= F.LDS_COUNTERS < sum(nb + 1 for _, nb in out["facets_direct"]), D
    assert 0 < X.lds_records(out["stats_on_chip"]) <= X.LDS_BUCKETS < X.lds_records(out["stats_direct"]), D
    return out


def facet_want(sets, cols, facets):
    return [F.facet_rows(sets, cols[name], nb) for name, nb in facets]


def order_want(sets, cols, order):
    name, k, desc = order
    return OC.rows(sets, cols[name], k, desc)


def stats_want(sets, cols, stats):
    return [X.stats_rows(sets, None if g is None else cols[g], nb, cols[v]) for g, nb, v in stats]


def same_facets(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


same_order = same_facets  # (docids, values, counts): arrays too


def same_stats(a, b):
    return all(X.same(x, y) for x, y in zip(a, b))


def consumer_rows(sets, cols, sp):
    """The expected rows of all three consumers over docID sets (or multisets: a wrong implementation's), by group of specs."""
    return {"facets_on_chip": facet_want(sets, cols, sp["facets_on_chip"]), "facets_direct": facet_want(sets, cols, sp["facets_direct"]),
            "orders": [order_want(sets, cols, o) for o in sp["orders"]], "stats_on_chip": stats_want(sets, cols, sp["stats_on_chip"]),
            "stats_direct": stats_want(sets, cols, sp["stats_direct"])}  # fmt: skip


def told(a, b):
    """Per consumer: do two consumer_rows differ?"""
    return {"facets": not (same_facets(a["facets_on_chip"], b["facets_on_chip"]) and same_facets(a["facets_direct"], b["facets_direct"])),
            "order": not all(same_order(x, y) for x, y in zip(a["orders"], b["orders"])),
            "stats": not (same_stats(a["stats_on_chip"], b["stats_on_chip"]) and same_stats(a["stats_direct"], b["stats_direct"]))}  # fmt: skip


# ---- the planner's facts about a list -------------------------------------------------------------------------------------------------------------------
def phrase_leaves(prog):
    """The phrase sub-programs (TERM ... PHRASE n) of a postfix program, in program order."""
    w = np.asarray(prog, dtype=np.uint32).tolist()
    return [np.array(w[i - (x & 0x0FFFFFFF) : i + 1], dtype=np.uint32) for i, x in enumerate(w) if x >> 28 == O.OP_PHRASE]


def conjunction_of(prog):
    """The program with every phrase taken as the conjunction of its terms: what a phrase task's candidate region holds before the positional check compacts it."""
    w = np.asarray(prog, dtype=np.uint32).copy()
    ph = w >> 28 == O.OP_PHRASE
    w[ph] = [O.tok(O.OP_AND, int(x) & 0x0FFFFFFF) for x in w[ph]]
    return w


class Facts:
    """What HostPlan (FLAG_DOCUMENTS_ONLY) says about a list: per caller query its slot, status, task kind, tasks, region and phrases; the hidden queries, each with the
    phrase sub-program it runs and the tree query that names it."""

    def __init__(self, hindex, progs, options=None):
        import trinity_amd as T
        from trinity_amd import hostplan as HP

        p = HP.HostPlan(hindex, progs, T.FLAG_DOCUMENTS_ONLY, options=options)
        try:
            nq = self.nq = len(progs)
            plan, tasks, qterms = p.plan.copy(), p.tasks.copy(), p.qterms.copy()
            self.n_plan, self.tree_queries = int(p.s["n_plan"]), int(p.s["tree_queries"])
            self.status = p.qstatus[:nq].astype(np.int64)
            self.slot = np.where(self.status == 0, p.slot_of_query[:nq].astype(np.int64), -1)
            self.qid = plan["qid"].astype(np.int64)
            self.slot_tasks, self.slot_cap = plan["ntasks"].astype(np.int64), plan["out_cap"].astype(np.int64)
            kind = tasks["kind"][plan["first_task"]]
            at = np.maximum(self.slot, 0)
            self.tree = (kind[at] == HP.TASK_TREE) & (self.slot >= 0)
            self.ntasks, self.out_cap = np.where(self.slot >= 0, self.slot_tasks[at], 0), np.where(self.slot >= 0, self.slot_cap[at], 0)
            self.nphrases = np.where(self.slot >= 0, plan["nphrases"].astype(np.int64)[at], 0)
            self.hidden = np.nonzero(plan["qid"] == HIDDEN)[0].tolist()
            self.hidden_prog, self.leaves = {}, {i: [] for i in range(nq)}
            for i in np.nonzero(self.tree)[0].tolist():
                sl = int(self.slot[i])
                nd = p.tree_nodes_wide(sl) if p.tree_kind(sl)[0] == HP.TREE_KIND_WIDE else p.tree_nodes(sl)
                subs = phrase_leaves(progs[i])
                for h in [int(x["arg"]) for x in nd if int(x["op"]) == O.OP_PHRASE]:
                    assert self.qid[h] == HIDDEN and h < sl, (i, h)
                    terms = set((qterms[int(plan["term_base"][h]) : int(plan["term_base"][h]) + int(plan["nterms"][h])] & 0x3FFFFFFF).tolist())
                    mine = [s for s in subs if set((s[:-1] & 0x0FFFFFFF).tolist()) == terms]
                    assert mine, (i, h, terms)
                    self.hidden_prog[h] = mine[0]
                    self.leaves[i].append(h)
            assert sorted(self.hidden_prog) == self.hidden
        finally:
            p.close()

    def multi_task_phrases(self):
        """The caller's phrase queries (no tree) of two or more tasks."""
        return [i for i in range(self.nq) if not self.tree[i] and self.nphrases[i] and self.ntasks[i] >= 2]


# ---- what a wrong implementation would answer: (sets, facts, ...) -> the docID multisets it would consume; consumer_rows() of those are its rows ----------------------
def hidden_counted(sets, facts, hidden_sets):
    """A hidden leaf's list consumed too, into its owner's row: the owner's set plus its phrase leaves' sets, as a multiset."""
    return [np.concatenate([s] + [hidden_sets[h] for h in facts.leaves[i]]) if facts.leaves[i] else s for i, s in enumerate(sets)]


def by_slot(sets, facts, hidden_sets):
    """Rows indexed by plan slot and read by caller query: row i holds what slot i consumed (a hidden slot: its leaf's list)."""
    per_slot = [hidden_sets[sl] if facts.qid[sl] == HIDDEN else sets[int(facts.qid[sl])] for sl in range(facts.n_plan)]
    return per_slot[: len(sets)]


def first_chunk_only(sets, facts):
    """Only the first chunk of a tree query's list read: its documents below C."""
    return [s[s < C] if facts.tree[i] else s for i, s in enumerate(sets)]


def last_dropped(sets, facts):
    """The last document of a tree query's region not read."""
    return [s[:-1] if facts.tree[i] else s for i, s in enumerate(sets)]


def root_filter_missing(masked_sets, facts, filtered_sets):
    """A tree query consumed without its filter (applied at the root only: its leaves ran against the mask alone): the masked-only set where a filter applies."""
    return [m if facts.tree[i] else f for i, (m, f) in enumerate(zip(masked_sets, filtered_sets))]


def capacity_not_count(sets, facts, candidate_sets):
    """A caller's phrase query of several tasks read by its segments' capacity, not their compacted counts: every candidate of the conjunction."""
    multi = set(facts.multi_task_phrases())
    return [candidate_sets[i] if i in multi else s for i, s in enumerate(sets)]


# ---- the wide catalogue ----------------------------------------------------------------------------------------------------------------------------------
def wide_progs():
    """wide_tree_cases' cases and the one left out, as test_gpu_wide_tree_limits.Catalogue orders them: (names, programs, statuses)."""
    cases, left = W.cases(), W.left_out()
    return W.NAMES + list(left), [cases[n][0] for n in W.NAMES] + [p for p, _, _ in left.values()], [0] * len(W.NAMES) + [st for _, st, _ in left.values()]
