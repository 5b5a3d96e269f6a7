"""Planner and launch options whose non-default values no other test sets (a helper module, imported by tests/test_plan_variants.py and
tests/test_gpu_plan_variants.py): a batch's answer depends on the segment and the queries alone — not on how plan_batch cuts a query into tasks
(phrase_task_div, dense_window_cost), which kernel and result form a union gets (scatter_bitmap_slack), the order of the tasks in sched[] / unit_sched[]
(pset_order, planes_order) or the streams the matching kernels run on (overlap, overlap_dense_wgs / overlap_cand_wgs).

VARIANTS lists them as (name, options, claim).  A claim is a function of (the default HostPlan, the variant's HostPlan) over the same corpus, queries, mode
and base options — one of CLAIM_CASES[name] — that is true only when the option did what it is there for: a variant whose option the planner ignored (or
whose name was mistyped into another option's) fails its claim instead of passing the GPU file vacuously.  The overlap* options change launches, not plans:
their claim is made on the GPU by run_matching's fork condition (tri_batch_info: dense_queries + pset_queries > 0 and cand_queries > 0).

Why base options: the catalogue's corpora are small (3 .. 17 docID windows), so by default a phrase query is one kind of task in a plan.  PHRASE_MIX makes ONE plan
of the stream corpus hold phrase queries as plane-set windows (both terms among the two with planes), bitmap windows (a term without a plane) and candidate
tiles (short enough for dense_min_postings = 65536, leads of two to seven tiles), with a cand_task_cost at which 1, 2, 4 and 8 all cut the tiles differently and a
dense_task_cost (96 K) at which, uncut, the lighter bitmap-window phrase queries are tasks of two windows and the heavier ones a task a window — seams on the first
window boundary, where every head term holds documents."""
import numpy as np

import structured as S
from trinity_amd import hostplan as HP

CONSTANTS = S.header_constants("dev_structs.hpp")
PL_PLANES = CONSTANTS["PL_PLANES"]
PSET_TASK_WINDOWS = CONSTANTS["PSET_TASK_WINDOWS"]
SPAN_WORDS = S.SPAN_BITS // 32
QT_TERM = CONSTANTS["QT_TERM"]
PSET_UNIT_SCATTER = CONSTANTS["PSET_UNIT_SCATTER"]
RESULT_DOCIDS, RESULT_BITMAP = 0, 1
FLAG_DOCS, FLAG_SCORED, FLAG_RICH = 1, 2, 4  # TRI_FLAG_DOCUMENTS_ONLY, TRI_FLAG_ACCUMULATED_SCORE, TRI_FLAG_MATCHED_TERMS (test_plan_variants.py checks them against the package)
MODES = {"docs": (FLAG_DOCS, 0), "scored": (FLAG_SCORED, 10), "rich": (FLAG_RICH, 0)}


def plane_words(D):
    """Words of one bitmap over a corpus of D documents as the planner lays it out (planner.hpp eligible_planes: whole windows and a spare one)."""
    return ((D >> 17) + 2) * SPAN_WORDS


PHRASE_MIX = {"dense_min_postings": 65536, "plane_div": S.ALL_PLANES, "plane_max_bytes": 2 * PL_PLANES * plane_words(S.D_STREAM) * 4, "cand_task_cost": 1 << 18, "dense_task_cost": 96 << 10}
ALL_WINDOWS = {"dense_min_postings": 0, "planes": 0}
MATCH_THEN_SCORE = {"dense_min_postings": 0, "fused": 0}  # scored queries as k_psets / k_and_dense / k_and tasks, then k_score (the one-pass kernels have no window tasks to cut)
SCATTER_PLANE_DIV = 4096  # at this plane_div lists of 128 documents and more are head terms: a union can then miss the scatter rule at slack 64 too

# ---- the query lists ----------------------------------------------------------------------------------------------------------------------
# (main corpus) unions of head terms with terms too short for a plane, around  min(N, head documents) x slack >= windows x SPAN_WORDS  for slack 1, 4 and 64
SCATTER_UNIONS = ["{lastwin} OR {last1}", "{rnd10} OR {df31} OR {first1}", "{edges} OR {last1}", "{runs} OR {df127}", "{df4065} OR {last1}", "{df4064} OR {df33}", "{df129} OR {df31}",
                  "{df128} OR {df127} OR {last1}", "{holes} OR {stub}", "{firstwin} OR {first1}"]  # fmt: skip


def scatter_unions(c):
    return [(c.q(t), 1) for t in SCATTER_UNIONS]


# (main corpus) the consumers' batches: window, plane-set and candidate-tile queries together — and, in the second list, scatter unions beside bitmap-window queries
CONSUMER_TEXTS = ["{df33}", "{all} OR {odd}", "{first1} OR {last1}", "{all} {odd}", "{edges} {all}", "{df33} {all}", "{df8193} {edges}", "{df4065} OR {last1}", "{df129} {odd}",
                  "{lastwin} OR ({all} {edges})", "{sparse_runs} {edges}", "{df24577} {rnd3}"]  # fmt: skip
CONSUMER_SCATTER_TEXTS = CONSUMER_TEXTS + ["{edges} OR {last1}", "{lastwin} OR {last1}", "{runs} OR {df127}", "{holes} OR {stub}"]
# the default mode's batch (its references walk every match in plain Python: small results), the ranker's pairs come from the lists' positions 1 .. f
RICH_TEXTS = ["{df33}", "{first1} OR {last1}", "{edges} {lastwin}", "{df33} {all}", "{df8193} {edges}", "{df4065} OR {last1}", "{df129} {odd}", "{sparse_runs} {edges}", "{df4064} {df4065} {all}",
              "{edges} ({df129} OR {df33})"]  # fmt: skip


# (tall corpus) the default mode over 17 .. 18 windows: unions and conjunctions of the rare lists (small results, bitmap-window tasks the default cuts in two)
TALL_RICH_TEXTS = ["{gap4_a} OR {gap4_b}", "{tall_edges} OR {gap4_b}", "{gap4_a} OR {gap4_c}", "{gap4_b} OR {tall_edges} OR {gap4_a}", "{tall_edges} {tall_odd}", "{gap4_c} {tall_33}", "{gap4_a} {tall_odd}",
                   "{tall_edges} NOT {tall_odd}"]  # fmt: skip


def tall_rich_queries(c):
    return [(c.q(t), 1) for t in TALL_RICH_TEXTS]


def consumer_queries(c):
    return [(c.q(t), 1) for t in CONSUMER_TEXTS]


def consumer_scatter_queries(c):
    return [(c.q(t), 1) for t in CONSUMER_SCATTER_TEXTS]


def rich_queries(c):
    return [(c.q(t), 1) for t in RICH_TEXTS]


def main_with_unions(c):
    return S.main_queries(c) + scatter_unions(c)


QUERY_LISTS = {"main": S.main_queries, "main+unions": main_with_unions, "unions": scatter_unions, "stream": S.stream_queries, "stream_phrases": S.stream_phrase_queries, "phrase": S.phrase_queries, "tall": S.tall_queries, "tall_scored": S.tall_scored_queries, "tall_rich": tall_rich_queries,
               "freq": S.freq_queries, "main_scored": S.main_scored_queries, "consumers": consumer_queries, "consumers+scatter": consumer_scatter_queries, "rich": rich_queries}  # fmt: skip


# ---- plans ----------------------------------------------------------------------------------------------------------------------------------
def host_plan(hindex, queries, mode, options, cus=256, threads=2):
    flags, topk = MODES[mode]
    p = HP.HostPlan(hindex, S.programs(queries), flags, topk, threads=threads, options=options, cus=cus)
    assert p.s["unsupported_queries"] == 0, (options, p.last_unsupported)
    return p


def slot_tasks(p, slot):
    q = p.plan[slot]
    return p.tasks[int(q["first_task"]) : int(q["first_task"]) + int(q["ntasks"])]


def task_shapes(p, slot):
    """A slot's tasks without the batch-wide offsets: (kind, begin, end, offset within the query's region) — the region itself moves when an EARLIER query's capacity changes."""
    t = slot_tasks(p, slot)
    return [(int(k), int(b), int(e), int(o) - int(p.plan["out_off"][slot])) for k, b, e, o in zip(t["kind"], t["begin"], t["end"], t["out_off"])]


def kind_of_slot(p, slot):
    return int(slot_tasks(p, slot)["kind"][0])


def sched_section(p, kind):
    """The part of sched[] that holds the tasks of `kind`, in schedule order."""
    s = p.sched
    return s[p.tasks["kind"][s] == kind]


def scatter_slots(p):
    """Plan slots that run as a scatter union (their k_psets units carry PSET_UNIT_SCATTER)."""
    u = p.units
    return set(p.tasks["slot"][u["tix"][(u["first"] & PSET_UNIT_SCATTER) != 0]].tolist())


def same_slots(p0, p1):
    return p0.s["n_plan"] == p1.s["n_plan"] and np.array_equal(p0.slot_of_query, p1.slot_of_query) and np.array_equal(p0.plan["nphrases"], p1.plan["nphrases"])


# ---- the claims -----------------------------------------------------------------------------------------------------------------------------
def claim_phrase_task_div(div, but=()):
    """`but`: task kinds another option of the same set cuts anew (their phrase-less queries are that option's business)."""

    def claim(p0, p1):
        if not same_slots(p0, p1):
            return False
        phrase = np.flatnonzero(p0.plan["nphrases"] > 0).tolist()
        plain = [s for s in np.flatnonzero(p0.plan["nphrases"] == 0).tolist() if kind_of_slot(p0, s) not in but]
        if not phrase or not plain or p0.s["n_ptasks"] == p1.s["n_ptasks"] or np.array_equal(p0.plan["ntasks"][phrase], p1.plan["ntasks"][phrase]):
            return False
        if any(task_shapes(p0, s) != task_shapes(p1, s) for s in plain):  # queries without phrases keep their tasks
            return False
        width = {k: [e - b for s in phrase for kk, b, e, _ in task_shapes(p1, s) if kk == k] for k in (HP.TASK_PSET, HP.TASK_DENSE, HP.TASK_CAND)}
        if div == 1:  # the cut a large phrase batch gets: plane-set tasks of several windows, bitmap-window tasks of several windows, candidate tasks of several tiles
            return all(w and max(w) > 1 for w in width.values())
        if div >= PSET_TASK_WINDOWS:  # finer than a plane-set task can be cut: one window each
            return bool(width[HP.TASK_PSET]) and max(width[HP.TASK_PSET]) == 1
        return True

    return claim


def claim_dense_window_cost(value):
    def claim(p0, p1):
        if not same_slots(p0, p1):
            return False
        pset = [s for s in range(p0.s["n_plan"]) if kind_of_slot(p0, s) == HP.TASK_PSET]
        if any(task_shapes(p0, s) != task_shapes(p1, s) for s in pset):
            return False
        dense = [s for s in range(p0.s["n_plan"]) if kind_of_slot(p0, s) == HP.TASK_DENSE]
        if not dense or any(kind_of_slot(p1, s) != HP.TASK_DENSE for s in dense):
            return False
        if value == 0:  # a query the default cuts (its windows cost 16 K each whatever they hold) is ONE task over all its windows
            return any(len(task_shapes(p0, s)) > 1 and len(task_shapes(p1, s)) == 1 and task_shapes(p1, s)[0][2] - task_shapes(p1, s)[0][1] == sum(e - b for _, b, e, _ in task_shapes(p0, s)) for s in dense)
        one = all(e - b == 1 for s in dense for _, b, e, _ in task_shapes(p1, s))
        return one and any(e - b > 1 for s in dense for _, b, e, _ in task_shapes(p0, s))

    return claim


def claim_scatter_bitmap_slack(value):
    def claim(p0, p1):
        if not same_slots(p0, p1):
            return False
        s0, s1 = scatter_slots(p0), scatter_slots(p1)
        gained, lost = s1 - s0, s0 - s1
        want, other = (gained, lost) if value > 4 else (lost, gained)
        if not want or other:
            return False
        for s in want:  # a flip is between k_and_dense's ascending docIDs and the scatter union's bitmap, nothing else
            dense, scat = (p0, p1) if value > 4 else (p1, p0)
            if kind_of_slot(dense, s) != HP.TASK_DENSE or int(dense.plan["form"][s]) != RESULT_DOCIDS or kind_of_slot(scat, s) != HP.TASK_PSET or int(scat.plan["form"][s]) != RESULT_BITMAP:
                return False
        return True

    return claim


def claim_order(kinds, units):
    """The tasks are the same multiset — here: the same array —, the section of sched[] (and, for k_psets, unit_sched[]) of `kinds` another permutation of the same tasks."""

    def claim(p0, p1):
        if p0.tasks.tobytes() != p1.tasks.tobytes() or p0.units.tobytes() != p1.units.tobytes():
            return False
        moved = False
        for k in kinds:
            a, b = sched_section(p0, k), sched_section(p1, k)
            if sorted(a.tolist()) != sorted(b.tolist()):
                return False
            moved = moved or not np.array_equal(a, b)
        if units:
            a, b = p0.unit_sched, p1.unit_sched
            if sorted(a.tolist()) != sorted(b.tolist()) or np.array_equal(a, b):
                return False
        others = [k for k in HP.SCHED_ORDER if k not in kinds]
        return moved and all(np.array_equal(sched_section(p0, k), sched_section(p1, k)) for k in others)

    return claim


def claim_combined(p0, p1):
    """What a large phrase batch gets: phrase tasks uncut AND two ranges per k_planes query (a small batch gets three)."""
    if not claim_phrase_task_div(1, but=(HP.TASK_PLANES, HP.TASK_PLANES8))(p0, p1):
        return False
    planes = [s for s in range(p0.s["n_plan"]) if kind_of_slot(p0, s) in (HP.TASK_PLANES, HP.TASK_PLANES8)]
    return all(len(task_shapes(p1, s)) == 2 for s in planes) and (not planes or any(len(task_shapes(p0, s)) == 3 for s in planes))


def claim_launch_only(p0, p1):
    """overlap*: nothing in the plan changes (and HostPlan does not even know the names); the GPU file asserts the fork condition instead."""
    return p0.block.tobytes() == p1.block.tobytes()


VARIANTS = [
    ("auto", {}, None),  # the automatic choices that justify the forced values: test_plan_variants.py::test_auto_choices_equal_the_forced_values
    ("phrase_task_div=1", {"phrase_task_div": 1}, claim_phrase_task_div(1)),
    ("phrase_task_div=2", {"phrase_task_div": 2}, claim_phrase_task_div(2)),
    ("phrase_task_div=8", {"phrase_task_div": 8}, claim_phrase_task_div(8)),
    ("dense_window_cost=0", {"dense_window_cost": 0}, claim_dense_window_cost(0)),
    ("dense_window_cost=1M", {"dense_window_cost": 1 << 20}, claim_dense_window_cost(1 << 20)),
    ("scatter_bitmap_slack=1", {"scatter_bitmap_slack": 1}, claim_scatter_bitmap_slack(1)),
    ("scatter_bitmap_slack=64", {"scatter_bitmap_slack": 64}, claim_scatter_bitmap_slack(64)),
    ("pset_order=0", {"pset_order": 0}, claim_order([HP.TASK_PSET], True)),
    ("planes_order=0", {"planes_order": 0}, claim_order([HP.TASK_PLANES, HP.TASK_PLANES8], False)),
    ("planes_order=2", {"planes_order": 2}, claim_order([HP.TASK_PLANES, HP.TASK_PLANES8], False)),
    ("overlap", {"overlap": 1}, claim_launch_only),
    ("overlap_wgs=1,1", {"overlap_dense_wgs": 1, "overlap_cand_wgs": 1}, claim_launch_only),
    ("overlap_wgs=2,3", {"overlap_dense_wgs": 2, "overlap_cand_wgs": 3}, claim_launch_only),
    ("large_phrase_batch", {"phrase_task_div": 1, "planes_split": 2}, claim_combined),
]
NAMES = [v[0] for v in VARIANTS]
OPTIONS = {v[0]: v[1] for v in VARIANTS}
CLAIMS = {v[0]: v[2] for v in VARIANTS}
LAUNCH_OPTIONS = ("overlap", "overlap_dense_wgs", "overlap_cand_wgs")  # read by tri_batch_run, unknown to the host planner
LAUNCH_VARIANTS = [n for n in NAMES if OPTIONS[n] and set(OPTIONS[n]) <= set(LAUNCH_OPTIONS)]
LAYOUTS = [{}] + [OPTIONS[n] for n in LAUNCH_VARIANTS]  # the stream layouts the consumers are run under
PLAN_VARIANTS = [n for n in NAMES if OPTIONS[n] and n not in LAUNCH_VARIANTS]
PHRASE_VARIANTS = [n for n in NAMES if "phrase_task_div" in OPTIONS[n]] + LAUNCH_VARIANTS
SCORED_VARIANTS = [n for n in NAMES if n.startswith(("planes_order", "pset_order"))] + LAUNCH_VARIANTS
TALL_VARIANTS = ["dense_window_cost=0", "dense_window_cost=1M", "phrase_task_div=1"]

# (corpus, query list, mode, base options) on which a variant's claim holds: the GPU file runs every one of them
_PHRASE_CASES = [("stream", "stream", "docs", PHRASE_MIX), ("stream", "stream", "scored", PHRASE_MIX), ("stream", "stream_phrases", "rich", PHRASE_MIX)]
CLAIM_CASES = {
    "phrase_task_div=1": _PHRASE_CASES,
    "phrase_task_div=2": _PHRASE_CASES,
    "phrase_task_div=8": _PHRASE_CASES,
    "large_phrase_batch": _PHRASE_CASES,
    "dense_window_cost=0": [("tall", "tall", "docs", {}), ("tall", "tall", "docs", ALL_WINDOWS), ("tall", "tall_scored", "scored", MATCH_THEN_SCORE), ("tall", "tall_rich", "rich", {})],
    "dense_window_cost=1M": [("tall", "tall", "docs", {}), ("tall", "tall", "docs", ALL_WINDOWS), ("tall", "tall_scored", "scored", MATCH_THEN_SCORE), ("tall", "tall_rich", "rich", {}),
                             ("main", "main+unions", "docs", {}), ("main", "rich", "rich", {})],
    "scatter_bitmap_slack=1": [("main", "main+unions", "docs", {}), ("main", "unions", "docs", {"plane_div": SCATTER_PLANE_DIV})],
    "scatter_bitmap_slack=64": [("main", "main+unions", "docs", {}), ("main", "unions", "docs", {"plane_div": SCATTER_PLANE_DIV})],
    "pset_order=0": [("main", "main+unions", "docs", {}), ("main", "main_scored", "scored", {"dense_min_postings": 0, "fused": 0}), ("freq", "freq", "scored", {"dense_min_postings": 0, "fused": 0})],
    "planes_order=0": [("main", "main_scored", "scored", {}), ("freq", "freq", "scored", {"dense_min_postings": 0}), ("freq", "freq", "scored", {"dense_min_postings": 0, "planes_split": 7})],
    "planes_order=2": [("main", "main_scored", "scored", {}), ("freq", "freq", "scored", {"dense_min_postings": 0}), ("freq", "freq", "scored", {"dense_min_postings": 0, "planes_split": 7})],
}
# the scored option sets of the order and stream-layout variants: what reaches k_planes, both k_fused word widths, and match-then-score (k_psets + k_and + k_and_dense)
SCORED_BASES = [{}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes_split": 7}, {"dense_min_postings": 0, "planes": 0}, {"dense_min_postings": 0, "planes": 0, "fused_halfwords": 0},
                {"dense_min_postings": 0, "fused": 0}]  # fmt: skip
# phrase_task_div on a list whose EVERY phrase query is bitmap windows: seams at the first window boundary, where the stream corpus' head terms all hold documents
SEAM_CASES = {n: _PHRASE_CASES[:1] + [("stream", "stream", "docs", ALL_WINDOWS)] for n in ("phrase_task_div=1", "phrase_task_div=2", "phrase_task_div=8", "large_phrase_batch")}
SEAM_CASES.update({n: CLAIM_CASES[n][:2] for n in ("dense_window_cost=0", "dense_window_cost=1M")})


# ---- the scatter rule restated from the postings ----------------------------------------------------------------------------------------------
def scatter_sides(c, texts, slack, plane_div=1024):
    """[(text, left, right, mixed)] of  min(N, head documents) x slack >= windows x SPAN_WORDS  (planner_tasks.hpp route_cnf) for pure unions over list names, from the postings:
    a head term holds at least docs_cnt / plane_div documents (planner.hpp eligible_planes); the windows are those up to the union's last document; mixed: the
    union holds head terms AND others (the only unions the rule is asked about)."""
    out = []
    min_df = max(1, c.docs_cnt // plane_div)
    for t in texts:
        names = [x.strip("{} ") for x in t.split(" OR ")]
        df = [c.lists[n][0].size for n in names]
        head = sum(d for d in df if d >= min_df)
        nwin = max(int(c.lists[n][0][-1]) for n in names) // S.SPAN_BITS + 1
        out.append((t, min(c.docs_cnt, head) * max(1, slack), nwin * SPAN_WORDS, 0 < head and any(d < min_df for d in df)))
    return out


# ---- seams: the documents on both sides of the cut between two tasks of a query ------------------------------------------------------------------
def seam_documents(c, p, slot):
    """[(last docID of a task's range, first docID of the next task's)] of a slot's window tasks (ranges of SPAN_BITS windows) and candidate-tile tasks (ranges of
    TILE_BLOCKS blocks of the lead list: the documents come from the postings)."""
    t = slot_tasks(p, slot)
    kind = int(t["kind"][0])
    out = []
    if kind in (HP.TASK_DENSE, HP.TASK_PSET):
        out = [(int(e) * S.SPAN_BITS - 1, int(e) * S.SPAN_BITS) for e in t["end"][:-1]]
    elif kind == HP.TASK_CAND:
        lead = c.lists[c.names[int(p.qterms[int(p.plan["term_base"][slot])]) & QT_TERM]][0]
        out = [(int(lead[int(e) * S.TILE_DOCS - 1]), int(lead[int(e) * S.TILE_DOCS])) for e in t["end"][:-1]]
    return out


def seams_reached(c, p, queries, want):
    """(queries with a match on the last docID before a seam, queries with one on the first docID after a seam, seams) over the callers' queries of a plan."""
    before = after = seams = 0
    for qi in range(len(queries)):
        sd = seam_documents(c, p, int(p.slot_of_query[qi]))
        seams += len(sd)
        if sd:
            w = np.asarray(want[qi])
            before += bool(np.isin([lo for lo, _ in sd], w).any())
            after += bool(np.isin([hi for _, hi in sd], w).any())
    return before, after, seams
