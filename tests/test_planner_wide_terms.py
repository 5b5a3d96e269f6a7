"""CPU tests of the planner's WIDE-REPORT queries (no GPU): default-mode queries of 17 .. 64 reportable terms behind option rich_max_terms — what is left out
at which setting, the 64-bit report mask of a leaf (a phrase whose terms fall on both sides of bit 32), the side table of rows and strides, k_rich's own
schedule, and that the narrow queries of a mixed batch are planned as they are alone.  Same small world as tests/test_planner_wide.py."""
import numpy as np
import pytest

import oracle_lib as O
import trinity_amd as T
from trinity_amd import hostplan as HP

from wide_terms_cases import NARROW, OPTS, OR65, SHAPES, mixed_programs, narrow_programs, shape_programs

OP_TERM, OP_AND, OP_OR, OP_PHRASE, OP_NOT, OP_OPT, OP_SOME = range(7)
RICH = T.FLAG_MATCHED_TERMS


@pytest.fixture(scope="module")
def world():
    T.build.build_host()
    seg = T.Segment(200_000, 20_000, 10, 42, codec=T.engine.CODEC_GOOGLE)
    return HP.HostIndex.from_segment(seg)


def test_default_options_leave_every_shape_out(world):
    for (name, *_), prog in zip(SHAPES, shape_programs(O)):
        p = HP.HostPlan(world, [prog, O.parse_query("t0 t1")], RICH, options={"tree_max_nodes": 1024})
        assert p.qstatus[:2].tolist() == [-3, 0] and p.s["unsupported_queries"] == 1, name
        assert "more than 16 reportable terms" in p.last_unsupported, (name, p.last_unsupported)
        assert p.s["n_rich_wide_tab"] == 0 and p.s["n_rich_wide"] == 0
        p.close()


def test_every_shape_is_lowered_at_64(world):
    progs = shape_programs(O)
    p = HP.HostPlan(world, progs, RICH, options=OPTS)
    assert not p.qstatus[: len(progs)].any() and p.s["unsupported_queries"] == 0 and p.s["tree_queries"] == len(progs)
    slots = p.slot_of_query[: len(progs)]
    assert p.plan["nscore"][slots].tolist() == [sh[3] for sh in SHAPES] == [17, 33, 64, 41, 60, 40, 42, 54]
    assert p.s["rich_R"] == 0  # (no narrow query: the batch-wide row width is not raised)
    # the side table: strides are nscore rounded up to 8, rows and mask slots of the queries follow one another without overlap
    rw = p.rich_wide
    assert len(rw) == p.s["n_plan"] and p.s["n_rich_wide"] == len(progs)
    cells = slots_at = 0
    for sl in range(p.s["n_plan"]):
        q = p.plan[sl]
        if sl in slots:
            stride = (int(q["nscore"]) + 7) // 8 * 8
            assert (int(rw[sl]["stride"]), int(rw[sl]["cells"]), int(rw[sl]["slots"])) == (stride, cells, slots_at), sl
            assert cells % 8 == 0  # 16-byte rows
            cells += int(q["out_cap"]) * stride
            slots_at += int(q["out_cap"])
        else:  # (a hidden phrase query)
            assert int(rw[sl]["stride"]) == 0 and int(q["nscore"]) == 0
    assert (p.s["rich_wide_cells"], p.s["rich_wide_slots"]) == (cells, slots_at)
    # every positive leaf's mask: one bit per term leaf, the OR of its terms' bits per phrase leaf; together every reportable term
    for i, sh in enumerate(SHAPES):
        sl = int(slots[i])
        kind, n = p.tree_kind(sl)
        assert (kind == HP.TREE_KIND_WIDE) == (n > 64), sh[0]
        nd = p.tree_nodes_wide(sl) if kind == HP.TREE_KIND_WIDE else p.tree_nodes(sl)
        sterms = p._view("off_sterms", p.s["n_sterms"], "<u4")[int(p.plan[sl]["score_base"]) :][: sh[3]].tolist()
        seen = 0
        for k in range(n):
            m = p.leaf_report_mask(sl, k)
            if nd[k]["op"] == OP_TERM and m:
                assert m == 1 << sterms.index(int(nd[k]["arg"])), (sh[0], k)
            elif nd[k]["op"] not in (OP_TERM, OP_PHRASE):
                assert kind == HP.TREE_KIND_NARROW or m == 0
                continue
            seen |= m
        assert seen == (1 << sh[3]) - 1, sh[0]
    p.close()


def test_a_phrase_leaf_carries_bits_on_both_sides_of_bit_32(world):
    name, text, mn, nscore, *_ = SHAPES[-1]
    assert name == "straddle"
    for opts in (OPTS, dict(OPTS, tree_wide_min_nodes=0)):  # the narrow record (the high word in the leaf's `kids`) and the wide one (`pad`)
        p = HP.HostPlan(world, [O.parse_query(text, some_min=mn)], RICH, options=opts)
        sl = int(p.slot_of_query[0])
        wide = p.tree_kind(sl)[0] == HP.TREE_KIND_WIDE
        assert wide == ("tree_wide_min_nodes" in opts)
        nd = p.tree_nodes_wide(sl) if wide else p.tree_nodes(sl)
        phrases = [k for k in range(len(nd)) if nd[k]["op"] == OP_PHRASE]
        assert len(phrases) == 2
        assert p.leaf_report_mask(sl, phrases[0]) == (1 << 31) | (1 << 32)  # "t0 t1"
        assert p.leaf_report_mask(sl, phrases[1]) == (1 << 32) | (1 << 33)  # "t1 t2"
        sterms = p._view("off_sterms", p.s["n_sterms"], "<u4")[int(p.plan[sl]["score_base"]) :][:nscore].tolist()
        assert sterms[31:34] == [0, 1, 2]
        p.close()


def test_a_65th_term_is_left_out_and_the_message_names_the_limit(world):
    p = HP.HostPlan(world, [O.parse_query(OR65), O.parse_query(SHAPES[2][1])], RICH, options=OPTS)
    assert p.qstatus[:2].tolist() == [-3, 0] and "more than 64 reportable terms" in p.last_unsupported
    p.close()
    or17, or33 = (O.parse_query(SHAPES[i][1]) for i in (0, 1))
    p = HP.HostPlan(world, [or17, or33], RICH, options={"rich_max_terms": 32})
    assert p.qstatus[:2].tolist() == [0, -3] and "more than 32 reportable terms" in p.last_unsupported
    p.close()


@pytest.mark.parametrize("value", [15, 65])
def test_rich_max_terms_is_validated(world, value):
    with pytest.raises(T.TrinityError, match="rich_max_terms"):
        HP.HostPlan(world, [O.parse_query("t0 t1")], RICH, options={"rich_max_terms": value})


def test_other_modes_are_untouched_by_the_option(world):
    """DocumentsOnly and scored batches have no reportable terms: the same block with and without the option."""
    progs = shape_programs(O) + narrow_programs(O)
    for flags, topk in ((T.FLAG_DOCUMENTS_ONLY, 0), (T.FLAG_ACCUMULATED_SCORE, 10)):
        a = HP.HostPlan(world, progs, flags, topk, options={"tree_max_nodes": 1024})
        b = HP.HostPlan(world, progs, flags, topk, options=OPTS)
        assert bytes(a.block) == bytes(b.block) and a.s == b.s and b.s["n_rich_wide_tab"] == 0
        a.close(), b.close()


def narrow_facts(p, qi):
    """What the kernels read of caller query qi, free of the places the batch gave it: its DevQuery's shape, its term lists, its tasks' kinds and spans, its tree
    record (rows and phrase slots are batch-relative: compared through the term / the hidden query's own terms)."""
    sl = int(p.slot_of_query[qi])
    q = p.plan[sl]
    facts = {f: int(q[f]) for f in ("nterms", "out_cap", "ntasks", "nscore", "nphrases", "form")}
    facts["qterms"] = p.qterms[int(q["term_base"]) :][: int(q["nterms"])].tolist()
    facts["sterms"] = p._view("off_sterms", p.s["n_sterms"], "<u4")[int(q["score_base"]) :][: int(q["nscore"])].tolist()
    tk = p.tasks[int(q["first_task"]) :][: int(q["ntasks"])]
    facts["tasks"] = [(int(t["kind"]), int(t["begin"]), int(t["end"]), int(t["out_off"]) - int(q["out_off"])) for t in tk]
    if int(tk[0]["kind"]) == HP.TASK_TREE:
        assert p.tree_kind(sl)[0] == HP.TREE_KIND_NARROW
        nd = p.tree_nodes(sl)
        tree_terms = p.tree_terms
        rec = []
        for x in nd:
            leaf = (int(tree_terms[int(x["row"])]) if x["op"] == OP_TERM else narrow_facts_hidden(p, int(x["arg"]))) if x["op"] in (OP_TERM, OP_PHRASE) else None
            rec.append((int(x["op"]), int(x["parent"]), int(x["ord"]), int(x["thr"]), int(x["arg"]) if x["op"] == OP_TERM else 0, int(x["score"]), int(x["rmask"]),
                        int(x["kid0"]), int(x["kid1"]), int(x["kids"]), leaf))  # fmt: skip
        facts["tree"] = rec
    return facts


def narrow_facts_hidden(p, slot):
    q = p.plan[slot]
    return (int(q["out_cap"]), tuple(p.qterms[int(q["term_base"]) :][: int(q["nterms"])].tolist()))


def test_a_mixed_batch_plans_its_narrow_queries_as_they_are_planned_alone(world):
    mixed, narrow_at = mixed_programs(O)
    alone = HP.HostPlan(world, narrow_programs(O), RICH)
    both = HP.HostPlan(world, mixed, RICH, options=OPTS)
    assert not both.qstatus[: len(mixed)].any() and not alone.qstatus[: len(NARROW)].any()
    assert both.s["rich_R"] == alone.s["rich_R"] == 12  # the widest NARROW query's count, not 64
    for j, qi in enumerate(narrow_at):
        assert narrow_facts(both, qi) == narrow_facts(alone, j), NARROW[j]
        assert int(both.rich_wide[int(both.slot_of_query[qi])]["stride"]) == 0
    # the output regions tile the capacity as ever
    plan = both.plan
    assert np.array_equal(plan["out_off"], np.concatenate([[0], np.cumsum(plan["out_cap"].astype(np.uint64))[:-1]]).astype(np.uint64))
    # the side table: wide rows and mask slots do not overlap
    rw = both.rich_wide
    wide_slots = [int(both.slot_of_query[qi]) for qi in range(len(mixed)) if qi not in narrow_at]
    spans = sorted((int(rw[sl]["cells"]), int(rw[sl]["cells"]) + int(plan[sl]["out_cap"]) * int(rw[sl]["stride"])) for sl in wide_slots)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == both.s["rich_wide_cells"]
    mspans = sorted((int(rw[sl]["slots"]), int(rw[sl]["slots"]) + int(plan[sl]["out_cap"])) for sl in wide_slots)
    assert all(a[1] <= b[0] for a, b in zip(mspans, mspans[1:])) and mspans[-1][1] == both.s["rich_wide_slots"]
    for sl in wide_slots:
        assert int(rw[sl]["stride"]) == (int(plan[sl]["nscore"]) + 7) // 8 * 8
    # k_rich's schedule: a permutation of the tasks, the wide-report queries' tasks — and only they — at its end, each part in sched's order
    rs, sched, tasks = both.rich_sched, both.sched, both.tasks
    nw = both.s["n_rich_wide"]
    assert nw == len(wide_slots) and np.array_equal(np.sort(rs), np.arange(both.s["n_tasks"], dtype=np.uint32))
    is_wide = np.isin(tasks["slot"][rs], wide_slots)
    assert not is_wide[: len(rs) - nw].any() and is_wide[len(rs) - nw :].all()
    order = {int(t): i for i, t in enumerate(sched)}
    for part in (rs[: len(rs) - nw], rs[len(rs) - nw :]):
        assert np.all(np.diff([order[int(t)] for t in part]) > 0)
    # ... and the same block on one thread and on four
    four = HP.HostPlan(world, mixed, RICH, threads=4, options=OPTS)
    assert bytes(four.block) == bytes(both.block) and four.s == both.s
    for p in (alone, both, four):
        p.close()


def test_a_batch_of_narrow_queries_is_the_same_block_whatever_the_option_says(world):
    progs = narrow_programs(O) * 40
    a = HP.HostPlan(world, progs, RICH)
    b = HP.HostPlan(world, progs, RICH, options={"rich_max_terms": 64})
    assert bytes(a.block) == bytes(b.block) and a.s == b.s and np.array_equal(a.qstatus, b.qstatus)
    a.close(), b.close()
