"""CPU tests of the planner's WIDE tree records (no GPU): trees of more than 64 nodes behind option tree_max_nodes, the record k_tree_wide.hpp's
kernels read (csrc/dev_structs.hpp DevTreeNodeW), its header's stack figures, the narrow / wide split of the schedule's TASK_TREE section, and what
is still left out.  Same small world as tests/test_planner.py."""
import numpy as np
import pytest

import oracle_lib as O
import trinity_amd as T
from trinity_amd import hostplan as HP

OP_TERM, OP_AND, OP_OR, OP_PHRASE, OP_NOT, OP_OPT, OP_SOME = range(7)
WIDE = {"tree_max_nodes": 1024}
BIG = " OR ".join(f"(t{2 * i} t{2 * i + 1})" for i in range(40))  # 40 conjunctions under an OR: 121 nodes
# (tests/test_gpu_parity.py's list: the trees no other kernel takes)
WIDE_TREES = ['t0 OR "t1 t2"', 't0 NOT ("t1 t2" t3)', "t0 OR (t1 t2) OR (t3 t4) OR (t5 t6) OR (t7 t8)", '[t0, "t1 t2", t3 t4, "t5 t6 t7"]', '"t0 t1" OR "t1 t2" OR "t2 t3"',
              "(t0 OR t1) (t2 OR t3) (t4 OR t5) (t6 OR t7) (t8 OR t9) (t10 OR t11) (t12 OR t13) (t14 OR t15) (t16 OR t17)", 't0 <"t1 t2">', '("t0 t1" OR t2) NOT "t3 t4"',
              "[t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11]", "t0 t1 t2 t3 t4 t5 t6 t7 t8 t9 t10 t11 t12 t13 t14 t15 t16 t17",
              't20 OR ((t0 OR "t1 t2") (t3 OR t4 OR t5) NOT (t6 "t7 t8"))']  # fmt: skip


@pytest.fixture(scope="module")
def world():
    T.build.build_host()
    seg = T.Segment(200_000, 20_000, 10, 42, codec=T.engine.CODEC_GOOGLE)
    return HP.HostIndex.from_segment(seg)


def tree_slots(p):
    plan, tasks = p.plan, p.tasks
    return [int(sl) for sl in np.nonzero(tasks["kind"][plan["first_task"]] == HP.TASK_TREE)[0]]


def planes(nkids):
    return int(nkids).bit_length()  # ceil(log2(nkids + 1))


def check_wide_record(p, sl):
    """A wide record: postfix order, one root, every child knows its parent's operator and planes; the header's two figures recomputed from the nodes — per
    root-to-leaf path a word per open AND / OR / NOT / OPT ancestor, its counter planes per open matchsome; the deepest path decides."""
    kind, n = p.tree_kind(sl)
    assert kind == HP.TREE_KIND_WIDE
    nd, hdr = p.tree_nodes_wide(sl), p.tree_header(sl)
    assert len(nd) == n == int(hdr[0]) and np.all(hdr[4:] == 0)
    par = nd["parent"].astype(np.int64)
    assert par[-1] == HP.TREE_NO_PARENT and np.all(par[:-1] > np.arange(n - 1)) and np.all(par[:-1] < n)
    kids = [[] for _ in range(n)]
    for k in range(n - 1):
        kids[par[k]].append(k)
    words, depth = np.zeros(n, np.int64), np.zeros(n, np.int64)
    stack = deep = 0
    for k in range(n - 1, -1, -1):
        x = nd[k]
        leaf = x["op"] in (OP_TERM, OP_PHRASE)
        assert int(x["nkids"]) == len(kids[k]) and leaf == (not kids[k])
        assert sorted(nd["ord"][kids[k]].tolist()) == list(range(len(kids[k])))
        assert int(x["cbits"]) == (planes(x["nkids"]) if x["op"] == OP_SOME else 0)
        if x["op"] == OP_SOME:
            assert 1 <= int(x["thr"]) <= int(x["nkids"])
        if x["op"] in (OP_NOT, OP_OPT):
            assert len(kids[k]) == 2
        if k < n - 1:
            px = nd[par[k]]
            assert x["pop"] == px["op"] and x["pcbits"] == px["cbits"]
            words[k] = words[par[k]] + (int(px["cbits"]) if px["op"] == OP_SOME else 1)
            depth[k] = depth[par[k]] + 1
        if leaf:
            stack, deep = max(stack, int(words[k])), max(deep, int(depth[k]))
    assert (int(hdr[2]), int(hdr[3])) == (stack, deep) and stack <= 64
    return n


def test_a_tree_of_121_nodes_is_lowered_as_a_wide_record(world):
    """THE feature: `big` at tree_max_nodes = 1024 — status 0, a tree query, a wide record of 121 nodes; over 700 copies mixed with narrow trees and CNFs the
    plan is the same block on one thread and on four, and the TASK_TREE section runs its narrow records first."""
    prog = O.parse_query(BIG)
    p = HP.HostPlan(world, [prog], T.FLAG_DOCUMENTS_ONLY, options=WIDE)
    assert p.qstatus[:1].tolist() == [0] and p.s["tree_queries"] == 1 and p.s["unsupported_queries"] == 0
    (sl,) = tree_slots(p)
    assert p.tree_kind(sl) == (HP.TREE_KIND_WIDE, 121) and check_wide_record(p, sl) == 121
    p.close()
    texts = [BIG, WIDE_TREES[2], "t0 t1", WIDE_TREES[8], "t3 OR t5 OR t9"]
    progs = [O.parse_query(t, some_min=2) for t in texts] * 700
    for flags, topk in ((T.FLAG_DOCUMENTS_ONLY, 0), (T.FLAG_ACCUMULATED_SCORE, 10)):
        plans = [HP.HostPlan(world, progs, flags, topk, threads=thr, options=WIDE) for thr in (1, 4)]
        a, b = plans
        assert bytes(a.block) == bytes(b.block) and a.s == b.s and np.array_equal(a.slot_of_query, b.slot_of_query)
        assert not a.qstatus[: len(progs)].any() and a.s["tree_queries"] == 3 * 700 == a.s["n_tree"]
        sched, tasks = a.sched, a.tasks
        sec = sched[a.s["n_tasks"] - a.s["n_tree"] :]  # (the last section)
        assert np.all(tasks["kind"][sec] == HP.TASK_TREE)
        wide = np.array([a.tree_kind(int(tasks["slot"][ti]))[0] for ti in sec])
        assert int(wide.sum()) == 700 and np.all(wide[:1400] == 0) and np.all(wide[1400:] == 1)
        # (stable: equal trees cost the same, so each part keeps the batch's order)
        assert np.all(np.diff(sec[1400:].astype(np.int64)) > 0)
        for q in a, b:
            q.close()


def test_default_options_still_leave_it_out(world):
    p = HP.HostPlan(world, [O.parse_query(BIG), O.parse_query("t0 t1")], T.FLAG_DOCUMENTS_ONLY)
    assert p.qstatus[:2].tolist() == [-3, 0] and p.s["unsupported_queries"] == 1 and p.s["tree_queries"] == 0
    p.close()


@pytest.mark.parametrize("value", [63, 1025, 0])
def test_tree_max_nodes_is_validated(world, value):
    with pytest.raises(T.TrinityError, match="tree_max_nodes"):
        HP.HostPlan(world, [O.parse_query("t0 t1")], T.FLAG_DOCUMENTS_ONLY, options={"tree_max_nodes": value})


def flat_or(n, first=0):
    return np.array([T.tok(T.OP_TERM, first + i) for i in range(n)] + [T.tok(T.OP_OR, n)], dtype=np.uint32)


def test_a_tree_of_more_than_1024_nodes_is_left_out(world):
    """1023 terms under an OR are 1024 nodes: lowered.  1024 terms are 1025: left out, the reason names the limit in force."""
    p = HP.HostPlan(world, [flat_or(1023), flat_or(1024)], T.FLAG_DOCUMENTS_ONLY, options=WIDE)
    assert p.qstatus[:2].tolist() == [0, -3] and p.s["tree_queries"] == 1
    assert p.tree_kind(tree_slots(p)[0]) == (HP.TREE_KIND_WIDE, 1024)
    assert "a tree of more than 1024 nodes" in p.last_unsupported
    p.close()
    p = HP.HostPlan(world, [flat_or(200)], T.FLAG_DOCUMENTS_ONLY, options={"tree_max_nodes": 128})
    assert p.qstatus[:1].tolist() == [-3] and "a tree of more than 128 nodes" in p.last_unsupported
    p.close()
    p = HP.HostPlan(world, [flat_or(200)], T.FLAG_DOCUMENTS_ONLY)
    assert p.qstatus[:1].tolist() == [-3] and "a tree of more than 64 nodes" in p.last_unsupported
    p.close()


def nested_some(levels, width, first=0):
    """`levels` matchsomes, each over width - 1 terms and the next one (the innermost: width terms): nested along one child only."""
    prog, t = [], first
    for lv in range(levels):
        n = width if lv == 0 else width - 1
        prog += [T.tok(T.OP_TERM, t + i) for i in range(n)]
        t += n
        prog.append(T.tok(T.OP_SOME, (2 << 16) | width))
    return np.array(prog, dtype=np.uint32)


def test_a_tree_that_needs_more_than_64_stack_words_is_left_out(world):
    """Ten nested matchsomes of 100 children each: 1001 nodes, seven counter planes a level, 70 words on the deepest path — left out.  Nine of them need 63: lowered.
    (Planes grow with log2 of the children, nodes with the children themselves: within 1024 nodes it is depth, not width, that passes 64 words.)"""
    p = HP.HostPlan(world, [nested_some(10, 100), nested_some(9, 100)], T.FLAG_DOCUMENTS_ONLY, options=WIDE)
    assert p.qstatus[:2].tolist() == [-3, 0] and "more than 64 words of evaluation stack" in p.last_unsupported
    (sl,) = tree_slots(p)
    assert check_wide_record(p, sl) == 9 * 100 + 1 and int(p.tree_header(sl)[2]) == 63 and int(p.tree_header(sl)[3]) == 9
    p.close()


@pytest.mark.parametrize("flags,topk", [(T.FLAG_DOCUMENTS_ONLY, 0), (T.FLAG_ACCUMULATED_SCORE, 10), (T.FLAG_MATCHED_TERMS, 0)])
def test_forced_wide_records_and_their_headers(world, flags, topk):
    """tree_wide_min_nodes = 0: every tree query of WIDE_TREES gets a wide record — same nodes, same leaves (term, row, scorer, reportable terms) as its narrow one —
    and the header's stack and counter-depth figures are what the record's own nodes give."""
    progs = [O.parse_query(t, some_min=2) for t in WIDE_TREES]
    narrow = HP.HostPlan(world, progs, flags, topk)
    forced = HP.HostPlan(world, progs, flags, topk, options={"tree_wide_min_nodes": 0})
    assert np.array_equal(narrow.qstatus, forced.qstatus) and narrow.s["tree_queries"] == forced.s["tree_queries"] >= len(WIDE_TREES) - 2
    assert tree_slots(narrow) == tree_slots(forced)
    for sl in tree_slots(forced):
        assert narrow.tree_kind(sl)[0] == HP.TREE_KIND_NARROW
        n = check_wide_record(forced, sl)
        a, b = narrow.tree_nodes(sl), forced.tree_nodes_wide(sl)
        assert len(a) == n
        for f in ("op", "arg", "row", "score", "rmask", "ord"):
            assert np.array_equal(a[f], b[f]), f
        assert np.array_equal(a["parent"][:-1], b["parent"][:-1]) and np.array_equal(a["thr"], b["thr"])
    assert np.array_equal(narrow.plan, forced.plan) and np.array_equal(narrow.tasks, forced.tasks)
    narrow.close(), forced.close()


def test_thresholds_above_255_are_carried(world):
    """A matchsome of 300 alternatives that wants 260 of them: the record says 260 (the narrow record's byte would have said 255)."""
    prog = np.array([T.tok(T.OP_TERM, i) for i in range(300)] + [T.tok(T.OP_SOME, (260 << 16) | 300)], dtype=np.uint32)
    p = HP.HostPlan(world, [prog], T.FLAG_DOCUMENTS_ONLY, options=WIDE)
    assert p.qstatus[:1].tolist() == [0]
    nd = p.tree_nodes_wide(tree_slots(p)[0])
    assert int(nd["thr"][-1]) == 260 and int(nd["cbits"][-1]) == 9 and int(nd["nkids"][-1]) == 300
    p.close()
