"""CPU checks of tests/plan_variants.py, the table tests/test_gpu_plan_variants.py runs on the device: every variant's claim holds on the corpus, query list, mode and
base options the GPU file uses for it, in both codecs — and is FALSE between two default plans, so a variant whose option was dropped or mistyped cannot pass —; the
query lists have matching documents on both sides of the seams of the variant's cut; unions sit on both sides of the scatter rule at slack 1, 4 and 64; the planner's
automatic choices produce, byte for byte, the plans of the forced values the GPU file runs; tree_max_bytes refuses one byte below the documented need and accepts the
need itself; the consumers' batches hold the kinds of queries run_matching's fork conditions ask for."""
import os
import re

import pytest

import consumer_tree_cases as CT
import plan_variants as V
import structured as S
import trinity_amd as T
from trinity_amd import hostplan as HP

PLK_WGS_PER_CU = 2  # planner_types.hpp PlanEnv::plk_wgs_per_cu, the k_planes workgroups a compute unit holds (test_the_table_names_real_options_and_flags reads it back)


@pytest.fixture(scope="module")
def corpora():
    T.build.build_host()
    made = {}

    def get(name):
        if name not in made:
            made[name] = S.CORPORA[name]()
        return made[name]

    return get


@pytest.fixture(scope="module")
def hindex(corpora):
    made = {}

    def get(name, codec):
        if (name, codec) not in made:
            made[name, codec] = corpora(name).host_index(codec)
        return made[name, codec]

    yield get
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def wants(corpora):
    """numpy docID sets of a (corpus, query list), evaluated once"""
    made = {}

    def get(name, key):
        if (name, key) not in made:
            c = corpora(name)
            made[name, key] = [c.evaluate(p) for p in S.programs(V.QUERY_LISTS[key](c))]
        return made[name, key]

    return get


def pair(corpora, hindex, case, codec, options):
    name, key, mode, base = case
    queries = V.QUERY_LISTS[key](corpora(name))
    return V.host_plan(hindex(name, codec), queries, mode, base), V.host_plan(hindex(name, codec), queries, mode, dict(base, **options))


def test_the_table_names_real_options_and_flags():
    assert (V.FLAG_DOCS, V.FLAG_SCORED, V.FLAG_RICH) == (T.FLAG_DOCUMENTS_ONLY, T.FLAG_ACCUMULATED_SCORE, T.FLAG_MATCHED_TERMS)
    assert len(set(V.NAMES)) == len(V.NAMES) == 15 and V.OPTIONS["auto"] == {}
    assert re.search(r"plk_wgs_per_cu = (\d+);", open(os.path.join(S.CSRC, "planner_types.hpp")).read()).group(1) == str(PLK_WGS_PER_CU)
    hip = open(os.path.join(S.CSRC, "trinity_hip.hip")).read()
    table = set(re.findall(r'\{"(\w+)", &tri_options::\w+\}', hip))  # tri_dev_set_option's table: a name it lacks fails the GPU file's first set_option
    for name, options, _ in V.VARIANTS:
        assert set(options) <= table, (name, set(options) - table)
    for base in [V.PHRASE_MIX, V.ALL_WINDOWS] + V.SCORED_BASES + [b for cases in V.CLAIM_CASES.values() for *_, b in cases]:
        assert set(base) <= table, base
    assert set(V.PLAN_VARIANTS) == set(V.CLAIM_CASES) and set(V.LAUNCH_VARIANTS) == {"overlap", "overlap_wgs=1,1", "overlap_wgs=2,3"} and len(V.LAYOUTS) == 4


def test_the_host_planner_knows_every_option(corpora, hindex):
    """An option name csrc/host/plan_host.cpp does not know raises: a typo cannot turn a variant into the default plan."""
    c = corpora("phrase")
    for name, options, _ in V.VARIANTS:
        V.host_plan(hindex("phrase", 1), S.phrase_queries(c), "docs", options).close()
    with pytest.raises(T.engine.TrinityError, match="unknown option phrase_task_dvi"):
        V.host_plan(hindex("phrase", 1), S.phrase_queries(c), "docs", {"phrase_task_dvi": 1})


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", V.PLAN_VARIANTS)
def test_claims_hold_and_fail_without_the_option(corpora, hindex, name, codec):
    """On every case the GPU file runs for the variant: the claim is true of (default plan, variant's plan) and false of (default plan, default plan)."""
    for case in V.CLAIM_CASES[name]:
        p0, p1 = pair(corpora, hindex, case, codec, V.OPTIONS[name])
        again = V.host_plan(hindex(case[0], codec), V.QUERY_LISTS[case[1]](corpora(case[0])), case[2], case[3])
        assert V.CLAIMS[name](p0, p1), (name, case)
        assert not V.CLAIMS[name](p0, again), (name, case)
        assert p0.block.tobytes() == again.block.tobytes()  # (planning is deterministic: the comparison above compares options, not runs)


@pytest.mark.parametrize("name", V.LAUNCH_VARIANTS)
def test_launch_options_leave_the_plan_alone(corpora, hindex, name):
    for key, mode in (("consumers+scatter", "docs"), ("rich", "rich"), ("main_scored", "scored")):
        p0, p1 = pair(corpora, hindex, ("main", key, mode, {}), 1, V.OPTIONS[name])
        assert V.CLAIMS[name](p0, p1), (name, key)


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("name", sorted(V.SEAM_CASES))
def test_matches_on_both_sides_of_the_variants_seams(corpora, hindex, wants, name, codec):
    """Under the VARIANT's cut, from the plan's begin / end and the postings: some query has a matching document on the last docID of one task's range, some query
    one on the first docID of the next task's — and the cut has seams the default cut has not, or lacks seams the default has.  Asserted for EACH of the variant's lists."""
    changed = False
    for case in V.SEAM_CASES[name]:
        c = corpora(case[0])
        queries = V.QUERY_LISTS[case[1]](c)
        p0, p1 = pair(corpora, hindex, case, codec, V.OPTIONS[name])
        before, after, seams = V.seams_reached(c, p1, queries, wants(case[0], case[1]))
        moved = any(V.seam_documents(c, p0, int(p0.slot_of_query[q])) != V.seam_documents(c, p1, int(p1.slot_of_query[q])) for q in range(len(queries)))
        print(f"[seams] {name} codec {codec} {case[1]} {case[3]}: {seams} seams, queries matching before one {before}, after one {after}, cut changed {moved}")
        assert before > 0 and after > 0, (name, case, seams, before, after)
        changed = changed or moved
    assert changed, name  # (phrase_task_div = 8 cuts bitmap windows as the default 4 does — one window a task —: its cut differs on the mixed plan)


@pytest.mark.parametrize("codec", [1, 2])
def test_unions_on_both_sides_of_the_scatter_rule(corpora, hindex, codec):
    """min(N, head documents) x slack >= windows x SPAN_WORDS, both sides restated from the postings: at slack 1, 4 and 64 the variant's unions sit on either side,
    and the plan runs exactly those on the left as scatter units with a bitmap result, the others in k_and_dense with ascending docIDs."""
    c = corpora("main")
    queries = V.scatter_unions(c)
    for slack in (1, 4, 64):
        p = V.host_plan(hindex("main", codec), queries, "docs", {"plane_div": V.SCATTER_PLANE_DIV, "scatter_bitmap_slack": slack})
        scat = V.scatter_slots(p)
        sides = V.scatter_sides(c, V.SCATTER_UNIONS, slack, V.SCATTER_PLANE_DIV)
        assert all(mixed for *_, mixed in sides), sides
        seen = set()
        for qi, (text, left, right, _) in enumerate(sides):
            slot = int(p.slot_of_query[qi])
            msg = f"slack {slack}: {text}: min(N, head documents) x slack = {left}, windows x SPAN_WORDS = {right}"
            assert (slot in scat) == (left >= right), msg
            assert (int(p.plan["form"][slot]) == V.RESULT_BITMAP) == (left >= right) and V.kind_of_slot(p, slot) == (HP.TASK_PSET if left >= right else HP.TASK_DENSE), msg
            seen.add(left >= right)
        assert seen == {True, False}, (slack, sides)
    # and the full catalogue under the default plane_div, where the GPU file checks every variant: unions on both sides at 1 and 4 (at 64 every head term passes)
    for slack in (1, 4):
        assert {left >= right for _, left, right, _ in V.scatter_sides(c, V.SCATTER_UNIONS[:6], slack)} == {True, False}, slack


@pytest.mark.parametrize("codec", [1, 2])
def test_auto_choices_equal_the_forced_values(corpora, hindex, codec):
    """What plan_batch chooses by itself (settle_batch_knobs) is, byte for byte, the plan of the forced value the GPU file runs: phrase_task_div 4 / 2 / 1 as the
    batch's phrase queries cross 8 and 16 per compute unit, planes_split 3 / 2 as its one-pass queries cross 2 n >= 4 cus plk_wgs_per_cu — at cus = 4."""
    cus = 4
    blocks = lambda hi, q, mode, o: V.host_plan(hi, q, mode, o, cus=cus, threads=1).block.tobytes()  # noqa: E731
    for name, key, base, reps in (("phrase", "phrase", {}, (1, 3, 5)), ("stream", "stream", V.PHRASE_MIX, (1, 3, 5))):
        c, hi = corpora(name), hindex(name, codec)
        one = V.QUERY_LISTS[key](c)
        phrases = sum('"' in t for t, _ in one)
        got = []
        for rep, div in zip(reps, (4, 2, 1)):
            queries = one * rep
            # (each text with a phrase counts once — a tree query's hidden phrase queries are planned after the choice)
            assert (phrases * rep <= 8 * cus) == (div == 4) and (phrases * rep <= 16 * cus) == (div != 1), (name, rep, phrases)
            auto = blocks(hi, queries, "docs", base)
            forced = {d: blocks(hi, queries, "docs", dict(base, phrase_task_div=d)) for d in (1, 2, 4)}
            assert auto == forced[div], (name, rep, div)
            got.append([d for d in (1, 2, 4) if forced[d] == auto])
        if name == "stream":  # (the phrase corpus is one window and one tile: every cut is the same cut there)
            assert got == [[4], [2], [1]], got
    c, hi = corpora("freq"), hindex("freq", codec)
    plk = PLK_WGS_PER_CU
    base = {"dense_min_postings": 0}
    for n, split in ((24, 3), (32, 2)):
        queries = S.freq_queries(c)[:n]
        p = V.host_plan(hi, queries, "scored", base, cus=cus, threads=1)
        assert (2 * p.s["planes_queries"] >= 4 * cus * plk) == (split == 2) and p.s["planes_queries"] > 0, (n, p.s["planes_queries"])
        forced = {d: blocks(hi, queries, "scored", dict(base, planes_split=d)) for d in (2, 3)}
        assert p.block.tobytes() == forced[split] != forced[5 - split], (n, split)


@pytest.mark.parametrize("codec", [1, 2])
def test_tree_max_bytes_at_the_need_and_one_below(corpora, hindex, codec):
    """The documented need — (distinct term leaves x PL_PLANES + phrase leaves + tree queries) x plane words x 4 — from the default plan's own counters: a budget of
    exactly that plans, one byte less is refused by name, and the refusal reports the same number."""
    c = corpora("stream")
    queries = CT.stream_list(c)
    hi = hindex("stream", codec)
    p = V.host_plan(hi, queries, "docs", {})
    assert p.s["tree_queries"] >= 5 and p.s["n_tree_hidden"] > 0 and p.s["plw"] == V.plane_words(S.D_STREAM)
    need = (p.s["n_tree_terms"] * V.PL_PLANES + p.s["n_tree_hidden"] + p.s["tree_queries"]) * p.s["plw"] * 4
    at = V.host_plan(hi, queries, "docs", {"tree_max_bytes": need})
    assert at.block.tobytes() == p.block.tobytes()
    with pytest.raises(T.engine.TrinityError, match="tree_max_bytes") as e:
        V.host_plan(hi, queries, "docs", {"tree_max_bytes": need - 1})
    said = re.search(r"need (\d+) bytes .* tree_max_bytes = (\d+)", str(e.value))
    assert said and (int(said.group(1)), int(said.group(2))) == (need, need - 1), str(e.value)


@pytest.mark.parametrize("codec", [1, 2])
def test_consumer_batches_meet_the_fork_conditions(corpora, hindex, codec):
    """run_matching forks k_and onto the second stream when a batch holds window (or plane-set) tasks AND candidate tiles, and k_psets_prep when it holds scatter
    unions AND bitmap-window tasks: the GPU file's three batches hold what their tests say."""
    c = corpora("main")
    for key, mode in (("consumers", "docs"), ("consumers+scatter", "docs"), ("rich", "rich")):
        p = V.host_plan(hindex("main", codec), V.QUERY_LISTS[key](c), mode, {})
        assert p.s["n_dense"] > 0 and p.s["n_cand"] > 0 and p.s["dense_queries"] + p.s["pset_queries"] > 0 and p.s["cand_queries"] > 0, (key, p.s)
        assert (len(V.scatter_slots(p)) >= 3) == (key == "consumers+scatter") and (p.s["n_pset"] > 0 or mode == "rich"), key
        if mode == "docs":
            assert int(p.sched[0]) != int(V.sched_section(p, HP.TASK_CAND)[0])  # (tasks scheduled before k_and's: option overlap's own condition)
    sets = [c.evaluate(pp) for pp in S.programs(V.rich_queries(c))]
    assert all(0 < len(s) <= 8200 for s in sets), [len(s) for s in sets]
