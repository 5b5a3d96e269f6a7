"""CPU checks of the high-docID segments (tests/high_docid_cases.py) the GPU file tests/test_gpu_high_docid.py reads: through HostPlan, in both codecs and at
every top, each case reaches the planner outcome it is there for; the numpy reference equals the oracle over the encoded bytes; and each of five wrong readers —
the 32-bit slips a kernel can make in this range — changes the expected result of a named query at a named top, so the GPU file's comparisons would see it.

The score-gap condition, measured on the oracle (test_score_gap_condition prints it): 0 of 40 scored (top, query, K) cases fall under structured.check_topk's
set-wise rule (bound: 10 %)."""
import numpy as np
import pytest

import high_docid_cases as H
import oracle_lib as O
import structured as S
import trinity_amd as T
from trinity_amd import hostplan as HP

SPAN = S.SPAN_BITS
PSET_UNIT_SCATTER = H.PSET_UNIT_SCATTER


@pytest.fixture(scope="module")
def base():
    T.build.build_host()
    return H.base_corpus()


@pytest.fixture(scope="module")
def corpora(base):
    made = {}

    def get(top, span=False):
        if (top, span) not in made:
            made[top, span] = H.shifted(base, H.TOPS[top], span)
        return made[top, span]

    return get


def plan_of(hi, c, flags=T.FLAG_DOCUMENTS_ONLY, topk=0, names=None, queries=None, **opts):
    opts.setdefault("plane_max_bytes", 2 * H.row_bytes(c.D))
    return HP.HostPlan(hi, S.programs(queries or H.docs_queries(c, names)), flags, topk, threads=2, options=opts)


def kind_of(p, qi):
    return int(p.tasks["kind"][int(p.plan["first_task"][int(p.slot_of_query[qi])])])


def tasks_of(p, qi):
    q = p.plan[int(p.slot_of_query[qi])]
    return p.tasks[int(q["first_task"]) : int(q["first_task"]) + int(q["ntasks"])]


def test_the_base_and_the_shift(base, corpora):
    df = dict(zip(base.names, base.df().tolist()))
    assert base.D == H.D_BASE and 3000 < base.postings < 10000
    assert df["h0"] > 32 * S.WIN_MIN_BLOCKS > df["h1"] > H.D_BASE // 1024 > max(df[n] for n in H.RARE)  # a cell index for h0 alone; planes for the heads alone
    assert H.TOPS == {"PK_LAST": 0x7FFEFFFF, "PK_FIRST": 0x7FFF0000, "SIGN": 1 << 31, "EXTENT_EQ": (1 << 32) - (1 << 18), "TOP": (1 << 32) - 2}
    assert (H.plw_of(H.EXTENT_EQ) * 32) == 1 << 32 and H.plw_of(H.EXTENT_EQ - 1) * 32 < 1 << 32 and H.nwin_of(H.SIGN) > H.PSCAT_MAX_TASKS * H.PSET_TASK_WINDOWS >= H.nwin_of(H.SIGN - 1)
    for top in H.TOPS:
        for span in (False, True):
            c = corpora(top, span)
            sh = H.shift_of(H.TOPS[top])
            assert c.D == H.TOPS[top] and c.docs_cnt == base.docs_cnt and sh % SPAN == 0 and 0 <= H.TOPS[top] - sh - H.D_BASE < SPAN
            for n in base.names:
                d, bd = c.lists[n][0].astype(np.int64), base.lists[n][0].astype(np.int64)
                body = d[2:] if span and n in H.HEADS else d
                assert np.array_equal(body[:-1], bd[:-1] + sh) and int(body[-1]) == H.TOPS[top], (top, n)  # every edge document stays on its edge; the last one sits on `top`
                assert (d[:2].tolist() == [1, 2]) == (span and n in H.HEADS)
            for case in ("pair_and", "phrase", "scatter", "tree", "rare_pair"):  # `top` is a match of what the GPU file reads at it
                got = c.evaluate(S.programs(H.docs_queries(c, [case]))[0])
                assert int(got[-1]) == H.TOPS[top] and (int(got[0]) == 1) == (span and case != "rare_pair"), (top, span, case)


@pytest.mark.parametrize("top", list(H.TOPS))
def test_evaluate_equals_the_oracle(corpora, top):
    """evaluate() == the oracle over the GOOGLE bytes on every DocumentsOnly query of the catalogue and every scored list; the oracle decodes the bytes back to the postings."""
    for span in (False, True):
        c = corpora(top, span)
        ora = c.oracle()
        for t, n in enumerate(c.names):
            d, f = ora.decode_term(t)
            assert np.array_equal(d, c.lists[n][0]) and np.array_equal(f, c.lists[n][1]), n
        queries = H.docs_queries(c) + H.scored_queries(c)
        for (text, mn), p in zip(queries, S.programs(queries)):
            want, _ = ora.exec(p, O.FLAG_DOCUMENTS_ONLY)
            assert len(want) and np.array_equal(c.evaluate(p), want), (top, span, text)


@pytest.mark.parametrize("name", list(H.WRONG_READERS))
def test_a_wrong_reader_changes_a_named_result(corpora, name):
    """Each slip changes the expected result of WRONG_AT's query at its top — and leaves it alone below 2^31 - 2^16, where the suite's other corpora live."""
    top, span, case = H.WRONG_AT[name]
    c = corpora(top, span)
    prog = S.programs(H.docs_queries(c, [case]))[0]
    right, wrong = c.evaluate(prog), H.misread(c, H.WRONG_READERS[name], prog)
    assert not np.array_equal(right, wrong), (name, top, span, case)
    assert np.array_equal(H.misread(c, lambda d, _c: d, prog), right)  # (the misreading harness itself reads right)
    low = corpora("PK_LAST", span)
    if name not in ("drops_top", "aliases_bottom"):  # (those two are wrong at every top)
        lp = S.programs(H.docs_queries(low, [case]))[0]
        assert np.array_equal(H.misread(low, H.WRONG_READERS[name], lp), low.evaluate(lp)), name


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("top", list(H.TOPS))
def test_each_case_reaches_what_it_is_for(corpora, codec, top):
    names = list(H.CASES)
    at = {n: i for i, n in enumerate(names)}
    for span in (False, True):
        c = corpora(top, span)
        nwin = H.nwin_of(c.D)
        hi = c.host_index(codec)
        heads = sorted(c.tid[n] for n in H.HEADS)
        # ---- plane-set windows, the scatter union (or what replaces it), the tree
        p = plan_of(hi, c, dense_min_postings=0, scatter_bitmap_slack=H.SCATTER_SLACK)
        assert p.s["unsupported_queries"] == 0 and p.s["plw"] == H.plw_of(c.D) and sorted(p.plane_terms.tolist()) == heads, (top, span)
        assert kind_of(p, at["pair_and"]) == HP.TASK_PSET and kind_of(p, at["tree"]) == HP.TASK_TREE and p.s["tree_queries"] == 1 and p.s["n_tree_terms"] == 1 and p.s["n_tree_hidden"] == 1
        tk = tasks_of(p, at["pair_and"])
        assert int(tk["begin"][0]) == 0 and int(tk["end"][-1]) == nwin and len(tk) == -(-nwin // H.PSET_TASK_WINDOWS)  # the top window holds a plane-set task
        assert (len(tk) > H.PSCAT_MAX_TASKS) == (c.D >= H.SIGN)
        scat = [u for u in p.units if int(u["first"]) & PSET_UNIT_SCATTER]
        for case in ("scatter", "scatter4"):
            q = p.plan[int(p.slot_of_query[at[case]])]
            if c.D < H.SIGN:  # a PSET_UNIT_SCATTER union, result a bitmap from document 0 to the top window's end
                assert kind_of(p, at[case]) == HP.TASK_PSET and int(q["form"]) == 1 and int(q["out_cap"]) == nwin * (SPAN // 32) and int(q["ntasks"]) <= H.PSCAT_MAX_TASKS, (top, case)
            else:  # route_cnf makes no scatter unit for a query of more than PSCAT_MAX_TASKS tasks: bitmap windows of k_and_dense, ascending docIDs
                assert kind_of(p, at[case]) == HP.TASK_DENSE and int(q["form"]) == 0 and int(tasks_of(p, at[case])["end"][-1]) == nwin, (top, case)
        assert (len(scat) > 0) == (c.D < H.SIGN) and all(int(u["end"]) * SPAN <= 1 << 31 for u in scat)
        p.close()
        # ---- bitmap windows with the rows decoded (no planes): a TASK_DENSE task holds the top window
        p = plan_of(hi, c, dense_min_postings=0, planes=0)
        assert p.s["n_plane_terms"] == 0 and p.s["n_pset"] == 0 and kind_of(p, at["pair_or"]) == HP.TASK_DENSE and int(tasks_of(p, at["pair_or"])["end"][-1]) == nwin
        p.close()
        # ---- candidate tiles: the lead list's last tile ends on `top`
        p = plan_of(hi, c)
        assert kind_of(p, at["rare_pair"]) == HP.TASK_CAND and kind_of(p, at["rare_lead"]) in (HP.TASK_CAND, HP.TASK_PROBE) and p.s["unsupported_queries"] == 0
        lead = int(p.qterms[int(p.plan["term_base"][int(p.slot_of_query[at["rare_pair"]])])]) & 0x3FFFFFFF
        assert int(c.lists[c.names[lead]][0][-1]) == c.D and int(tasks_of(p, at["rare_pair"])["end"][-1]) == 1
        p.close()
        # ---- k_probe, when told to take every single-lead conjunction
        p = plan_of(hi, c, names=["rare_lead", "pair_and"], plane_div=S.ALL_PLANES, probe_max_blocks=1 << 20)
        assert p.s["n_probe"] > 0 and kind_of(p, 0) == HP.TASK_PROBE
        p.close()
        hi.close()


@pytest.mark.parametrize("codec", [1, 2])
def test_k_planes_gate(corpora, codec):
    """planes_queries > 0 at PK_LAST and == 0 at PK_FIRST, the plans otherwise equal: what k_planes ran, k_fused runs."""
    s = {}
    for top in ("PK_LAST", "PK_FIRST"):
        c = corpora(top)
        hi = c.host_index(codec)
        p = plan_of(hi, c, T.FLAG_ACCUMULATED_SCORE, 10, queries=H.scored_queries(c), dense_min_postings=0)
        s[top] = dict(p.s)
        p.close()
        hi.close()
    a, b = s["PK_LAST"], s["PK_FIRST"]
    assert a["planes_queries"] > 0 and b["planes_queries"] == 0 and b["fused_queries"] == a["fused_queries"] + a["planes_queries"]
    assert a["n_planes"] + a["n_planes8"] > 0 and b["n_planes"] + b["n_planes8"] == 0
    for k in ("n_plan", "dense_queries", "cand_queries", "pset_queries", "probe_queries", "tree_queries", "unsupported_queries", "n_dense", "n_cand", "n_pset", "n_tree"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("codec", [1, 2])
def test_k_fused_gate(corpora, codec):
    """Below FUSED_MAX_DOC scored CNF queries run in one pass and a matchsome off its truth table; from it on (TOP) the scored queries run match-then-score with
    nothing left out, and the matchsome is left out by name."""
    assert H.EXTENT_EQ < H.FUSED_MAX_DOC == 0xFFFFC000 <= H.TOP and f"{H.FUSED_MAX_DOC:#x}" == "0xffffc000"
    for top in ("SIGN", "EXTENT_EQ", "TOP"):
        c = corpora(top, True)
        hi = c.host_index(codec)
        for opts in H.SCORED_SETS:
            p = plan_of(hi, c, T.FLAG_ACCUMULATED_SCORE, 10, queries=H.scored_queries(c), **opts)
            onepass = p.s["n_fused"] + p.s["n_fused16"] + p.s["n_fusedgen"]
            assert p.s["unsupported_queries"] == 0 and p.s["planes_queries"] == 0 and (onepass == 0 or c.D < H.FUSED_MAX_DOC), (top, opts)
            if opts.get("dense_min_postings") == 0 and opts.get("fused", 1):
                assert (p.s["fused_queries"] > 0) == (c.D < H.FUSED_MAX_DOC), (top, opts)
            p.close()
        for flags in (T.FLAG_DOCUMENTS_ONLY, T.FLAG_ACCUMULATED_SCORE):
            p = plan_of(hi, c, flags, 10 if flags == T.FLAG_ACCUMULATED_SCORE else 0, queries=[(c.q(H.TRUTH[0]), H.TRUTH[1])])
            if c.D < H.FUSED_MAX_DOC:
                assert p.s["unsupported_queries"] == 0 and kind_of(p, 0) == HP.TASK_FUSED_GEN
            else:
                assert p.s["unsupported_queries"] == 1 and int(p.qstatus[0]) == -3 and "0xffffc000" in p.last_unsupported and "2^32" in p.last_unsupported, p.last_unsupported
            p.close()
        hi.close()


def test_score_gap_condition(corpora):
    """The share of scored (top, query, K) cases the oracle's own scores put under structured.check_topk's set-wise rule: at most 10 %."""
    cases = setwise = 0
    for top in ("PK_LAST", "SIGN", "EXTENT_EQ", "TOP"):
        c = corpora(top)
        ora = c.oracle()
        queries = H.scored_queries(c)
        for (text, mn), p in zip(queries, S.programs(queries)):
            docs, scores = ora.exec(p, O.FLAG_ACCUM_SCORE)
            for k in (10, 256) if text == c.q(H.SCORED_K256) else (10,):
                cases += 1
                setwise += not S.score_gaps(scores, k)[0]
    print(f"high-docID score-gap condition: {setwise} of {cases} scored cases under the set-wise rule")
    assert cases == 40 and setwise <= 0.10 * cases, (setwise, cases)


def test_the_sparse_isect_restatement_equals_isect_cases():
    """high_docid_cases.isect_restate == isect_cases.restate where the latter's array over the docID space is affordable; the gadget's run is credited."""
    import isect_cases as IC

    c, groups = H.isect_gadget(3 * S.PL_W + 1234)
    pg = [[c.lists[c.names[t]][0].astype(np.int64) for t in g] for g in groups]
    lst, hist, _ = IC.restate(pg, 0, (), top=c.D)
    assert H.isect_restate(c, groups) == (lst, hist) and len(lst) >= 2 and any(f == c.D - 10 for _, f in hist.values())
