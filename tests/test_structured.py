"""CPU checks of the structured segments (tests/structured.py) the GPU file tests/test_gpu_structured.py reads: the numpy reference used there is right (it
equals the oracle over the encoded bytes, and the oracle decodes the bytes back to the postings), the catalogue reaches the task kinds and the two dense_pass
branches it claims to, the mirrored geometry constants have not drifted, and the top-K comparison rarely needs its tie-group form.

The score-gap condition, measured on the oracle (test_score_gap_condition prints both): 46 of 912 scored (query, K, similarity) cases, 5.0 %, fall under the
set-wise rule (bound: 10 %); the smallest relative gap between distinct oracle scores within ranks 1 .. K + 1 is 3.1e-11 (tolerance: 1e-5) — the same addends
summed in another order."""
import numpy as np
import pytest

import oracle_lib as O
import structured as S
import trinity_amd as T
from trinity_amd import hostplan as HP

KINDS = ["n_dense", "n_cand", "n_pset", "n_planes", "n_planes8", "n_fused", "n_fused16", "n_fusedgen", "n_tree"]
KIND_ID = {"n_dense": HP.TASK_DENSE, "n_cand": HP.TASK_CAND, "n_pset": HP.TASK_PSET, "n_planes": HP.TASK_PLANES, "n_planes8": HP.TASK_PLANES8, "n_fused": HP.TASK_FUSED,
           "n_fused16": HP.TASK_FUSED16, "n_fusedgen": HP.TASK_FUSED_GEN, "n_tree": HP.TASK_TREE}  # fmt: skip


@pytest.fixture(scope="module")
def corpora():
    T.build.build_host()
    return {k: f() for k, f in S.CORPORA.items()}


def test_geometry_mirrors():
    k = S.header_constants("dev_structs.hpp", "k_match.hpp", "k_planes.hpp", "k_fused.hpp", "k_phrase.hpp")
    for f, names in S.MIRRORS.items():
        for n in names:
            assert k[n] == getattr(S, n), (f, n, k[n], getattr(S, n))
    assert S.FUS_W % S.PL_RANK_DOCS == 0 and S.D_MAIN == 4 * S.SPAN_BITS + 37


def test_catalogue_has_the_shapes_it_names(corpora):
    m = corpora["main"]
    d = {n: m.lists[n][0].astype(np.int64) for n in m.names}
    assert m.D == S.D_MAIN and d["all"].size == m.D
    for w in S.WINDOWS:  # a document on every boundary of every window, and on both sides of it
        b = np.arange(w, m.D, w)
        assert np.isin(np.concatenate([b - 1, b, b + 1]), d["edges"]).all(), w
    win = lambda x: np.unique(x // S.SPAN_BITS).tolist()  # noqa: E731
    assert win(d["lastwin"]) == [3, 4] and win(d["stub"]) == [4] and win(d["firstwin"]) == [0] and win(d["midwin"]) == [2] and win(d["holes"]) == [0, 4]
    assert [d[f"df{n}"].size for n in S.DF_EDGES] == S.DF_EDGES and d["first1"].tolist() == [1] and d["last1"].tolist() == [m.D]
    nblocks = lambda n: -(-d[n].size // 32)  # noqa: E731
    assert nblocks("df4064") == S.WIN_MIN_BLOCKS - 1 and nblocks("df4065") == S.WIN_MIN_BLOCKS and nblocks("df8192") == S.TILE_BLOCKS and nblocks("df8193") == S.TILE_BLOCKS + 1
    sparse = lambda x: x.size * 28 < int(x[-1])  # noqa: E731  (index_host.hpp: TERM_SPARSE)
    assert sparse(d["sp_lo"]) and not sparse(d["sp_hi"]) and d["sp_hi"].size == d["sp_lo"].size + 1 and sparse(d["sparse_runs"]) and (np.diff(d["sparse_runs"]) == 1).sum() > 5000
    f = corpora["freq"]
    cyc = f.lists["all_cyc"][1]
    assert set(cyc.tolist()) == set(S.FREQ_CYCLE) and {0, S.PL_STORED, S.PL_NESTED, 6, 7, 14, 15, 30, 31, 254, 255, 300} <= set(S.FREQ_CYCLE)
    assert np.all(np.diff(f.lists["odd_rise"][1].astype(np.int64)) >= 0) and np.all(np.diff(f.lists["odd_fall"][1].astype(np.int64)) <= 0) and int(f.lists["all_rise"][1].max()) > 2 * S.PL_W // S.CELL_DOCS
    assert f.lists["third_last3"][1][-4:].tolist() == [1, 7, 30, 300] and set(f.lists["all_one"][1].tolist()) == {1}
    t = corpora["tall"]
    assert t.D == S.D_TALL and int(t.lists["beyond"][0].min()) > 1 << 21
    for n in ("gap4_a", "gap4_b", "gap4_c"):
        assert int(np.diff(t.lists[n][0].astype(np.int64)).max()) >= 1 << 21, n  # a four-byte delta (prefix varint)


@pytest.mark.parametrize("name", list(S.CORPORA))
def test_the_checker_checks_itself(corpora, name):
    """evaluate() (numpy over the postings arrays) == the oracle over the GOOGLE bytes, for every query the GPU file runs; the oracle decodes the bytes back to the postings."""
    c = corpora[name]
    ora = c.oracle()
    for t, n in enumerate(c.names):
        d, f = ora.decode_term(t)
        assert np.array_equal(d, c.lists[n][0]) and np.array_equal(f, c.lists[n][1]), n
    queries = S.QUERIES[name](c) + (S.SCORED_CASES[name][0](c) if name in ("main", "tall") else []) + (S.tie_queries(c) if name == "freq" else [])
    assert len(queries) >= 17
    nonempty = 0
    for (text, mn), p in zip(queries, S.programs(queries)):
        want, _ = ora.exec(p, O.FLAG_DOCUMENTS_ONLY)
        got = c.evaluate(p)
        assert np.array_equal(got, want), (text, mn, len(got), len(want))
        nonempty += len(want) > 0
    assert nonempty >= len(queries) // 2
    if name == "main":  # masked documents: the final result minus the masked set (masked_documents_registry::test right before consider())
        mk = c.lists["edges"][0]
        ora.set_masked(mk)
        for (text, mn), p in list(zip(queries, S.programs(queries)))[::7]:
            assert np.array_equal(c.evaluate(p, masked=mk), ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0]), text


def kinds_of_queries(p, nq):
    """Task kind of every query of a HostPlan (-1: not lowered)."""
    out = np.full(nq, -1, dtype=np.int64)
    plan, tasks = p.plan, p.tasks
    for qi in range(nq):
        sl = int(p.slot_of_query[qi])
        if sl != 0xFFFFFFFF:
            out[qi] = int(tasks["kind"][int(plan["first_task"][sl])])
    return out


@pytest.mark.parametrize("codec", [1, 2])
def test_routing(corpora, codec):
    """Every option set of the GPU file puts queries of the intended lists on the intended task kinds; between them all nine kinds are reached; nothing is refused."""
    reached = {k: 0 for k in KINDS}

    def plan(c, hi, queries, flags, topk, opts):
        progs = S.programs(queries)
        p = HP.HostPlan(hi, progs, flags, topk, threads=4, options=opts)
        assert p.s["unsupported_queries"] == 0, opts
        for k in KINDS:
            reached[k] += p.s[k]
        kinds = kinds_of_queries(p, len(progs))
        p.close()
        return kinds

    def on_kind(c, queries, kinds, kind, *lists):
        """queries that name every one of `lists` and run as `kind`"""
        words = [f"t{c.tid[n]}" for n in lists]
        return [t for (t, _), k in zip(queries, kinds) if k == KIND_ID[kind] and all(w in t.replace("(", " ").replace(")", " ").split() for w in words)]

    m, f, tall, ph = corpora["main"], corpora["freq"], corpora["tall"], corpora["phrase"]
    hi = m.host_index(codec)
    mq = S.main_queries(m)
    for opts, want in S.DOCS_OPTION_SETS:
        kinds = plan(m, hi, mq, T.FLAG_DOCUMENTS_ONLY, 0, opts)
        for k in want:
            assert (kinds == KIND_ID[k]).sum() > 0, (opts, k)
        assert on_kind(m, mq, kinds, "n_cand", "edges"), opts  # the boundary list as a candidate-tile lead or probe in every set ...
        if opts == {"dense_min_postings": 0, "planes": 0}:  # ... and what dense_pass decodes itself: the boundary list, the list whose deferred blocks overflow, the sparse-flag pair
            for n in ("edges", "dense_many_slow", "sp_lo", "sp_hi", "holes", "lastwin"):
                assert on_kind(m, mq, kinds, "n_dense", n), n
        if "planes" not in opts and "n_pset" in want:
            assert on_kind(m, mq, kinds, "n_pset", "all", "odd") and on_kind(m, mq, kinds, "n_pset", "holes")
    # the mixed-delivery batch: docID-form results of 1, 2, 3 (mod 4) documents, each directly before a bitmap-form one
    xq = S.mixed_queries(m)
    p = HP.HostPlan(hi, S.programs(xq), T.FLAG_DOCUMENTS_ONLY, 0, threads=2)
    forms = [int(p.plan["form"][int(p.slot_of_query[i])]) for i in range(len(xq))]
    p.close()
    assert forms == [0, 1] * (len(xq) // 2) and {len(m.evaluate(pp)) % 4 for pp in S.programs(xq)[0::2]} == {1, 2, 3}
    sq = S.main_scored_queries(m)
    for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}):
        plan(m, hi, sq, T.FLAG_ACCUMULATED_SCORE, 10, opts)
    hi.close()
    hi = f.host_index(codec)
    fq = S.freq_queries(f)
    for opts, want in S.SCORED_OPTION_SETS:
        kinds = plan(f, hi, fq, T.FLAG_ACCUMULATED_SCORE, 10, opts)
        for k in want:
            assert (kinds == KIND_ID[k]).sum() > 0, (opts, k)
            if opts:
                assert on_kind(f, fq, kinds, k, "all_cyc" if k != "n_cand" else "n10"), (opts, k)  # the saturating frequencies through every one-pass variant
    hi.close()
    hi = tall.host_index(codec)
    tq = S.tall_queries(tall)
    kinds = plan(tall, hi, tq, T.FLAG_DOCUMENTS_ONLY, 0, {"dense_min_postings": 0, "planes": 0})
    assert on_kind(tall, tq, kinds, "n_dense", "dense_tail3") and on_kind(tall, tq, kinds, "n_dense", "beyond")
    hi.close()
    hi = ph.host_index(codec)
    for flags in (T.FLAG_DOCUMENTS_ONLY, T.FLAG_ACCUMULATED_SCORE, T.FLAG_MATCHED_TERMS):
        for opts in ({}, {"dense_min_postings": 0}):
            plan(ph, hi, S.phrase_queries(ph), flags, 10 if flags == T.FLAG_ACCUMULATED_SCORE else 0, opts)
    hi.close()
    hi = f.host_index(codec)
    plan(f, hi, S.rich_freq_queries(f), T.FLAG_MATCHED_TERMS, 0, {})
    hi.close()
    # the stream corpus (tests/test_gpu_stream.py): plane_max_bytes = N rows makes exactly the head terms of df rank < N eligible, and every batch of the docs-only and
    # scored tables CHOOSES every eligible head term it names — the GPU file's model of the plane cache relies on both; the rare terms never get a plane
    st = corpora["stream"]
    hi = st.host_index(codec)
    heads = S.STREAM_HEADS
    assert [st.names[t] for t in np.argsort(-st.df(), kind="stable")[: len(heads)]] == heads  # (a term's plane row is its df rank: h_i's is i)
    plw = ((S.D_STREAM >> 17) + 2) * (S.SPAN_BITS // 32)
    row_bytes = S.header_constants("dev_structs.hpp")["PL_PLANES"] * plw * 4

    def chosen(queries, flags, topk, opts):
        p = HP.HostPlan(hi, S.programs(queries), flags, topk, threads=2, options=opts)
        assert p.s["unsupported_queries"] == 0 and p.s["plw"] == plw, opts
        for k in KINDS:
            reached[k] += p.s[k]
        out = sorted(st.names[t] for t in p.plane_terms.tolist())
        nptasks = p.s["n_ptasks"]
        p.close()
        return out, nptasks

    for n, names in ((2, heads[:2]), (2, heads[:5]), (3, heads[:3]), (4, heads[:4]), (5, heads[:5]), (6, heads[4:6]), (len(heads), heads), (0, heads)):
        cap = {"plane_div": S.ALL_PLANES, "plane_max_bytes": n * row_bytes} if n else {}
        want = sorted(x for x in names if heads.index(x) < (n or len(heads)))
        assert chosen(S.stream_docs_queries(st, names), T.FLAG_DOCUMENTS_ONLY, 0, cap)[0] == want, (n, names)
        for opts in ({}, {"dense_min_postings": 0}, {"fused": 0, "planes": 3}):
            for k in (10, 256):
                assert chosen(S.stream_scored_queries(st, names), T.FLAG_ACCUMULATED_SCORE, k, dict(cap, **opts))[0] == want, (n, names, opts, k)
    for n, names in ((2, heads[:2]), (len(heads), heads[:6])):
        for flags in (T.FLAG_DOCUMENTS_ONLY, T.FLAG_ACCUMULATED_SCORE):
            got, nptasks = chosen(S.stream_phrase_queries(st, names), flags, 10 if flags == T.FLAG_ACCUMULATED_SCORE else 0, {"plane_div": S.ALL_PLANES, "plane_max_bytes": n * row_bytes})
            assert nptasks > 0 and got and set(got) <= set(names), (n, got)
    hi.close()
    assert all(reached[k] > 0 for k in KINDS), reached


def test_dense_pass_lists_have_the_properties_they_claim(corpora):
    """From the ENCODED bytes: neither list is TERM_SPARSE by index_host.hpp's rule (documents * 28 < last document), so k_and_dense takes the static path
    and defers their odd blocks; `dense_many_slow` has more than DENSE_SLOW_CAP full blocks with a multi-byte delta inside ONE SPAN_BITS window (the deferred
    list overflows); `dense_tail3` has a block with more than 64 bytes of deltas (the cooperative decoder hands it to one lane)."""
    m, t = corpora["main"], corpora["tall"]
    blocks = S.google_blocks(m.g_index, m.g_terms, m.tid["dense_many_slow"])
    assert sum(b[1] for b in blocks) == m.lists["dense_many_slow"][0].size and blocks[-1][0] == int(m.lists["dense_many_slow"][0][-1])
    assert not sum(b[1] for b in blocks) * 28 < blocks[-1][0]
    per_window = {}
    prev = 0
    for last, n, nbytes, longest in blocks:
        if longest > 1 and prev // S.SPAN_BITS == last // S.SPAN_BITS:  # a deferred block that lies inside one window
            per_window[last // S.SPAN_BITS] = per_window.get(last // S.SPAN_BITS, 0) + 1
        prev = last
    assert max(per_window.values()) > S.DENSE_SLOW_CAP, per_window
    blocks = S.google_blocks(t.g_index, t.g_terms, t.tid["dense_tail3"])
    assert sum(b[1] for b in blocks) == t.lists["dense_tail3"][0].size and not sum(b[1] for b in blocks) * 28 < blocks[-1][0]
    assert max(b[2] for b in blocks) > 64 and sum(b[3] == 1 and b[1] == 32 for b in blocks) >= 3000
    # and the sparse-flag pair, from the bytes as well
    for n, flag in (("sp_lo", True), ("sp_hi", False)):
        blocks = S.google_blocks(m.g_index, m.g_terms, m.tid[n])
        assert (sum(b[1] for b in blocks) * 28 < blocks[-1][0]) == flag, n


def test_score_gap_condition(corpora):
    """Top-K docID lists are compared exactly wherever all distinct oracle scores within ranks 1 .. K + 1 differ by more than rtol = 1e-5 (structured.check_topk);
    at most 10 % of the scored (query, K, similarity) cases may need the set-wise rule instead — or the frequency patterns have to change, not the rule."""
    cases = setwise = 0
    smallest = np.inf
    for name, (qf, ks) in S.SCORED_CASES.items():
        c = corpora[name]
        ora = c.oracle()
        runs = [(qf(c), 0)] + ([(S.tie_queries(c), sim) for sim in (0, 1, 2)] if name == "freq" else [])
        for queries, sim in runs:
            ora.set_similarity(sim)
            for (text, mn), p in zip(queries, S.programs(queries)):
                docs, scores = ora.exec(p, O.FLAG_ACCUM_SCORE)
                for k in ks:
                    exact, gap = S.score_gaps(scores, k)
                    cases += 1
                    setwise += not exact
                    smallest = min(smallest, gap)
    print(f"score-gap condition: {setwise} of {cases} scored cases ({100.0 * setwise / cases:.1f} %) under the set-wise rule; smallest relative gap between distinct scores {smallest:.3g}")
    assert cases >= 600 and setwise <= 0.10 * cases, (setwise, cases)
