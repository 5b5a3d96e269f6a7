"""GPU tests of the wide tree kernels (run with -m gpu on an MI355X): k_tree_eval_wide / k_tree_leaves_wide (csrc/k_tree_wide.hpp) through the C-ABI —
the trees the project has reference answers for forced through them (option tree_wide_min_nodes = 0), trees of more than 64 nodes (option
tree_max_nodes = 1024) against the CPU oracle's iterator trees, vocabularies the oracle does not take against numpy over the decoded lists, and the
default options, which still leave such a tree out."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import GOLDEN, World, options, rich_flat, run_docs_only, run_rich, run_scored
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)
from trinity_amd import hostplan as HP

pytestmark = pytest.mark.gpu
WIDE = {"tree_max_nodes": 1024}
FORCED = {"tree_wide_min_nodes": 0}
BIG = " OR ".join(f"(t{2 * i} t{2 * i + 1})" for i in range(40))  # 40 conjunctions under an OR: 121 nodes


def deep_text():
    deep = "t0"
    for i in range(1, 34):
        deep = f"(({deep}) OR t{i % 12})" if i % 2 else f"(({deep}) (t{i % 12} OR t{(i + 1) % 12}))"
    return deep


# name, expression, some_min, also run in the default mode (at most 16 reportable terms), matches at D = 2000 / 66000 (the oracle's, worked out on the CPU)
SHAPES = [
    ("or-of-and", " OR ".join(f"(t{i} t{i + 1})" for i in range(40)), 1, False, (1573, 45322)),
    ("cnf", " ".join(f"(t{(3 * i) % 12} OR t{(3 * i + 1) % 12} OR t{(3 * i + 2) % 12})" for i in range(22)), 1, False, (211, 4500)),
    ("some130", "[" + ", ".join(f"t{i % 60}" for i in range(130)) + "]", 20, False, (379, 5033)),  # 8 counter planes: one more than the narrow kernel has
    ("not-wide", "t0 NOT (" + " OR ".join(f"(t{i} t{i + 1})" for i in range(1, 35)) + ")", 1, False, (694, 28164)),
    ("deep", deep_text(), 1, True, (386, 10756)),
    ("or-of-and12", " OR ".join(f"(t{i % 12} t{(i * 5 + 1) % 12})" for i in range(30)), 1, True, (1500, 43665)),
    ("opt-wide", "t1 <" + " OR ".join(f"(t{i % 12} t{(i + 3) % 12})" for i in range(25)) + ">", 1, True, (1186, 35244)),
    ("phrases", " OR ".join(f'"t{i % 10} t{(i + 1) % 10}"' for i in range(20)) + " OR " + " OR ".join(f"(t{i} t{i + 1})" for i in range(12, 30)), 1, False, (581, 16017)),
]  # fmt: skip
WORLDS = [(2000, 200, 10, 42), (66000, 500, 10, 42)]  # (the second: just past one 65 536-document chunk of the tree kernels — the last chunk is short)


def shape_programs():
    return [O.parse_query(text, some_min=mn) for _, text, mn, _, _ in SHAPES]


def masked_set(D):
    return np.array(sorted(set(np.random.default_rng(3).integers(1, D, D // 7).tolist())), dtype=np.uint32)  # (as the narrow kernels' tree test builds it)


class Memo:
    """The oracle's answers under a dropped set (the index's masked documents, a query's filter, both), computed once each."""

    def __init__(self, ora):
        self.ora, self.memo = ora, {}

    def get(self, key, drop, prog, rich=False):
        k = (key, prog.tobytes(), rich)
        if k not in self.memo:
            self.ora.set_masked(drop)
            try:
                self.memo[k] = self.ora.exec_rich(prog) if rich else self.ora.exec(prog, O.FLAG_ACCUM_SCORE)
            finally:
                self.ora.set_masked(np.zeros(0, np.uint32))
        return self.memo[k]


# ------------------------------------------------------------------------------------------ 1: the wide kernels on the trees the reference answered
@pytest.mark.parametrize("corpus", sorted(json.load(open(os.path.join(GOLDEN, "ref_phrase_trees.json")))["corpora"]))
def test_forced_wide_gives_the_reference_answers_and_the_narrow_kernels_streams(T, dev, corpus):
    """tests/golden/ref_phrase_trees.json with tree_wide_min_nodes = 0 — every tree query runs k_tree_eval_wide / k_tree_leaves_wide: the reference's answers hold
    exactly as they do for the narrow kernels (test_gpu_parity.py: docsets and their hashes against the oracle, the reference's counts, top-10, score sums and
    default-mode stream hashes).  Then the same batches at default options: docsets, counts and matched terms equal; scores within 1e-5 — and bit for bit, which
    is printed (both kernels add the reached leaves' scores in node order, in double)."""
    g = json.load(open(os.path.join(GOLDEN, "ref_phrase_trees.json")))
    c = g["corpora"][corpus]
    w = World(T, dev, c["D"], c["V"], c["slots"], c["seed"])
    recs = [r for r in g["results"] if r["corpus"] == corpus]
    progs = [np.array(O.program_from_exec_tree(r["tree"]), dtype=np.uint32) for r in recs]

    def everything():
        sets, hashes, info = run_docs_only(w, progs)
        d, s, cnt, counts = run_scored(w, progs, 10)
        full = T.Batch(w.ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=0)
        full.run()
        full.sync()
        fc = full.counts()
        streams = [(full.docset(i, int(fc[i])), full.scores(i, int(fc[i]))) for i in range(len(progs))]
        full.close()
        return sets, hashes, info, d, s, cnt, counts, streams, run_rich(w, progs)

    with options(dev, **FORCED):
        hp = HP.HostPlan(HP.HostIndex.from_segment(w.seg), progs, T.FLAG_DOCUMENTS_ONLY, options=FORCED)
        tree_slots = np.nonzero(hp.tasks["kind"][hp.plan["first_task"]] == HP.TASK_TREE)[0]
        assert len(tree_slots) and all(hp.tree_kind(int(sl))[0] == HP.TREE_KIND_WIDE for sl in tree_slots)  # (what the device plans: the same planner, the same options)
        hp.close()
        sets, hashes, info, d, s, cnt, counts, streams, rich = everything()
    assert info["unsupported_queries"] == 0 and info["tree_queries"] == len(tree_slots) > len(recs) // 2
    hashed = 0
    for i, r in enumerate(recs):
        want, _ = w.ora.exec(progs[i], O.FLAG_DOCUMENTS_ONLY)
        assert np.array_equal(sets[i], want) and int(hashes[i]) == O.fnv1a_docs(want), r["q"]
        assert int(counts[i]) == r["n"], r["q"]
        top = r["top"]
        assert d[i, : len(top)].tolist() == [x[0] for x in top], r["q"]
        np.testing.assert_allclose(s[i, : len(top)], [x[1] for x in top], rtol=1e-5, err_msg=r["q"])
        assert np.array_equal(streams[i][0], sets[i]) or r["n"] != len(sets[i]), r["q"]
        assert abs(float(np.sum(streams[i][1][: r["n"]])) - r["score_sum"]) <= 1e-5 * max(1.0, r["score_sum"]), r["q"]
        docs, terms, present, freq, pos = rich[i]
        assert len(docs) == r["rich_n"] and int(freq.sum()) == r["hits_total"], r["q"]
        assert int(sum(bin(int(x)).count("1") for x in present)) == r["terms_total"], r["q"]
        if r["rich_fnv"] is not None:
            assert str(O.fnv1a_u32_stream(rich_flat(docs, terms, present, freq, pos))) == r["rich_fnv"], r["q"]
            hashed += 1
    assert hashed >= len(recs) // 2
    n_sets, n_hashes, n_info, n_d, n_s, n_cnt, n_counts, n_streams, n_rich = everything()  # default options: the narrow kernels
    assert n_info["tree_queries"] == info["tree_queries"]
    identical = True
    for i, r in enumerate(recs):
        assert np.array_equal(n_sets[i], sets[i]) and int(n_hashes[i]) == int(hashes[i]) and int(n_counts[i]) == int(counts[i]), r["q"]
        assert np.array_equal(n_d[i], d[i]) and int(n_cnt[i]) == int(cnt[i]), r["q"]
        np.testing.assert_allclose(s[i], n_s[i], rtol=1e-5, atol=0, err_msg=r["q"])
        assert np.array_equal(n_streams[i][0], streams[i][0]), r["q"]
        np.testing.assert_allclose(streams[i][1], n_streams[i][1], rtol=1e-5, atol=0, err_msg=r["q"])
        identical &= np.array_equal(streams[i][1], n_streams[i][1]) and np.array_equal(s[i], n_s[i])
        for a, b in zip(rich[i], n_rich[i]):  # docs, terms, present, freq, positions
            assert np.array_equal(a, b), r["q"]
    print(f"[wide trees] {corpus}: {len(recs)} trees, scores of the narrow and the wide kernels identical: {identical}")
    w.ix.close()


# ------------------------------------------------------------------------------------------ 2: trees only the wide kernels take, against the oracle
@pytest.mark.parametrize("shape", WORLDS, ids=["2000", "66000"])
def test_trees_of_more_than_64_nodes_match_the_oracle(T, dev, shape):
    """tree_max_nodes = 1024: eight shapes of 65 .. 200 nodes (an OR of conjunctions, a wide CNF, a matchsome of 130 children, a wide excluded side, a 33-level
    alternation, an <optional> side, phrases among the leaves) in DocumentsOnly, AccumulatedScore top-10 and full-stream mode, three of them in the default mode —
    without and with masked documents, and once more with a TRI_FILTER_DROP filter on every second query (the oracle drops the same documents)."""
    w = World(T, dev, *shape)
    D = shape[0]
    progs = shape_programs()
    memo = Memo(w.ora)
    hp = HP.HostPlan(HP.HostIndex.from_segment(w.seg), progs, T.FLAG_DOCUMENTS_ONLY, options=WIDE)
    for i, (name, *_rest) in enumerate(SHAPES):
        kind, nodes = hp.tree_kind(int(hp.slot_of_query[i]))
        assert hp.qstatus[i] == 0 and kind == HP.TREE_KIND_WIDE and nodes > 64, (name, nodes)
    hp.close()
    none = np.zeros(0, np.uint32)
    mask = masked_set(D)
    drop = np.array(sorted(set(np.random.default_rng(9).integers(1, D + 1, D // 5).tolist())), dtype=np.uint32)
    rich_idx = [i for i, sh in enumerate(SHAPES) if sh[3]]
    flt = None
    try:
        with options(dev, **WIDE):
            for tag, mk, filtered in (("plain", none, False), ("masked", mask, False), ("masked+filter", mask, True)):
                w.ix.set_masked(mk)
                if filtered and flt is None:
                    flt = T.Filter(w.ix, drop)
                gone = {False: ("masked" if len(mk) else "plain", mk), True: ("both", np.union1d(mk, drop).astype(np.uint32))}

                def want(i, rich=False):
                    key, dr = gone[filtered and i % 2 == 1]
                    return memo.get(key, dr, progs[i], rich)

                def batch(ps, idx, flags, topk=0):
                    b = T.Batch(w.ix, ps, flags, topk=topk)
                    if filtered:
                        b.set_filters([flt], [0 if i % 2 == 1 else T.engine.NO_FILTER for i in idx])
                    b.run()
                    b.sync()
                    return b

                allq = list(range(len(progs)))
                b = batch(progs, allq, T.FLAG_DOCUMENTS_ONLY)
                assert not b.query_status().any() and b.info()["tree_queries"] == len(progs) and b.info()["unsupported_queries"] == 0
                counts, hashes = b.counts(), b.docset_hashes()
                for i, sh in enumerate(SHAPES):
                    docs, _ = want(i)
                    if tag == "plain":
                        assert len(docs) == sh[4][WORLDS.index(shape)] > 0, (sh[0], len(docs))
                    assert int(counts[i]) == len(docs) > 0, (tag, sh[0], int(counts[i]), len(docs))
                    assert np.array_equal(b.docset(i, len(docs)), docs) and int(hashes[i]) == O.fnv1a_docs(docs), (tag, sh[0])
                b.close()
                for k in (10, 0):
                    b = batch(progs, allq, T.FLAG_ACCUMULATED_SCORE, k)
                    counts = b.counts()
                    tk = b.topk_results() if k else None
                    for i, sh in enumerate(SHAPES):
                        docs, scores = want(i)
                        assert int(counts[i]) == len(docs), (tag, k, sh[0])
                        if k:
                            td, ts = w.ora.topk(docs, scores, k)
                            assert tk[0][i, : len(td)].tolist() == td.tolist(), (tag, sh[0])
                            np.testing.assert_allclose(tk[1][i, : len(td)], ts, rtol=1e-5, atol=0, err_msg=sh[0])
                        else:
                            assert np.array_equal(b.docset(i, len(docs)), docs), (tag, sh[0])
                            np.testing.assert_allclose(b.scores(i, len(docs)), scores, rtol=1e-5, atol=0, err_msg=sh[0])
                    b.close()
                b = batch([progs[i] for i in rich_idx], rich_idx, T.FLAG_MATCHED_TERMS)
                assert not b.query_status().any() and b.info()["tree_queries"] == len(rich_idx)
                counts = b.counts()
                for j, i in enumerate(rich_idx):
                    wdocs, wflat, tt, ht = want(i, rich=True)
                    docs = b.docset(j, int(counts[j]))
                    terms, present, freq, pos = b.matched_terms(j, len(docs))
                    assert np.array_equal(docs, wdocs), (tag, SHAPES[i][0])
                    assert int(freq.sum()) == ht and int(sum(bin(int(x)).count("1") for x in present)) == tt, (tag, SHAPES[i][0])
                    assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), (tag, SHAPES[i][0])
                b.close()
    finally:
        if flt is not None:
            flt.close()
        w.ix.set_masked(none)
        w.ix.close()


# ------------------------------------------------------------------------------------------ 3: more distinct terms than the oracle takes
def test_vocabularies_past_the_oracles_64_terms_match_numpy(T, dev):
    """A flat OR of t20 .. t169 and a matchsome of t20 .. t119 (min 3): the docsets are what numpy makes of the decoded lists; the OR's scores are, per document,
    the sum of the scores of three 50-term ORs at default options — narrow trees, which the oracle pins."""
    w = World(T, dev, *WORLDS[0])
    lists = {t: w.ora.decode_term(t)[0] for t in range(20, 170)}
    wide_or = np.array([T.tok(T.OP_TERM, t) for t in range(20, 170)] + [T.tok(T.OP_OR, 150)], dtype=np.uint32)
    some = np.array([T.tok(T.OP_TERM, t) for t in range(20, 120)] + [T.tok(T.OP_SOME, (3 << 16) | 100)], dtype=np.uint32)
    thirds = [np.array([T.tok(T.OP_TERM, t) for t in range(a, a + 50)] + [T.tok(T.OP_OR, 50)], dtype=np.uint32) for a in (20, 70, 120)]
    union = np.unique(np.concatenate(list(lists.values())))
    held = np.bincount(np.concatenate([lists[t] for t in range(20, 120)]), minlength=w.D + 1)
    atleast3 = np.nonzero(held >= 3)[0].astype(np.uint32)
    assert len(union) and len(atleast3)
    with options(dev, **WIDE):
        sets, _, info = run_docs_only(w, [wide_or, some])
        assert info["tree_queries"] == 2 and info["unsupported_queries"] == 0
        full = T.Batch(w.ix, [wide_or], T.FLAG_ACCUMULATED_SCORE, topk=0)
        full.run()
        full.sync()
        n = int(full.counts()[0])
        docs, scores = full.docset(0, n), full.scores(0, n)
        full.close()
    assert np.array_equal(sets[0], union) and np.array_equal(sets[1], atleast3) and np.array_equal(docs, union)
    parts = T.Batch(w.ix, thirds, T.FLAG_ACCUMULATED_SCORE, topk=0)  # (default options: 51 nodes each, the narrow kernels)
    parts.run()
    parts.sync()
    assert parts.info()["tree_queries"] == 3
    total = np.zeros(w.D + 1, dtype=np.float64)
    pc = parts.counts()
    for j, third in enumerate(thirds):
        pd, ps = parts.docset(j, int(pc[j])), parts.scores(j, int(pc[j]))
        od, osc = w.ora.exec(third, O.FLAG_ACCUM_SCORE)
        assert np.array_equal(pd, od)
        np.testing.assert_allclose(ps, osc, rtol=1e-5, atol=0)
        total[pd] += ps
    parts.close()
    np.testing.assert_allclose(scores, total[docs], rtol=1e-5, atol=0)
    w.ix.close()


# ------------------------------------------------------------------------------------------ 4: the default
def test_default_options_still_leave_a_121_node_tree_out(T, dev):
    w = World(T, dev, *WORLDS[0])
    texts = ["t0 t1", BIG, 't0 OR "t1 t2"', "t3 OR t5 OR t9"]
    progs = [O.parse_query(t) for t in texts]
    assert dev.get_option("tree_max_nodes") == 64 and dev.get_option("tree_wide_min_nodes") == 65
    b = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY, allow_unsupported=True)
    assert b.query_status().tolist() == [0, -3, 0, 0] and b.info()["unsupported_queries"] == 1 and b.info()["tree_queries"] == 1
    b.run()
    b.sync()
    counts = b.counts()
    for i, p in enumerate(progs):
        want = w.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] if i != 1 else np.zeros(0, np.uint32)
        assert int(counts[i]) == len(want) and np.array_equal(b.docset(i, len(want)), want), texts[i]
    b.close()
    for bad in (63, 1025):
        with options(dev, tree_max_nodes=bad):
            with pytest.raises(T.TrinityError):
                T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY, allow_unsupported=True)
    w.ix.close()


# ------------------------------------------------------------------------------------------ 5: re-runs, collections
def test_wide_batches_rerun_and_run_as_parts_of_a_collection(T, dev):
    """A wide batch run twice answers twice the same (the hidden phrase queries' lists, the match bitmaps and the chunk counts are rebuilt); or-of-and with a narrow
    tree and a CNF beside it over a collection of two segments: counts add up, docsets concatenate, ONE top-10 over both."""
    old = World(T, dev, 20000, 2000, 10, 42)
    new = World(T, dev, 6000, 2000, 10, 7)
    try:
        old.ix.set_masked(np.arange(1, 6001, dtype=np.uint32))
        texts = [SHAPES[0][1], SHAPES[7][1], 't0 OR "t1 t2"', "t0 t1"]
        progs = [O.parse_query(t) for t in texts]
        with options(dev, **WIDE):
            b = T.Batch(new.ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=0)
            runs = []
            for rep in range(2):
                b.run()
                b.sync()
                c = b.counts()
                runs.append([(b.docset(i, int(c[i])), b.scores(i, int(c[i]))) for i in range(len(progs))])
            b.close()
            for (d0, s0), (d1, s1), p in zip(runs[0], runs[1], progs):
                wd, ws = new.ora.exec(p, O.FLAG_ACCUM_SCORE)
                assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(d0, wd)
                np.testing.assert_allclose(s0, ws, rtol=1e-5, atol=0)
            parts = [T.Batch(x.ix, progs, T.FLAG_DOCUMENTS_ONLY) for x in (old, new)]
            cb = T.CollectionBatch(parts)
            cb.run()
            cb.sync()
            counts = cb.counts()
            sparts = [T.Batch(x.ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=10) for x in (old, new)]
            sb = T.CollectionBatch(sparts)
            sb.run()
            sb.sync()
            d, s, c = sb.topk_results()
            scounts = sb.counts()
        for i, (t, p) in enumerate(zip(texts, progs)):
            do, so = old.ora.exec(p, O.FLAG_ACCUM_SCORE)
            keep = do > 6000
            dn, sn = new.ora.exec(p, O.FLAG_ACCUM_SCORE)
            want = np.concatenate([do[keep], dn])
            assert int(counts[i]) == len(want) == int(scounts[i]) and len(want), t
            assert np.array_equal(cb.docset(i, len(want)), want), t
            td, ts = old.ora.topk(want, np.concatenate([so[keep], sn]), 10)
            assert int(c[i]) == len(td) and d[i, : len(td)].tolist() == td.tolist(), t
            np.testing.assert_allclose(s[i, : len(td)], ts, rtol=1e-5, atol=0)
        cb.close()
        sb.close()
        for x in parts + sparts:
            x.close()
    finally:
        old.ix.close()
        new.ix.close()
