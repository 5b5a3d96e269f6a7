"""GPU tests of the default mode's device ranker (run with -m gpu on an MI355X): tri_batch_set_ranker / tri_batch_ranked — k_rich_rank and k_rank_merge
(csrc/k_rich_rank.hpp) behind the two k_rich passes.  The expected lists never come from the engine: tests/rank_cases.py restates the score in plain Python over
the CPU oracle's default mode (exec_rich), and every comparison is bit for bit — docIDs, the scores' 64 bits, counts, and zero rows past the count."""
import ctypes as C

import numpy as np
import pytest

import decode_hits_cases as DC
import oracle_lib as O
import rank_cases as R
from test_gpu_parity import World, options
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)
from wide_terms_cases import NARROW, NARROW_MIN, OPTS, SHAPES, WORLDS, mixed_programs, narrow_programs, shape_programs

pytestmark = pytest.mark.gpu
CASES = [(wi, codec) for wi in range(len(WORLDS)) for codec in (1, 2)]
IDS = [f"{WORLDS[wi][0]}-codec{codec}" for wi, codec in CASES]
RANK_LANE_RUN = 128  # csrc/k_rich_rank.hpp: two neighbouring runs of more hits than this together go to a whole wave
CAP, ADJ = 3, 4.0


def w3(k):
    return 1 + k % 3


# the queries of test 1: the narrow shapes, a conjunction whose slot order is not its term order, one that matches nothing, one the default mode leaves out
def parity_texts(V):
    return NARROW + ["t3 t1 t0", " ".join(f"t{V - 1 - i}" for i in range(5)), SHAPES[0][1]]


PAIR_QUERIES = ["t0 t1", "t0 OR t1 OR t2", '"t0 t1" OR "t1 t2" OR "t2 t3"', 't0 <"t1 t2">', NARROW[5]]  # (+ the 17-term OR: test 5)

_ORA, _RECS, _ROWS = {}, {}, {}


def oracle_of(wi):
    """The expectations' oracle: one Google-coded index per world (both codecs hold the same corpus and answer alike — tests/test_abi.py)."""
    if wi not in _ORA:
        _ORA[wi] = O.Index.generate(*WORLDS[wi])
    return _ORA[wi]


def recs_of(wi, prog, key="plain", drop=None):
    k = (wi, key, np.asarray(prog, dtype=np.uint32).tobytes())
    if k not in _RECS:
        ora = oracle_of(wi)
        if drop is not None:
            ora.set_masked(drop)
        try:
            _RECS[k] = R.records(ora.exec_rich(prog)[1])
        finally:
            if drop is not None:
                ora.set_masked(np.zeros(0, np.uint32))
    return _RECS[k]


def want_rows(wi, prog, cap, adj, fn, key="plain", drop=None):
    """The query's whole expected ranking [(doc, score, pairs)] under weights fn(slot) (None: 1.0), computed once and shared"""
    k = (wi, key, np.asarray(prog, dtype=np.uint32).tobytes(), cap, adj, None if fn is None else tuple(fn(i) for i in range(64)))
    if k not in _ROWS:
        w = None if fn is None else R.token_weights([prog], fn)
        _ROWS[k] = R.rows(recs_of(wi, prog, key, drop), prog, cap, adj, w)
    return _ROWS[k]


def run_ranked(T, ix, progs, K, cap=CAP, adj=ADJ, fn=w3, flags=None, allow_unsupported=False, filters=None, weights=None):
    """-> (docids, scores, counts, status, info) of one ranked batch"""
    b = T.Batch(ix, progs, T.FLAG_MATCHED_TERMS if flags is None else flags, allow_unsupported=allow_unsupported)
    try:
        b.set_ranker(K, cap, adj, weights if weights is not None else (None if fn is None else R.token_weights(progs, fn)))
        if filters is not None:
            b.set_filters(*filters)
        b.run()
        b.sync()
        return b.ranked() + (b.query_status(), b.info())
    finally:
        b.close()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check_row(d, s, c, qi, rows, K, name):
    n = min(len(rows), K)
    got = list(zip(d[qi, :n].tolist(), bits(s[qi, :n]).tolist()))
    want = [(r[0], int(bits([r[1]])[0])) for r in rows[:n]]
    if got != want:
        at = next(i for i in range(n) if got[i] != want[i])
        print(f"[rank] {name} K {K}: first difference at rank {at}: got (doc {got[at][0]}, {s[qi, at]!r}) want (doc {want[at][0]}, {rows[at][1]!r}, pairs {rows[at][2]})")
    assert int(c[qi]) == n, (name, K, int(c[qi]), n)
    assert got == want, (name, K)
    assert not d[qi, n:].any() and not bits(s[qi, n:]).any(), (name, K)  # rows past the count are zero


@pytest.fixture(scope="module")
def worlds(T, dev):
    made = {}

    def get(case):
        if case not in made:
            made[case] = World(T, dev, *WORLDS[case[0]], codec=case[1])
        return made[case]

    yield get
    for w in made.values():
        w.ix.close()


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ranked_lists_equal_the_restatement(T, worlds, case):
    wi = case[0]
    w = worlds(case)
    texts = parity_texts(WORLDS[wi][1])
    progs = [O.parse_query(t, some_min=NARROW_MIN) for t in texts]
    zero, left_out = len(texts) - 2, len(texts) - 1
    assert len(recs_of(wi, progs[zero])) == 0
    for K in (1, 10, 256):
        d, s, c, status, info = run_ranked(T, w.ix, progs, K, allow_unsupported=True)
        assert status.tolist() == [0] * left_out + [-3] and info["unsupported_queries"] == 1  # 17 reportable terms at rich_max_terms = 16
        assert int(c[left_out]) == 0 and not d[left_out].any() and not bits(s[left_out]).any()
        for qi in range(left_out):
            check_row(d, s, c, qi, want_rows(wi, progs[qi], CAP, ADJ, w3), K, texts[qi])
    # the lists cannot be had from the frequencies alone: the expected top-10 holds a document with a pair, and differs from the adjacency-0 top-10
    for text in PAIR_QUERIES:
        prog = progs[texts.index(text)]
        top = want_rows(wi, prog, CAP, ADJ, w3)[:10]
        flat = want_rows(wi, prog, CAP, 0.0, w3)[:10]
        assert any(r[2] for r in top) and [r[0] for r in top] != [r[0] for r in flat], text
        assert sum(1 for r in want_rows(wi, prog, CAP, ADJ, w3) if r[1] == top[9][1]) >= 3, text  # documents tied at the 10th score: the docID rule decides the list


# ------------------------------------------------------------------------------------------ 2
def test_all_ties_go_to_the_lowest_docids(T, worlds):
    w = worlds((0, 1))
    progs = [O.parse_query("t0 t1"), O.parse_query("t0 OR t1 OR t2")]
    conj = w.ora.exec(progs[0], O.FLAG_DOCUMENTS_ONLY)[0]
    for K in (1, 10, 256):
        d, s, c, _, _ = run_ranked(T, w.ix, progs, K, cap=1, adj=0.0, fn=None)
        n = min(K, len(conj))
        assert int(c[0]) == n and d[0, :n].tolist() == conj[:n].tolist() and np.all(s[0, :n] == 2.0)
        check_row(d, s, c, 0, want_rows(0, progs[0], 1, 0.0, None), K, "t0 t1")
        check_row(d, s, c, 1, want_rows(0, progs[1], 1, 0.0, None), K, "t0 OR t1 OR t2")


# ------------------------------------------------------------------------------------------ 3
def test_non_dyadic_weights_are_not_contracted(T, worlds):
    """Weights and an adjacency no power of two divides: a fused multiply-add anywhere in the sum rounds once where the contract rounds twice."""
    w = worlds((0, 1))
    vals = [0.1, -0.7, 1.0 / 3.0, 0.45, 2.3, 0.9]

    def fn(k):
        return vals[k % len(vals)]

    texts = ["t0 t1", "t0 OR t1 OR t2", NARROW[5], NARROW[6], "t3 t1 t0"]
    progs = [O.parse_query(t, some_min=NARROW_MIN) for t in texts]
    d, s, c, _, _ = run_ranked(T, w.ix, progs, 256, cap=5, adj=0.3, fn=fn)
    for qi, text in enumerate(texts):
        rows = want_rows(0, progs[qi], 5, 0.3, fn)
        check_row(d, s, c, qi, rows, 256, text)
    assert any(r[1] < 0 for r in want_rows(0, progs[0], 5, 0.3, fn))  # (the negative weight shows)


# ------------------------------------------------------------------------------------------ 4
def test_many_tasks_per_query(T, dev, worlds):
    """tri_batch_info carries no task count (and does not grow), so the "more tasks than queries" assertion is made on the HOST planner's cut of the same batch under
    the same options (trinity_amd.hostplan: the planner.hpp tri_batch_create includes) — not on what the device batch was actually cut into, which nothing reports."""
    from trinity_amd import hostplan as HP

    w = worlds((1, 1))
    progs = narrow_programs(O)
    cut = {"cand_task_cost": 4096, "dense_task_cost": 4096}
    hi = HP.HostIndex.from_segment(w.seg)
    try:
        plan = HP.HostPlan(hi, progs, T.FLAG_MATCHED_TERMS, options=cut)
        per_query = [int(q["ntasks"]) for q in plan.plan if q["qid"] != 0xFFFFFFFF]
        assert plan.s["n_tasks"] > len(progs) and max(per_query) > 1, (plan.s["n_tasks"], per_query)
    finally:
        hi.close()
    plain = run_ranked(T, w.ix, progs, 10)
    with options(dev, **cut):
        many = run_ranked(T, w.ix, progs, 10)
    for qi, text in enumerate(NARROW):
        rows = want_rows(1, progs[qi], CAP, ADJ, w3)
        check_row(*many[:3], qi, rows, 10, text + " (many tasks)")
        check_row(*plain[:3], qi, rows, 10, text)
    for a, b in zip(plain[:3], many[:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("case", [(0, 1), (0, 2), (1, 1)], ids=["2000-codec1", "2000-codec2", "66000-codec1"])
def test_wide_report_queries(T, dev, worlds, case):
    wi = case[0]
    w = worlds(case)
    names = [sh[0] for sh in SHAPES]
    shapes = shape_programs(O)
    wide = [shapes[names.index(n)] for n in ("or17", "or64", "straddle")]
    mixed, narrow_at = mixed_programs(O)
    progs = wide + mixed
    with options(dev, **OPTS):
        d, s, c, status, info = run_ranked(T, w.ix, progs, 10)
    assert not status.any() and info["tree_queries"] >= len(wide) + len(shapes)
    for qi, prog in enumerate(progs):
        check_row(d, s, c, qi, want_rows(wi, prog, CAP, ADJ, w3), 10, f"query {qi}")
    # the narrow queries of the mixed batch rank as they do alone
    narrow = narrow_programs(O)
    da, sa, ca, _, _ = run_ranked(T, w.ix, narrow, 10)
    for j, qi in enumerate(narrow_at):
        q = len(wide) + qi
        assert int(c[q]) == int(ca[j]) and np.array_equal(d[q], da[j]) and np.array_equal(bits(s[q]), bits(sa[j])), NARROW[j]
    top = want_rows(wi, wide[0], CAP, ADJ, w3)[:10]  # the 17-term OR: pairs decide its list too
    assert any(r[2] for r in top) and [r[0] for r in top] != [r[0] for r in want_rows(wi, wide[0], CAP, 0.0, w3)[:10]]


# ------------------------------------------------------------------------------------------ 6
LONGDOCS = (6000, 400, 90, 11)


def test_long_documents(T, dev):
    """Frequencies up to 29, up to 41 hits a row, up to 8 pairs a match."""
    w = World(T, dev, *LONGDOCS)
    try:
        texts = ["t0 t1", "t0 OR t1 OR t2", NARROW[6], "t3 t1 t0"]
        progs = [O.parse_query(t) for t in texts]
        d, s, c, _, _ = run_ranked(T, w.ix, progs, 10, cap=40)
        for qi, text in enumerate(texts):
            recs = R.records(w.ora.exec_rich(progs[qi])[1])
            rows = R.rows(recs, progs[qi], 40, ADJ, R.token_weights([progs[qi]], w3))
            if qi == 1:
                assert max(f for _, t in recs for f, _ in t.values()) >= 20 and max(r[2] for r in rows) >= 4
            check_row(d, s, c, qi, rows, 10, text)
    finally:
        w.ix.close()


def long_rows_case(T):
    """Two terms, a at odd and b at even positions.  Document 5: 100 + 100 hits (above RANK_LANE_RUN: a wave counts its pairs); 9: 64 + 64 = the bound exactly (a
    lane); 10: 65 + 64, one above; 20: 3000 + 3000; 12: both terms, no pair; 30: one pair; 21 / 22: one term each."""
    half = RANK_LANE_RUN // 2
    A = {5: list(range(1, 201, 2)), 9: list(range(1, 2 * half + 1, 2)), 10: list(range(1, 2 * half + 3, 2)), 12: [1, 3, 5], 20: list(range(1, 6001, 2)), 21: [7], 30: [4, 9]}
    B = {5: list(range(2, 202, 2)), 9: list(range(2, 2 * half + 2, 2)), 10: list(range(2, 2 * half + 2, 2)), 12: [10, 20], 20: list(range(2, 6002, 2)), 22: [8], 30: [5, 11]}
    assert len(A[9]) + len(B[9]) == RANK_LANE_RUN and len(A[10]) + len(B[10]) == RANK_LANE_RUN + 1
    docs, freqs, pos, tf = [], [], [], [0]
    for X in (A, B):
        for doc in sorted(X):
            docs.append(doc)
            freqs.append(len(X[doc]))
            pos += X[doc]
        tf.append(len(docs))
    index, terms = T.engine.host_encode_google(np.array(docs, np.uint32), np.array(freqs, np.uint32), np.array(pos, np.uint16), np.array(tf, np.uint64))
    return index, terms, 40, len(docs), len(pos)


def test_rows_longer_than_a_lane_takes(T, dev):
    index, terms, docs_cnt, postings, hits = long_rows_case(T)
    ora = O.Index.wrap(index, terms, docs_cnt, postings, hits)
    ix = T.Index(dev, index, terms, docs_cnt)
    try:
        texts = ["t0 t1", "t0 OR t1", "t1 t0"]
        progs = [O.parse_query(t) for t in texts]
        d, s, c, _, _ = run_ranked(T, ix, progs, 10, cap=3)
        for qi, text in enumerate(texts):
            rows = R.rows(R.records(ora.exec_rich(progs[qi])[1]), progs[qi], 3, ADJ, R.token_weights([progs[qi]], w3))
            check_row(d, s, c, qi, rows, 10, text)
        rows = R.rows(R.records(ora.exec_rich(progs[0])[1]), progs[0], 3, ADJ, None)
        assert {r[0]: r[2] for r in rows} == {20: 3000, 5: 100, 9: 64, 10: 64, 30: 1, 12: 0}
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 7
def zero_position_case(T):
    """Hits at position 0 (legal only with a payload).  Document 5: term 0 sits at 0, term 1 at 1 — no pair; document 3: term 0 at 0 and 4, term 1 at 5 — one pair."""
    docs = [3, 5, 8, 3, 5, 9]
    freqs = [2, 1, 1, 1, 2, 1]
    pos = [0, 4, 0, 6, 5, 1, 7, 2]
    lens = [2, 0, 1, 0, 0, 0, 0, 0]
    words = [0xBEEF, 0, 0x7F, 0, 0, 0, 0, 0]
    index, terms = T.engine.host_encode_google(np.array(docs, np.uint32), np.array(freqs, np.uint32), np.array(pos, np.uint16), np.array([0, 3, 6], np.uint64),
                                               np.array(lens, np.uint8), np.array(words, np.uint64))  # fmt: skip
    return index, terms, 20, len(docs), len(pos)


@pytest.mark.parametrize("make", [lambda T: DC.payload_case(), zero_position_case], ids=["payload_case", "position0"])
def test_payload_segments_rank_alike_with_and_without_the_payload_flag(T, dev, make):
    index, terms, docs_cnt, postings, hits = make(T)
    ora = O.Index.wrap(index, terms, docs_cnt, postings, hits)
    ix = T.Index(dev, index, terms, docs_cnt)
    try:
        texts = ["t0 t1", "t0 OR t1", "t1 t0"] + (["t0 OR t1 OR t2", "t2 t1"] if len(terms) > 2 else [])
        progs = [O.parse_query(t) for t in texts]
        plain = run_ranked(T, ix, progs, 10)
        flagged = run_ranked(T, ix, progs, 10, flags=T.FLAG_MATCHED_TERMS | T.FLAG_HIT_PAYLOADS)
        for a, b in zip(plain[:3], flagged[:3]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        for qi, text in enumerate(texts):
            recs = R.records(ora.exec_rich(progs[qi])[1])
            check_row(*flagged[:3], qi, R.rows(recs, progs[qi], CAP, ADJ, R.token_weights([progs[qi]], w3)), 10, text)
        if make is zero_position_case:
            recs = dict(R.records(ora.exec_rich(progs[0])[1]))
            assert recs[5][0][1] == [0] and recs[5][1][1] == [1, 7] and R.pairs_of(recs[5], [0, 1]) == 0  # 0 next to 1: not a pair
            assert recs[3][0][1] == [0, 4] and recs[3][1][1] == [5] and R.pairs_of(recs[3], [0, 1]) == 1
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("case", [(0, 1), (0, 2)], ids=["2000-codec1", "2000-codec2"])
def test_masked_documents_and_per_query_filters(T, worlds, case):
    wi = case[0]
    w = worlds(case)
    D = WORLDS[wi][0]
    mask = np.array(sorted(set(np.random.default_rng(3).integers(1, D, D // 7).tolist())), dtype=np.uint32)
    drop = np.array(sorted(set(np.random.default_rng(9).integers(1, D + 1, D // 5).tolist())), dtype=np.uint32)
    keep = np.array(sorted(set(np.random.default_rng(5).integers(1, D + 1, D // 2).tolist())), dtype=np.uint32)
    texts = ["t0 t1", "t0 OR t1 OR t2", NARROW[6], "t3 t1 t0"]
    progs = [O.parse_query(t) for t in texts]
    gone = {"mask": mask, "drop": np.union1d(mask, drop).astype(np.uint32), "keep": np.union1d(mask, np.setdiff1d(np.arange(1, D + 1), keep)).astype(np.uint32)}
    fdrop = fkeep = None
    try:
        w.ix.set_masked(mask)
        fdrop, fkeep = T.Filter(w.ix, drop), T.Filter(w.ix, keep, keep=True)
        NO = T.engine.NO_FILTER
        for foq, keys in (([NO] * 4, ["mask"] * 4), ([0, 1, NO, 0], ["drop", "keep", "mask", "drop"])):
            d, s, c, _, _ = run_ranked(T, w.ix, progs, 10, filters=([fdrop, fkeep], foq))
            for qi, key in enumerate(keys):
                check_row(d, s, c, qi, want_rows(wi, progs[qi], CAP, ADJ, w3, key, gone[key]), 10, f"{texts[qi]} ({key})")
    finally:
        for f in (fdrop, fkeep):
            if f is not None:
                f.close()
        w.ix.set_masked(np.zeros(0, np.uint32))


# ------------------------------------------------------------------------------------------ 9
def test_lifecycle(T, worlds):
    w = worlds((0, 1))
    texts = ["t0 t1", "t0 OR t1 OR t2"]
    progs = [O.parse_query(t) for t in texts]
    never = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS)
    b = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS)
    try:
        base = never.info()["launches"]
        b.set_ranker(10, CAP, ADJ, R.token_weights(progs, w3))
        assert b.info()["launches"] == base + 2  # k_rich_rank + k_rank_merge
        with pytest.raises(T.TrinityError, match="tri_batch_sync"):
            b.ranked()  # not run yet
        lists = []
        for _ in range(2):  # a second run / sync gives the same lists
            b.run()
            b.sync()
            lists.append(b.ranked())
        for x, y in zip(*lists):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for qi, text in enumerate(texts):
            check_row(*lists[0], qi, want_rows(0, progs[qi], CAP, ADJ, w3), 10, text)
        # matched_terms on a ranked batch still equals the oracle
        from test_gpu_parity import rich_flat

        counts = b.counts()
        for qi, prog in enumerate(progs):
            docs = b.docset(qi, int(counts[qi]))
            wdocs, wflat, _, _ = w.ora.exec_rich(prog)
            assert np.array_equal(docs, wdocs) and np.array_equal(rich_flat(docs, *b.matched_terms(qi, len(docs))), wflat)
        # replacing the ranker between runs takes effect
        b.set_ranker(5, 1, 0.0, None)
        with pytest.raises(T.TrinityError, match="tri_batch_sync"):
            b.ranked()  # (set after the last sync: nothing ranked under it yet)
        b.run()
        b.sync()
        d, s, c = b.ranked()
        assert d.shape == (2, 5)
        for qi, text in enumerate(texts):
            check_row(d, s, c, qi, want_rows(0, progs[qi], 1, 0.0, None), 5, text + " (replaced)")
        # clearing it
        b.clear_ranker()
        assert b.info()["launches"] == base
        b.run()
        b.sync()
        with pytest.raises(T.TrinityError, match="no ranker"):
            b.ranked()
        assert b.info()["launches"] == never.info()["launches"]
    finally:
        b.close()
        never.close()


def test_refusals_name_the_field(T, worlds):
    w = worlds((0, 1))
    L = T.engine.hip_lib()
    progs = [O.parse_query("t0 t1")]
    ntok = len(progs[0])
    b = T.Batch(w.ix, progs, T.FLAG_MATCHED_TERMS)
    other = T.Batch(w.ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        b.set_ranker(7, 2, 1.5, None)
        b.run()
        b.sync()
        before = b.ranked()

        def refused(batch, word, kind=1, topk=10, cap=3, reserved=0, adj=4.0, weights=None):
            spec = T.engine.TriRanker(kind, topk, cap, reserved, adj)
            wt = None if weights is None else np.array(weights, dtype=np.float64)
            assert L.tri_batch_set_ranker(batch.h, C.byref(spec), None if wt is None else wt.ctypes.data) == -1  # TRI_ERR_INVALID
            assert word.encode() in L.tri_last_error(), (word, L.tri_last_error())

        refused(other, "mode")
        refused(b, "topk", topk=0)
        refused(b, "topk", topk=257)
        refused(b, "freq_cap", cap=0)
        refused(b, "kind", kind=2)
        refused(b, "reserved", reserved=1)
        refused(b, "adjacency", adj=float("nan"))
        refused(b, "adjacency", adj=float("inf"))
        refused(b, "adjacency", adj=-1.0)
        refused(b, "weights", weights=[1.0] * (ntok - 1) + [float("inf")])
        refused(b, "weights", weights=[float("nan")] + [1.0] * (ntok - 1))
        # ... and left the batch as it was
        after = b.ranked()
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert after[0].shape == (1, 7)
        b.set_ranker(3, 1, 0.0, [-1.0] * ntok)  # negative weights are legal
        d = np.zeros(3, np.uint32)
        assert L.tri_batch_ranked(other.h, d.ctypes.data, d.ctypes.data, d.ctypes.data) == -1 and b"no ranker" in L.tri_last_error()
    finally:
        b.close()
        other.close()
