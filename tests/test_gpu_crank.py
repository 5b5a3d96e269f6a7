"""GPU tests of the default mode over a COLLECTION of segments (run with -m gpu on an MI355X): tri_cbatch_ranked — k_rank_merge_sources (csrc/k_rich_rank.hpp) behind
the parts' own rank passes — and tri_cbatch_matched_terms[_wide] / tri_cbatch_matched_payloads.  The expected lists never come from the engine: tests/crank_cases.py
blends, by a stable sort, the per-source restatements of tests/rank_cases.py over the CPU oracle's default mode; every comparison is bit for bit — docIDs, the
scores' 64 bits, counts, and zero rows past the count."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import crank_cases as CR
import decode_hits_cases as DC
import oracle_lib as O
import rank_cases as R
from test_gpu_parity import options, rich_flat
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)
from test_gpu_rank import PAIR_QUERIES, bits, check_row, parity_texts, zero_position_case
from wide_terms_cases import NARROW_MIN, OPTS, SHAPES

pytestmark = pytest.mark.gpu
CAP, ADJ, w3 = CR.CAP, CR.ADJ, CR.w3
V = CR.WORLDS[0][1]
NONE = np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def sources(T, dev):
    """codec -> the collection's indexes, oldest first (no masks installed)"""
    made = {}

    def get(codec):
        if codec not in made:
            made[codec] = [T.Index.from_segment(dev, T.Segment(*w, codec=codec)) for w in CR.WORLDS]
        return made[codec]

    yield get
    for ixs in made.values():
        for ix in ixs:
            ix.close()


@contextlib.contextmanager
def masked(ixs, masks=None):
    """Every source masked by the documents the newer ones update (crank_cases.masks)"""
    for ix, m in zip(ixs, CR.masks() if masks is None else masks):
        ix.set_masked(m)
    try:
        yield
    finally:
        for ix in ixs:
            ix.set_masked(NONE)


@contextlib.contextmanager
def collection(T, ixs, progs, flags=None, allow_unsupported=False, topk=0):
    """-> (CollectionBatch, parts); progs: one list for every part, or a list of lists, one per part"""
    per_part = progs if isinstance(progs[0], list) else [progs] * len(ixs)
    parts, cb = [], None
    try:
        for ix, p in zip(ixs, per_part):
            parts.append(T.Batch(ix, p, T.FLAG_MATCHED_TERMS if flags is None else flags, topk=topk, allow_unsupported=allow_unsupported))
        cb = T.CollectionBatch(parts, allow_unsupported=allow_unsupported)
        yield cb, parts
    finally:
        if cb is not None:
            cb.close()
        for b in parts:
            b.close()


def set_rankers(parts, progs, K, cap=CAP, adj=ADJ, fn=w3):
    per_part = progs if isinstance(progs[0], list) else [progs] * len(parts)
    for b, p in zip(parts, per_part):
        b.set_ranker(K, cap, adj, None if fn is None else R.token_weights(p, fn))


def run_ranked(T, ixs, progs, K, cap=CAP, adj=ADJ, fn=w3, allow_unsupported=False):
    """-> (docids, scores, counts, status) of one ranked collection batch"""
    with collection(T, ixs, progs, allow_unsupported=allow_unsupported) as (cb, parts):
        set_rankers(parts, progs, K, cap, adj, fn)
        cb.run()
        cb.sync()
        return cb.ranked() + (cb.query_status(),)


def same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("codec", [1, 2])
def test_merged_lists_equal_the_restatement(T, sources, codec):
    assert PAIR_QUERIES == CR.PAIR_QUERIES
    ixs = sources(codec)
    texts = parity_texts(V)
    progs = [O.parse_query(t, some_min=NARROW_MIN) for t in texts]
    zero, left_out = len(texts) - 2, len(texts) - 1
    assert CR.want(progs[zero], 256, CAP, ADJ, w3) == []
    # the 17-term OR: a part leaves it out when its source knows all 17 terms (rich_max_terms = 16) and contributes nothing; the newest source lacks one of them
    # and runs it as a 16-term query
    ran = [si for si in range(len(ixs)) if len(CR.present_slots(si, progs[left_out])) <= 16]
    assert ran == [2]
    # K = 256: a query's merge takes up to 256 entries from each of the two older sources and the newest one's 20 documents
    assert max(sum(min(len(rows), 256) for rows in CR.source_rows(p, CAP, ADJ, w3)) for p in progs[:left_out]) > 512
    with masked(ixs):
        for K in (1, 10, 256):
            d, s, c, status = run_ranked(T, ixs, progs, K, allow_unsupported=True)
            assert status.tolist() == [0] * left_out + [-3]
            lists = CR.source_rows(progs[left_out], CAP, ADJ, w3)
            check_row(d, s, c, left_out, CR.blend([rows if si in ran else [] for si, rows in enumerate(lists)], K), K, texts[left_out])
            for qi in range(left_out):
                check_row(d, s, c, qi, CR.want(progs[qi], K, CAP, ADJ, w3), K, texts[qi])
    # ... and left out in every part (the two older sources alone): count 0, zero rows, status -3
    with masked(ixs[:2], CR.masks()[:2]):
        d, s, c, status = run_ranked(T, ixs[:2], progs, 10, allow_unsupported=True)
    assert status.tolist() == [0] * left_out + [-3]
    assert int(c[left_out]) == 0 and not d[left_out].any() and not bits(s[left_out]).any()


# ------------------------------------------------------------------------------------------ 2
def test_all_ties_go_to_the_lowest_docids_of_the_collection(T, sources):
    """freq_cap 1, adjacency 0, NULL weights: every match of a single term or of a conjunction has the same score — the list is the K lowest docIDs of the collection,
    and with the masks on those are a NEWER source's: a merge that takes the sources in order fails.  (An OR's matches score by how many terms they hold.)"""
    ixs = sources(1)
    texts = ["t5", "t0 t1", "t0 OR t1 OR t2"]
    progs = [O.parse_query(t) for t in texts]
    with masked(ixs):
        for K in (1, 10, 256):
            d, s, c, _ = run_ranked(T, ixs, progs, K, cap=1, adj=0.0, fn=None)
            for qi, text in enumerate(texts):
                want = CR.want(progs[qi], K, 1, 0.0, None)
                check_row(d, s, c, qi, want, K, text)
                if qi < 2:
                    assert len({r[1] for r in want}) == 1 and [r[0] for r in want] == sorted(r[0] for r in want), text
                    assert want[0][-1] > 0 and (K < 256 or len({r[-1] for r in want}) > 1), text  # a newer source leads (its docIDs are the lowest), an older one follows


# ------------------------------------------------------------------------------------------ 3
def test_the_same_docid_in_several_sources(T, sources):
    """No masks: the sources' docID ranges overlap.  All ties (zero weights on an OR of the 16 head terms, which every document matches): documents 1 .. 20 appear three
    times each and the following ones twice, exactly as the stable sort says."""
    ixs = sources(1)
    texts = [" OR ".join(f"t{i}" for i in range(16)), "t5", "t0 t1"]
    progs = [O.parse_query(t) for t in texts]
    every = CR.source_rows(progs[0], 1, 0.0, lambda k: 0.0, masked=False)
    assert [len(rows) for rows in every] == [w[0] for w in CR.WORLDS]  # every document of every source matches
    with collection(T, ixs, progs) as (cb, parts):
        for b in parts:
            b.set_ranker(256, 1, 0.0, [0.0] * sum(len(p) for p in progs))
        cb.run()
        cb.sync()
        d, s, c = cb.ranked()
    n3 = CR.WORLDS[2][0]
    assert int(c[0]) == 256 and d[0].tolist() == ([x for doc in range(1, n3 + 1) for x in (doc,) * 3] + [x for doc in range(n3 + 1, 600) for x in (doc, doc)])[:256]
    for qi, text in enumerate(texts):
        check_row(d, s, c, qi, CR.want(progs[qi], 256, 1, 0.0, lambda k: 0.0, masked=False), 256, text)
    # ... and under NULL weights, where the duplicates fall wherever the oracle's sources share a match
    d, s, c, _ = run_ranked(T, ixs, progs[1:], 256, cap=1, adj=0.0, fn=None)
    for qi, text in enumerate(texts[1:]):
        want = CR.want(progs[1 + qi], 256, 1, 0.0, None, masked=False)
        assert len({r[0] for r in want}) < len(want), text
        check_row(d, s, c, qi, want, 256, text)


# ------------------------------------------------------------------------------------------ 4
def shifted(prog, by):
    """The program with every term id moved by `by`: the query resolved against a source that knows none of its terms (ids past its term table, one per term)"""
    return np.array([int(t) + by if (int(t) >> 28) == R.OP_TERM else int(t) for t in prog], dtype=np.uint32)


def test_a_part_that_knows_none_of_the_terms(T, dev, sources):
    ixs = sources(1)
    texts = ["t0 t1", "t0 OR t1 OR t2", '"t0 t1" OR "t1 t2" OR "t2 t3"', "t5"]
    progs = [O.parse_query(t) for t in texts]
    # a fourth, newest source: two terms of its own; the queries' terms resolve to ids past its table
    index, terms = T.engine.host_encode_google(np.array([1, 2, 3, 2, 4], np.uint32), np.array([1, 1, 1, 1, 1], np.uint32), np.array([1, 2, 3, 4, 5], np.uint16), np.array([0, 3, 5], np.uint64))
    stranger = T.Index(dev, index, terms, 10)
    try:
        with masked(ixs):
            three = run_ranked(T, ixs, progs, 10)
            with collection(T, ixs + [stranger], [progs, progs, progs, [shifted(p, len(terms)) for p in progs]]) as (cb, parts):
                set_rankers(parts, progs, 10)  # (the same tokens carry the weights in the shifted programs)
                for _ in range(2):
                    cb.run()
                    cb.sync()
                    four = cb.ranked()
                    assert not parts[3].counts().any() and not parts[3].ranked()[2].any()
                    assert same(three[:3], four)
            for qi, text in enumerate(texts):
                check_row(*four, qi, CR.want(progs[qi], 10, CAP, ADJ, w3), 10, text)
    finally:
        stranger.close()


# ------------------------------------------------------------------------------------------ 5
GUARD = 8


def guarded(n, dtype):
    a = np.empty(n + 2 * GUARD, dtype=dtype)
    a.view(np.uint8)[:] = 0xA5
    return a


def intact(a):
    g = a.view(np.uint8)
    w = GUARD * a.itemsize
    return bool((g[:w] == 0xA5).all() and (g[len(g) - w :] == 0xA5).all())


def inner(a):
    return a.ctypes.data + GUARD * a.itemsize


def concat_rows(parts, q, wide=False):
    """The parts' own calls, source after source: (docs, present, freq, positions)"""
    docs, present, freq, pos = [], [], [], []
    for b in parts:
        ds = b.docset(q)
        if not len(ds):
            continue  # (no rows; a source that knows none of the query's terms reports no columns either)
        _, p, f, ps = (b.matched_terms_wide if wide else b.matched_terms)(q, len(ds))
        docs.append(ds), present.append(p), freq.append(f), pos.append(ps)
    return np.concatenate(docs), np.concatenate(present), np.concatenate(freq), np.concatenate(pos)


def test_rows_are_the_parts_rows_source_after_source(T, dev, sources):
    ixs = sources(1)
    L = T.engine.hip_lib()
    texts = ["t0 t1", "t0 OR t1 OR t2", '"t0 t1" OR "t1 t2" OR "t2 t3"', 't0 <"t1 t2">', "t5"]
    progs = [O.parse_query(t) for t in texts]
    with masked(ixs), collection(T, ixs, progs) as (cb, parts):
        cb.run()
        cb.sync()
        counts = cb.counts()
        for qi, text in enumerate(texts):
            n = int(counts[qi])
            docs, present, freq, pos = concat_rows(parts, qi)
            cdocs = cb.docset(qi, n)
            terms, cpresent, cfreq, cpos = cb.matched_terms(qi, n)
            assert np.array_equal(cdocs, docs) and np.array_equal(cpresent, present) and np.array_equal(cfreq, freq) and np.array_equal(cpos, pos), text
            _, wpresent, wfreq, wpos = cb.matched_terms_wide(qi, n)
            assert wpresent.dtype == np.uint64 and np.array_equal(wpresent, present.astype(np.uint64)) and np.array_equal(wfreq, freq) and np.array_equal(wpos, pos), text
            # ... and the oracle's: each source's default-mode stream under its mask, one after the other
            flats = []
            for si in range(len(ixs)):
                ora = CR.oracle_of(si)
                ora.set_masked(CR.masks()[si])
                try:
                    flats.append(ora.exec_rich(progs[qi])[1])
                finally:
                    ora.set_masked(NONE)
            assert np.array_equal(rich_flat(cdocs, terms, cpresent, cfreq, cpos), np.concatenate(flats)), text
        # guard words around every output of one call
        n, nt = int(counts[1]), 3
        npos = C.c_size_t()
        assert L.tri_cbatch_matched_terms(cb.h, 1, None, None, None, 0, C.byref(npos)) == 0
        gp, gf, gs = guarded(n, np.uint32), guarded(n * nt, np.uint16), guarded(npos.value, np.uint16)
        assert L.tri_cbatch_matched_terms(cb.h, 1, inner(gp), inner(gf), inner(gs), npos.value, C.byref(npos)) == 0
        assert intact(gp) and intact(gf) and intact(gs)
        _, present, freq, pos = concat_rows(parts, 1)
        assert np.array_equal(gp[GUARD:-GUARD], present) and np.array_equal(gf[GUARD:-GUARD].reshape(n, nt), freq) and np.array_equal(gs[GUARD:-GUARD], pos)
        # a too-small cap is refused, as the batch call refuses it
        assert L.tri_cbatch_matched_terms(cb.h, 1, inner(gp), inner(gf), inner(gs), npos.value - 1, C.byref(npos)) == -1 and b"positions need" in L.tri_last_error()
        # the wrong mode
        plen = C.c_size_t(5)
        assert L.tri_cbatch_matched_payloads(cb.h, 0, None, None, 0, C.byref(plen)) == -1 and b"TRI_FLAG_HIT_PAYLOADS" in L.tri_last_error() and plen.value == 5


def test_payload_rows(T, dev):
    made = [DC.payload_case(), zero_position_case(T)]
    ixs = [T.Index(dev, index, terms, docs_cnt) for index, terms, docs_cnt, _, _ in made]
    oras = [O.Index.wrap(*m) for m in made]
    try:
        texts = ["t0 t1", "t0 OR t1", "t1 t0"]
        progs = [O.parse_query(t) for t in texts]
        with collection(T, ixs, progs, flags=T.FLAG_MATCHED_TERMS | T.FLAG_HIT_PAYLOADS) as (cb, parts):
            cb.run()
            cb.sync()
            counts = cb.counts()
            for qi, text in enumerate(texts):
                n = int(counts[qi])
                docs, present, freq, pos = concat_rows(parts, qi)
                lens = np.concatenate([b.matched_payloads(qi)[0] for b in parts])
                words = np.concatenate([b.matched_payloads(qi)[1] for b in parts])
                terms, cpresent, cfreq, cpos = cb.matched_terms(qi, n)
                clens, cwords = cb.matched_payloads(qi)
                assert np.array_equal(cb.docset(qi, n), docs) and np.array_equal(cpresent, present) and np.array_equal(cfreq, freq) and np.array_equal(cpos, pos), text
                assert len(clens) == len(cpos) and np.array_equal(clens, lens) and np.array_equal(cwords, words) and clens.any(), text
                assert np.array_equal(rich_flat(docs, terms, cpresent, cfreq, cpos), np.concatenate([o.exec_rich(progs[qi])[1] for o in oras])), text
            # a too-small cap
            L = T.engine.hip_lib()
            m = C.c_size_t()
            gl, gw = guarded(len(clens), np.uint8), guarded(len(clens), np.uint64)
            assert L.tri_cbatch_matched_payloads(cb.h, 2, inner(gl), inner(gw), len(clens) - 1, C.byref(m)) == -1 and b"payloads need" in L.tri_last_error()
            assert (gl.view(np.uint8) == 0xA5).all() and (gw.view(np.uint8) == 0xA5).all()
    finally:
        for ix in ixs:
            ix.close()


def test_wide_report_rows_and_column_disagreement(T, dev, sources):
    ixs = sources(1)[:2]  # (the newest source lacks one of the 17 terms: its part reports 16 columns, and the collection's row calls refuse the query — as below)
    L = T.engine.hip_lib()
    or17 = O.parse_query(SHAPES[0][1])
    # "t0 OR t1 OR t2" where the middle source knows neither t1 nor t2: both resolve to one unknown id there, and the source reports fewer columns
    per_part = [[or17, O.parse_query("t0 OR t1 OR t2")], [or17, O.parse_query(f"t0 OR t{V + 50} OR t{V + 50}")]]
    with options(dev, **OPTS), masked(ixs, CR.masks()[:2]), collection(T, ixs, per_part) as (cb, parts):
        cb.run()
        cb.sync()
        counts = cb.counts()
        n = int(counts[0])
        docs, present, freq, pos = concat_rows(parts, 0, wide=True)
        terms, cpresent, cfreq, cpos = cb.matched_terms(0, n)  # (17 terms: the binding takes the wide call)
        assert len(terms) == 17 and cpresent.dtype == np.uint64 and int(cpresent.max()) >> 16
        assert np.array_equal(cb.docset(0, n), docs) and np.array_equal(cpresent, present) and np.array_equal(cfreq, freq) and np.array_equal(cpos, pos)
        npos = C.c_size_t(12345)
        gp = guarded(n, np.uint32)
        assert L.tri_cbatch_matched_terms(cb.h, 0, inner(gp), None, None, 0, C.byref(npos)) == -1  # the narrow call on a 17-term query
        assert b"tri_batch_matched_terms_wide" in L.tri_last_error() and npos.value == 12345 and (gp.view(np.uint8) == 0xA5).all()
        # the parts disagree in the query's columns: refused, both counts named, nothing written
        nts = []
        for b in parts:
            tb, nt = np.zeros(64, np.uint32), C.c_uint32()
            assert L.tri_batch_query_terms_wide(b.h, 1, tb.ctypes.data, C.byref(nt)) == 0
            nts.append(nt.value)
        assert nts[0] == 3 and nts[1] not in (0, 3), nts
        n1 = int(counts[1])
        for fn, dt in ((L.tri_cbatch_matched_terms, np.uint32), (L.tri_cbatch_matched_terms_wide, np.uint64)):
            gp, gf, gs = guarded(n1, dt), guarded(n1 * 3, np.uint16), guarded(4 * n1 * 3, np.uint16)
            npos = C.c_size_t(12345)
            assert fn(cb.h, 1, inner(gp), inner(gf), inner(gs), 4 * n1 * 3, C.byref(npos)) == -1
            msg = L.tri_last_error().decode()
            assert f"{nts[1]} terms" in msg and "3 in" in msg, msg
            assert npos.value == 12345 and all((g.view(np.uint8) == 0xA5).all() for g in (gp, gf, gs))
        # (read part by part, the query still answers)
        assert sum(len(b.docset(1)) for b in parts) == n1 == len(cb.docset(1, n1))


# ------------------------------------------------------------------------------------------ 6
def test_lifecycle_and_refusals(T, sources):
    ixs = sources(1)
    texts = ["t0 t1", "t0 OR t1 OR t2", "t10 t11"]
    progs = [O.parse_query(t) for t in texts]
    with collection(T, ixs, progs) as (cb, parts), collection(T, ixs, progs) as (never, never_parts):
        base = [b.info()["launches"] for b in never_parts]
        set_rankers(parts[:2], progs, 10)
        with pytest.raises(T.TrinityError, match="tri_cbatch_sync"):
            cb.ranked()  # not run yet
        cb.run()
        with pytest.raises(T.TrinityError, match="tri_cbatch_sync"):
            cb.ranked()  # run, not synced
        cb.sync()
        with pytest.raises(T.TrinityError, match="no ranker on part 2"):
            cb.ranked()
        parts[2].set_ranker(10, CAP + 1, ADJ, R.token_weights(progs, w3))
        cb.run()
        cb.sync()
        with pytest.raises(T.TrinityError, match="part 2's ranker differs from part 0's in freq_cap"):
            cb.ranked()
        # a refusal writes nothing
        L = T.engine.hip_lib()
        g = guarded(3 * 10, np.float64)
        assert L.tri_cbatch_ranked(cb.h, inner(g), inner(g), inner(g)) == -1 and (g.view(np.uint8) == 0xA5).all()
        assert L.tri_cbatch_ranked(cb.h, None, inner(g), inner(g)) == -1 and b"null argument" in L.tri_last_error()
        # the same ranker on every part: the same CollectionBatch runs again, and the list stands
        set_rankers(parts, progs, 10)
        assert [b.info()["launches"] for b in parts] == [n + 2 for n in base]  # k_rich_rank + k_rank_merge a part, as for a lone batch
        cb.run()
        cb.sync()
        d, s, c = cb.ranked()
        assert d.shape == (3, 10)
        unmasked = [CR.want(p, 256, CAP, ADJ, w3, masked=False) for p in progs]
        for qi, text in enumerate(texts):
            check_row(d, s, c, qi, unmasked[qi][:10], 10, text + " (no masks)")
        # another K re-sizes the blocks
        set_rankers(parts, progs, 256)
        cb.run()
        cb.sync()
        d, s, c = cb.ranked()
        assert d.shape == (3, 256)
        for qi, text in enumerate(texts):
            check_row(d, s, c, qi, unmasked[qi], 256, text + " (no masks, K 256)")
        # the masks swapped in between two runs: fewer matches, and the rows past the count are zero again
        with masked(ixs):
            cb.run()
            cb.sync()
            d, s, c = cb.ranked()
            shorter = 0
            for qi, text in enumerate(texts):
                want = CR.want(progs[qi], 256, CAP, ADJ, w3)
                shorter += len(want) < len(unmasked[qi])
                check_row(d, s, c, qi, want, 256, text + " (masks on)")
            assert shorter
            # the parts' own lists still stand next to the merged one
            for si, b in enumerate(parts):
                pd, ps, pc = b.ranked()
                for qi, text in enumerate(texts):
                    check_row(pd, ps, pc, qi, CR.source_rows(progs[qi], CAP, ADJ, w3)[si], 256, f"{text} (part {si})")
        # a collection that was never ranked launches what it launched
        never.run()
        never.sync()
        assert [b.info()["launches"] for b in never_parts] == base
        with pytest.raises(T.TrinityError, match="no ranker on part 0"):
            never.ranked()


def test_unranked_collections_answer_as_before(T, sources):
    """An unranked default-mode collection and a scored one: counts, docsets and the scored top-K against the oracle, the parts' launches those of lone batches."""
    ixs = sources(1)
    texts = ["t0 t1", "t0 OR t1 OR t2", "t5", "[t0, t1, t2]"]
    progs = [O.parse_query(t, some_min=2) for t in texts]
    with masked(ixs):
        lone = [T.Batch(ix, progs, T.FLAG_MATCHED_TERMS) for ix in ixs]
        slone = [T.Batch(ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=10) for ix in ixs]
        try:
            with collection(T, ixs, progs) as (cb, parts), collection(T, ixs, progs, flags=T.FLAG_ACCUMULATED_SCORE, topk=10) as (sb, sparts):
                for x in (cb, sb):
                    x.run()
                    x.sync()
                assert [b.info()["launches"] for b in parts] == [b.info()["launches"] for b in lone]
                assert [b.info()["launches"] for b in sparts] == [b.info()["launches"] for b in slone]
                counts, scounts = cb.counts(), sb.counts()
                d, s, c = sb.topk_results()
                for qi, (text, prog) in enumerate(zip(texts, progs)):
                    docs, scores = [], []
                    for si in range(len(ixs)):
                        ora = CR.oracle_of(si)
                        ora.set_masked(CR.masks()[si])
                        try:
                            do, so = ora.exec(prog, O.FLAG_ACCUM_SCORE)
                        finally:
                            ora.set_masked(NONE)
                        docs.append(do), scores.append(so)
                    want = np.concatenate(docs)
                    assert int(counts[qi]) == len(want) == int(scounts[qi]), text
                    assert np.array_equal(cb.docset(qi, len(want)), want), text
                    td, ts = CR.oracle_of(0).topk(want, np.concatenate(scores), 10)
                    assert int(c[qi]) == len(td) and d[qi, : len(td)].tolist() == td.tolist(), text
                    np.testing.assert_allclose(s[qi, : len(td)], ts, rtol=1e-5, atol=0)
                for x in (cb, sb):
                    with pytest.raises(T.TrinityError, match="no ranker on part 0"):
                        x.ranked()
        finally:
            for b in lone + slone:
                b.close()
