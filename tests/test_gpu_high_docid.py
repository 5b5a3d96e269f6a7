"""GPU tests on segments whose docIDs lie between 2^31 and the top of u32 (run with -m gpu on an MI355X): the read paths on tests/high_docid_cases.py's corpora — a
base of a few thousand postings moved up so that its largest docID is 0x7ffeffff (the last k_planes takes), 2^31, 2^32 - 2^18 (a plane row's extent is exactly
2^32) and 2^32 - 2 (the largest a segment holds; the rows' spare window lies past 2^32), each also with documents 1 and 2 in the head lists, so that a query's
range runs from the bottom of the docID space to its top.  Every other corpus of the suite ends at or below 2^26 + 37.

The reference for docID sets, counts, hashes and bitmap words is structured.Corpus.evaluate (numpy set algebra over the postings arrays; test_high_docid_cases.py
shows it equals the oracle); for scores and the default mode's records it is the oracle over the GOOGLE bytes (structured.check_topk: scores at rtol 1e-5, docIDs
exactly — no scored case here falls under its set-wise rule); for hits it is the positions that were encoded.  No array indexed by docID is allocated here.

What costs at these tops is memory, not postings: a bitmap over the docID space is up to 512 MiB, so plane_max_bytes holds two rows and tree_max_bytes the one
tree query's nine planes, both from high_docid_cases' formulas.  One device handle; every index, batch and filter is closed by the test that made it, and the
handle's pool_in_use_bytes is then what it was; nothing sleeps or retries."""
import contextlib
import os

import numpy as np
import pytest

import high_docid_cases as H
import oracle_lib as O
import structured as S
from test_gpu_parity import options, rich_flat, run_rich

pytestmark = pytest.mark.gpu
OVERRIDDEN = bool(os.environ.get("TRINITY_TEST_OPTIONS", "").strip())  # (a run-wide option set may force other paths: info() counters are asserted only without one)
GPU_TOPS = ["PK_LAST", "SIGN", "EXTENT_EQ", "TOP"]
SPAN = S.SPAN_BITS


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


@pytest.fixture(scope="module")
def dev(T):
    from conftest import apply_test_options

    d = apply_test_options(T.Device(0))
    yield d
    d.close()


@pytest.fixture(scope="module")
def corpora():
    base = H.base_corpus()
    made = {}

    def get(top, span=False):
        if (top, span) not in made:
            made[top, span] = base if top == "BASE" else H.shifted(base, H.TOPS[top] if isinstance(top, str) else top, span)
        return made[top, span]

    return get


def budgets(c):
    """Two plane rows; the tree query's planes (one term leaf of PL_PLANES planes, one phrase leaf, the query's own) and three to spare."""
    return {"plane_max_bytes": 2 * H.row_bytes(c.D), "tree_max_bytes": (H.PL_PLANES + 5) * H.plw_of(c.D) * 4}


@contextlib.contextmanager
def uploaded(T, dev, c, codec):
    """The corpus on the device; closed on the way out, and the pool's bytes in use are back where they were."""
    before = dev.memory()["pool_in_use_bytes"]
    ix = c.upload(T, dev, codec)
    try:
        yield ix
    finally:
        ix.close()
    assert dev.memory()["pool_in_use_bytes"] == before, (dev.memory(), before)


def set_bits(words, first=0):
    """The documents of a bitmap's set bits, ascending (no array of the bitmap's documents: the non-zero words alone are unpacked)."""
    nz = np.flatnonzero(words)
    bits = np.unpackbits(words[nz].view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    r, b = np.nonzero(bits)
    return (first + 32 * nz[r].astype(np.int64) + b).astype(np.uint32)


# ------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("top", GPU_TOPS)
def test_decode_equals_the_postings(T, dev, corpora, top, codec):
    """tri_decode_terms of every list; tri_decode_hits_at for (term, top), (term, top + 1) and (term, 0xffffffff): the hits that were encoded, or absent."""
    c = corpora(top, True)
    with uploaded(T, dev, c, codec) as ix:
        docs, freqs, offs = ix.decode_terms(np.arange(len(c.names), dtype=np.uint32), c.df())
        assert np.array_equal(offs, c.term_first) and np.array_equal(docs, c.docs) and np.array_equal(freqs, c.freqs)
        n = len(c.names)
        terms = np.tile(np.arange(n, dtype=np.uint32), 4)
        targets = np.repeat(np.array([c.D, min(c.D + 1, 0xFFFFFFFF), 0xFFFFFFFF, 1], dtype=np.uint32), n)
        f, pos, _, _, ho = ix.decode_hits_at(terms, targets)
        for i, (t, d) in enumerate(zip(terms.tolist(), targets.tolist())):
            held = c.doc_positions(t).get(d)
            if held is None:
                assert int(f[i]) == 0xFFFFFFFF and int(ho[i + 1]) == int(ho[i]), (top, codec, c.names[t], d)
            else:
                assert int(f[i]) == held.size and np.array_equal(pos[int(ho[i]) : int(ho[i + 1])], held), (top, codec, c.names[t], d)
        assert all(int(f[t]) != 0xFFFFFFFF for t in range(n)) and (f[n : 3 * n] == 0xFFFFFFFF).all()  # every list ends on `top`; nothing lies above it


# ------------------------------------------------------------------------------------------ DocumentsOnly
DOCS_SETS = [o for o, _ in S.DOCS_OPTION_SETS] + [{"dense_min_postings": 0, "scatter_bitmap_slack": H.SCATTER_SLACK}, {"plane_div": S.ALL_PLANES, "probe_max_blocks": 1 << 20}]


def check_docs_batch(T, dev, ix, c, queries, progs, want, hashes, opts, masked=None, filt=None, with_hashes=True):
    """One DocumentsOnly batch: counts, sets (one by one, all at once, in the engine's own form) and hashes against numpy; every bitmap-form result word by word.
    (with_hashes: tri_batch_docset_hashes walks a bitmap-form result one lane a query — 6.8 s for the 256 MiB bitmaps of a scatter union at 0x7ffeffff, measured.)"""
    with options(dev, **dict(budgets(c), **opts)):
        b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        if filt is not None:
            b.set_filters([filt], np.zeros(len(progs), dtype=np.uint32))
        b.run()
        b.sync()
        counts, hs, info = b.counts(), (b.docset_hashes() if with_hashes else None), b.info()
        flat, offs = b.docsets()
        mixed, moffs, forms = b.docsets_mixed()
        nbm = 0
        for i, (text, _) in enumerate(queries):
            exp = want[i] if masked is None else want[i][~np.isin(want[i], masked)]
            tag = (hex(c.D), opts, text)
            assert int(counts[i]) == len(exp), tag + (int(counts[i]), len(exp))
            assert np.array_equal(b.docset(i, len(exp)), exp), tag
            assert np.array_equal(flat[int(offs[i]) : int(offs[i + 1])], exp), tag
            assert hs is None or int(hs[i]) == (hashes[i] if masked is None else O.fnv1a_docs(exp)), tag
            bm = b.docset_bitmap(i)
            assert (bm is not None) == bool(forms[i]), tag
            part = mixed[int(moffs[i]) : int(moffs[i + 1])]
            if bm is None:
                assert np.array_equal(part, exp), tag
                continue
            nbm += 1
            first, words = bm
            assert first == 0 and words.size == H.nwin_of(c.D) * (SPAN // 32) and np.array_equal(part, words), tag
            assert np.array_equal(set_bits(words, first), exp), tag  # bit j of word i is document 32 i + j, and no other bit is set
        assert info["unsupported_queries"] == 0 and b.query_status().tolist() == [0] * len(progs)
        return info, nbm
    finally:
        b.close()


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("span", [False, True])
@pytest.mark.parametrize("top", GPU_TOPS)
def test_docsets_match_numpy(T, dev, corpora, top, span, codec):
    """The catalogue — plane pairs as AND / OR / NOT, a short lead against a plane, merges of rare lists, scatter unions, CNFs, a phrase, a phrase under an OR
    (TASK_TREE) — under structured.DOCS_OPTION_SETS (k_psets, k_and_dense with and without planes, k_and's probes and merges, both result forms), with
    scatter_bitmap_slack raised (PSET_UNIT_SCATTER below 2^31; from 2^31 on the planner runs the same unions as bitmap windows of k_and_dense) and with every
    single-lead conjunction through k_probe."""
    c = corpora(top, span)
    queries = H.docs_queries(c)
    progs = S.programs(queries)
    want = [c.evaluate(p) for p in progs]
    hashes = [O.fnv1a_docs(s) for s in want]
    seen = {"dense_queries": 0, "cand_queries": 0, "pset_queries": 0, "probe_queries": 0, "tree_queries": 0, "phrase_queries": 0}
    with uploaded(T, dev, c, codec) as ix:
        for opts in DOCS_SETS:
            # (with documents 1 and 2 the two 256 MiB bitmaps' hashes have a test of their own, below: 6.8 s of the hash kernel)
            info, nbm = check_docs_batch(T, dev, ix, c, queries, progs, want, hashes, opts, with_hashes=not (span and c.D < H.SIGN and "scatter_bitmap_slack" in opts))
            for k in seen:
                seen[k] += info[k]
            if not OVERRIDDEN:
                assert info["tree_queries"] == 1 and (info["plane_terms"] == 2 or opts.get("planes", 7) == 0), (opts, info["plane_terms"])
                if "scatter_bitmap_slack" in opts:  # the two scatter unions: bitmaps through k_psets below 2^31, ascending docIDs through k_and_dense from there on
                    assert nbm == info["bitmap_queries"] == (2 if c.D < H.SIGN else 0) and info["pset_queries"] > 0, (opts, nbm, info["bitmap_queries"])
    if not OVERRIDDEN:
        assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("codec", [1, 2])
def test_scatter_bitmaps_hash_with_the_bottom_documents(T, dev, corpora, codec):
    """The case test_docsets_match_numpy leaves to a test of its own: the two 256 MiB scatter bitmaps at 0x7ffeffff with documents 1 and 2, through
    tri_batch_docset_hashes (one lane a query over a bitmap-form result: 6.8 s) and every other delivery."""
    c = corpora("PK_LAST", True)
    queries = H.docs_queries(c, ["scatter", "scatter4", "pair_or"])
    progs = S.programs(queries)
    want = [c.evaluate(p) for p in progs]
    with uploaded(T, dev, c, codec) as ix:
        info, nbm = check_docs_batch(T, dev, ix, c, queries, progs, want, [O.fnv1a_docs(s) for s in want], {"dense_min_postings": 0, "scatter_bitmap_slack": H.SCATTER_SLACK})
        assert OVERRIDDEN or nbm == 2


# ------------------------------------------------------------------------------------------ scored top-K
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("top", GPU_TOPS)
def test_scored_topk_matches_the_oracle(T, dev, corpora, top, codec):
    """K = 10 (and 256 on one list) through k_planes (0x7ffeffff alone: planner_tasks.hpp's gate), k_fused in both widths (below 0xffffc000: planner_lower.hpp's) and
    match-then-score, structured.check_topk against the oracle; counts against numpy.  The set-wise share equals the CPU file's: none."""
    c = corpora(top, True)
    ora = c.oracle()
    queries = H.scored_queries(c)
    progs = S.programs(queries)
    ref = [ora.exec(p, O.FLAG_ACCUM_SCORE) for p in progs]
    counts_want = [len(c.evaluate(p)) for p in progs]
    seen = {"planes_queries": 0, "fused_queries": 0, "cand_queries": 0, "dense_queries": 0, "pset_queries": 0}
    setwise = cases = 0
    with uploaded(T, dev, c, codec) as ix:
        for opts in H.SCORED_SETS:
            for k, sel in ((10, range(len(progs))), (256, [H.SCORED.index(H.SCORED_K256)])):
                with options(dev, **dict(budgets(c), **opts)):
                    b = T.Batch(ix, [progs[i] for i in sel], T.FLAG_ACCUMULATED_SCORE, topk=k)
                try:
                    b.run()
                    b.sync()
                    d, s, n = b.topk_results()
                    counts, info = b.counts(), b.info()
                finally:
                    b.close()
                assert info["unsupported_queries"] == 0
                for j, i in enumerate(sel):
                    docs, scores = ref[i]
                    tag = (top, codec, opts, k, queries[i][0])
                    assert int(counts[j]) == counts_want[i] == len(docs) and int(n[j]) == min(k, len(docs)), tag
                    setwise += S.check_topk(d[j, : int(n[j])], s[j, : int(n[j])], docs, scores, k, ora, tag)
                    cases += 1
                for key in seen:
                    seen[key] += info[key]
                if not OVERRIDDEN:
                    assert (info["planes_queries"] > 0) <= (c.D < H.PK_FIRST) and (info["fused_queries"] > 0) <= (c.D < H.FUSED_MAX_DOC), (opts, info["planes_queries"], info["fused_queries"])
    assert setwise == 0 and cases == len(H.SCORED_SETS) * (len(progs) + 1)  # (tests/test_high_docid_cases.py::test_score_gap_condition: 0 of 40)
    if not OVERRIDDEN:
        assert (seen["planes_queries"] > 0) == (c.D < H.PK_FIRST) and (seen["fused_queries"] > 0) == (c.D < H.FUSED_MAX_DOC) and seen["cand_queries"] > 0, seen


@pytest.mark.parametrize("codec", [1, 2])
def test_a_truth_table_query_is_left_out_by_name_at_the_top(T, dev, corpora, codec):
    """A matchsome runs off k_fused's truth table; on a segment whose docIDs reach 0xffffc000 it is left out: status TRI_ERR_UNSUPPORTED, the message names the limit, the
    other queries of the batch run.  One window below the limit's tops (2^32 - 2^18) it matches what numpy says."""
    for top in ("EXTENT_EQ", "TOP"):
        c = corpora(top, True)
        queries = [(c.q(H.TRUTH[0]), H.TRUTH[1]), (c.q(H.CASES["pair_and"]), 1)]
        progs = S.programs(queries)
        want = [c.evaluate(p) for p in progs]
        with uploaded(T, dev, c, codec) as ix:
            with options(dev, **budgets(c)):
                b = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY, allow_unsupported=True)
            try:
                b.run()
                b.sync()
                st, counts = b.query_status().tolist(), b.counts()
                if c.D < H.FUSED_MAX_DOC:
                    assert st == [0, 0] and np.array_equal(b.docset(0, int(counts[0])), want[0]), top
                else:
                    assert st == [-3, 0] and int(counts[0]) == 0 and b.info()["unsupported_queries"] == 1, (top, st)
                assert np.array_equal(b.docset(1, int(counts[1])), want[1]), top
            finally:
                b.close()


# ------------------------------------------------------------------------------------------ the default mode
class _W:
    pass


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("top", GPU_TOPS)
def test_default_mode_matches_the_oracle(T, dev, corpora, top, codec):
    """Matched terms, frequencies and positions of conjunctions, unions and phrases whose matches include `top` (and document 1), against the oracle's records."""
    c = corpora(top, True)
    ora = c.oracle()
    progs = S.programs([(c.q(t), 1) for t in H.RICH])
    with uploaded(T, dev, c, codec) as ix:
        w = _W()
        w.T, w.ix = T, ix
        for opts in ({}, {"dense_min_postings": 0}):
            with options(dev, **dict(budgets(c), **opts)):
                res = run_rich(w, progs)
            for t, p, (docs, terms, present, freq, pos) in zip(H.RICH, progs, res):
                wdocs, wflat, tt, ht = ora.exec_rich(p)
                assert int(wdocs[-1]) == c.D and np.array_equal(docs, wdocs), (top, codec, opts, t)
                assert int(freq.sum()) == ht and np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), (top, codec, opts, t)


# ------------------------------------------------------------------------------------------ masked documents, filters
def dropped_of(f, c, keep):
    """The documents 1 .. D a filter drops, from Filter.bitmap()'s words (bit 0 and the bits past D are unspecified) — or, for an allow-list, the documents it
    KEEPS: the clear bits, read off the complement, so that neither way expands more than the few words that differ from all-clear / all-set."""
    words = f.bitmap()
    assert words.size == H.plw_of(c.D)
    docs = set_bits(np.invert(words) if keep else words)
    return docs[(docs >= 1) & (docs <= c.D)]


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("top", GPU_TOPS)
def test_masked_documents_and_filters(T, dev, corpora, top, codec):
    """tri_index_set_masked, Filter(index, docids) in both modes and Filter.from_docset from docID-form results and (below 2^31) a bitmap-form one, each holding
    `top`, `top - 1` and document 1: results equal evaluate minus the dropped documents, and Filter.bitmap()'s bits are exactly the listed documents."""
    c = corpora(top, True)
    names = ["pair_and", "pair_or", "pair_not", "rare_lead", "rare_or", "scatter", "cnf", "term_head", "phrase", "tree"]
    queries = H.docs_queries(c, names)
    progs = S.programs(queries)
    want = [c.evaluate(p) for p in progs]
    hashes = [O.fnv1a_docs(s) for s in want]
    # (no list holds top - 1 — the last document alone moved onto `top` —: a listed docID without a document; its bit is set all the same)
    drop = np.union1d(np.array([1, c.D - 1, c.D], dtype=np.uint32), c.lists["r1"][0][::3]).astype(np.uint32)
    everything = np.unique(c.docs)
    sets = ({"dense_min_postings": 0}, {})
    with uploaded(T, dev, c, codec) as ix:
        ix.set_masked(drop)
        for opts in sets:
            check_docs_batch(T, dev, ix, c, queries, progs, want, hashes, opts, masked=drop)
        ix.set_masked(np.zeros(0, dtype=np.uint32))
        for keep in (False, True):
            listed = np.union1d(np.setdiff1d(everything, drop), [c.D - 2]).astype(np.uint32) if keep else drop
            f = T.Filter(ix, listed, keep=keep)
            try:
                assert np.array_equal(dropped_of(f, c, keep), listed), (top, keep)
                for opts in sets:
                    check_docs_batch(T, dev, ix, c, queries, progs, want, hashes, opts, masked=drop, filt=f)
            finally:
                f.close()
        # from_docset: the union of the head lists, the scatter union — a bitmap below 2^31 — and a union of rare lists, as allow-lists and as drop lists
        with options(dev, **dict(budgets(c), dense_min_postings=0, scatter_bitmap_slack=H.SCATTER_SLACK)):
            src = T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY)
        try:
            src.run()
            src.sync()
            for q in (names.index("pair_or"), names.index("scatter"), names.index("rare_or")):
                if not OVERRIDDEN:
                    assert src.docset_form(q) == (1 if names[q] == "scatter" and c.D < H.SIGN else 0), names[q]
                assert int(want[q][-1]) == c.D and (int(want[q][0]) == 1) == (names[q] != "rare_or"), (top, names[q])  # (the set the filter is made of holds `top` — and document 1)
                for keep in (True, False):
                    f = T.Filter.from_docset(src, q, keep=keep)
                    try:
                        assert np.array_equal(dropped_of(f, c, keep), want[q]), (top, names[q], keep)
                        dropped = np.setdiff1d(everything, want[q]).astype(np.uint32) if keep else want[q]
                        check_docs_batch(T, dev, ix, c, queries, progs, want, hashes, {"dense_min_postings": 0}, masked=dropped, filt=f)
                    finally:
                        f.close()
        finally:
            src.close()


# ------------------------------------------------------------------------------------------ tri_isect_run's stated limit
@pytest.mark.parametrize("codec", [1, 2])
def test_isect_refuses_docids_that_reach_2_31(T, dev, corpora, codec):
    """An index whose docIDs reach 2^31: TRI_ERR_UNSUPPORTED for the whole call, the message names the limit, nothing is handed out."""
    from trinity_amd.engine import TrinityError

    c = corpora("SIGN")
    with uploaded(T, dev, c, codec) as ix:
        with pytest.raises(TrinityError, match=r"2\^31"):
            ix.intersect([([[c.tid["h0"]], [c.tid["h1"]]], 0)])


@pytest.mark.parametrize("codec", [1, 2])
def test_isect_answers_just_below_its_limit(T, dev, codec):
    """The other side of the refusal: a largest docID of 2^31 - 1, one gadget request whose run ends on the last document — results and table H equal the restatement."""
    c, groups = H.isect_gadget(H.SIGN - 1)
    lst, hist = H.isect_restate(c, groups)
    with uploaded(T, dev, c, codec) as ix:
        x = ix.intersect([(groups, 0)])
        try:
            assert x.status() == [0] and x.results(0) == lst and x.histogram(0) == sorted((m, n, f) for m, (n, f) in hist.items())
        finally:
            x.close()


# ------------------------------------------------------------------------------------------ a collection of an ordinary segment and one at the top
@pytest.mark.parametrize("codec", [1, 2])
def test_a_collection_of_a_small_and_a_top_segment(T, dev, corpora, codec):
    """tri_cbatch_docset and the counts over two parts: the unshifted base and the TOP segment (same terms, same queries)."""
    parts = [corpora("BASE"), corpora("TOP", True)]
    names = ["pair_and", "pair_or", "rare_lead", "scatter", "cnf", "phrase", "tree"]
    progs = S.programs(H.docs_queries(parts[0], names))
    before = dev.memory()["pool_in_use_bytes"]
    ixs, batches, cb = [], [], None
    try:
        for c in parts:
            ixs.append(c.upload(T, dev, codec))
            with options(dev, **dict(budgets(c), dense_min_postings=0)):
                batches.append(T.Batch(ixs[-1], progs, T.FLAG_DOCUMENTS_ONLY))
        cb = T.CollectionBatch(batches)
        cb.run()
        cb.sync()
        counts = cb.counts()
        for i, p in enumerate(progs):
            want = np.concatenate([c.evaluate(p) for c in parts])
            assert int(counts[i]) == want.size and np.array_equal(cb.docset(i, want.size), want), names[i]
    finally:
        if cb is not None:
            cb.close()
        for b in batches:
            b.close()
        for ix in ixs:
            ix.close()
    assert dev.memory()["pool_in_use_bytes"] == before


# ------------------------------------------------------------------------------------------ the write side's document 2^32 - 2, uploaded
def test_the_written_top_document_reads_back(T, dev):
    """write_cases' `top` term (documents 5 and 2^32 - 2) as tri_encode_google and tri_encode_lucene write it on the device, uploaded and read back by
    tri_decode_terms — the one case tests/test_gpu_write_structured.py keeps from the read side (its UPLOAD_MAX_DOC)."""
    import write_cases as W

    c = W.EncCase("top", [W._plain([5, W.TOP_DOC], [2, 1]), W._plain([1, 2, W.TOP_DOC - 1], [1, 3, 2])], [])
    before = dev.memory()["pool_in_use_bytes"]
    gi, gt = dev.encode_google(c.docs, c.freqs, c.pos, c.tf)
    li, lh, lt = dev.encode_lucene(c.docs, c.freqs, c.pos, c.tf)
    for args, kw in (((gi, gt, W.TOP_DOC), {}), ((li, lt, W.TOP_DOC), {"codec": 2, "hits": lh})):
        ix = T.Index(dev, *args, **kw)
        try:
            d, f, offs = ix.decode_terms(np.arange(c.nterms, dtype=np.uint32), np.diff(c.tf.astype(np.int64)))
            assert np.array_equal(offs, c.tf) and np.array_equal(d, c.docs) and np.array_equal(f, c.freqs), kw
        finally:
            ix.close()
    assert dev.memory()["pool_in_use_bytes"] == before
