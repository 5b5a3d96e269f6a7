"""GPU tests of the PFOR128 decoders at CHOSEN group shapes (run with -m gpu on an MI355X): LValStream (codec_streams.hpp), PfRegs<8> and PfRegs<4> (k_fused.hpp)
over the lists of tests/pfor_cases.py — every deltas width 2 .. 20 (1 with exceptions), every freqs width 0 .. 16, exception counts of 1, 8, 9, 16, 17 and 32 in a
quarter, both sides of the `cnt > 16 || cnt * eb > 64` rule on either side of a block, the hits.data widths 1 .. 14 — and lists that string all of them block after
block.  tests/test_pfor_cases.py shows on the CPU, from the encoded bytes, that every list has the header words it is there for, and from the host planner that the
unions with the dense partner are k_psets scatter unions.

Which decoder a kernel uses: k_decode, k_match (k_and, k_and_dense's dense_pass), k_probe, k_score, k_rich, k_phrase and k_decode_hits read through LValStream;
row_decode (PfRegs<8> / PfRegs<4>, the joint fallback) is called from k_fused, the k_planes kernels (plane rows included) and k_psets' scatter only.

The yardstick is the input: decode_terms and decode_hits against the postings and positions arrays, docID sets against structured.Corpus.evaluate (numpy over the
arrays), scores and the default mode's records against the oracle over the GOOGLE bytes of the same postings (structured.check_topk: rtol 1e-5, the tie rule).
Everything runs on the LUCENE-coded upload; the GOOGLE-coded one decodes and answers the DocumentsOnly queries once, as a cross-check of the yardstick.

The `wide` corpus (D = 2^26 + 37) is built and uploaded once for the file.  One device handle; every index is closed by its fixture; nothing retries."""
import numpy as np
import pytest

import decode_hits_cases as DC
import pfor_cases as PC
import structured as S
from test_gpu_parity import ALL_PLANES, options, rich_flat, run_rich
from test_gpu_structured import OVERRIDDEN, SWorld, check_docsets, check_scored

pytestmark = pytest.mark.gpu
WHICH = ["narrow", "wide"]
PROBE = {"plane_div": ALL_PLANES, "probe_max_blocks": 1 << 20}  # every single-lead conjunction through k_probe (test_gpu_parity.PLANE_SETS)
RICH_MAX_FREQ = 2048  # default-mode conjunctions run over the lists whose documents hold at most this many hits (the records are compared hit by hit in Python)
SCORED_SETS = range(len(S.SCORED_OPTION_SETS))


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
def worlds(T, dev):
    made = {}

    def get(which, codec=2):
        if (which, codec) not in made:
            made[which, codec] = SWorld(T, dev, PC.corpus(which), codec)
        return made[which, codec]

    yield get
    for w in made.values():
        w.ix.close()


# ------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("codec", [2, 1])
@pytest.mark.parametrize("which", WHICH)
def test_decode_terms_equals_the_postings(worlds, which, codec):
    """tri_decode_terms (k_decode: LValStream on both sides of every block) of every list == the postings that were encoded."""
    w = worlds(which, codec)
    c = w.c
    docs, freqs, offs = w.ix.decode_terms(np.arange(len(c.names), dtype=np.uint32), c.df())
    assert np.array_equal(offs, c.term_first)
    assert np.array_equal(docs, c.docs), [n for t, n in enumerate(c.names) if not np.array_equal(docs[int(offs[t]) : int(offs[t + 1])], c.lists[n][0])]
    assert np.array_equal(freqs, c.freqs), [n for t, n in enumerate(c.names) if not np.array_equal(freqs[int(offs[t]) : int(offs[t + 1])], c.lists[n][1])]


# ------------------------------------------------------------------------------------------ DocumentsOnly
@pytest.mark.parametrize("which", WHICH)
def test_docsets_match_numpy(worlds, which):
    """Sets, counts and docset hashes of pfor_cases.docs_queries under every DocumentsOnly option set of structured.py, with every conjunction through k_probe, and
    (narrow) with plane_div = 64.  LValStream: candidate tiles (k_and), forced windows (k_and_dense), k_probe.  row_decode: the plane rows k_psets and the
    candidate tiles read (the partners' under the default options, every list's under plane_div = ALL_PLANES), and k_psets' scatter — every `L OR p_dense` and
    `p_dense OR union` whose L has no plane: the shape lists under the default options, the narrow corpus' mixed lists under plane_div = 64
    (tests/test_pfor_cases.py pins both on the host planner).  The GOOGLE-coded upload answers the same queries once."""
    w = worlds(which)
    queries = PC.docs_queries(w.c, which)
    progs, want, hashes = w.want("docs", queries)
    assert sum(len(x) > 0 for x in want) == len(want)
    seen = {"dense_queries": 0, "cand_queries": 0, "pset_queries": 0, "probe_queries": 0, "bitmap_queries": 0}
    for opts in [o for o, _ in S.DOCS_OPTION_SETS] + [PROBE] + ([PC.SCATTER_OPTS] if which == "narrow" else []):
        info = check_docsets(w, queries, progs, want, hashes, opts)
        for k in seen:
            seen[k] += info[k]
        if not OVERRIDDEN and opts == {"dense_min_postings": 0, "planes": 0}:
            assert info["dense_queries"] > len(queries) // 2 and info["pset_queries"] == 0, info
        if not OVERRIDDEN and opts == PROBE:
            assert info["probe_queries"] > 0, info
        if not OVERRIDDEN and opts in ({}, PC.SCATTER_OPTS):  # at least the scatter unions run in k_psets and leave bitmaps
            nscat = len(PC.lists_of(w.c, which)) - (2 if which == "narrow" and not opts else 0)
            assert info["pset_queries"] >= nscat and info["bitmap_queries"] >= nscat, (opts, info["pset_queries"], info["bitmap_queries"], nscat)
    if not OVERRIDDEN:
        assert all(v > 0 for v in seen.values()), seen
    check_docsets(worlds(which, 1), queries, progs, want, hashes, {})


# ------------------------------------------------------------------------------------------ scored
@pytest.mark.parametrize("oset", SCORED_SETS)
@pytest.mark.parametrize("which", WHICH)
def test_scored_topk_under_every_kernel_variant(worlds, which, oset):
    """BM25 top-K at K = 10 and 256 of the SAME queries (pfor_cases.docs_queries; a shape list has 261 documents: K = 256 ranks nearly all of them, so a wrong
    frequency anywhere in a block moves a score) under one scored option set of structured.py a case: the planner's choice, k_planes (planes_split 1 and 7 among
    them), k_fused with 16- and 32-bit window words — PfRegs<8> and PfRegs<4> side by side in row_decode, the joint fallback — and match-then-score (fused: 0:
    k_score's FreqStream)."""
    w = worlds(which)
    opts, kinds = S.SCORED_OPTION_SETS[oset]
    queries = PC.docs_queries(w.c, which)
    progs, want, _ = w.want("docs", queries)
    counts_want = [len(x) for x in want]
    for k in (10, 256):
        check_scored(w, "docs", queries, progs, counts_want, k, opts)
    if not OVERRIDDEN and opts:
        with options(w.dev, **opts):
            b = w.T.Batch(w.ix, progs, w.T.FLAG_ACCUMULATED_SCORE, topk=10)
        try:
            b.run()
            b.sync()
            info = b.info()
        finally:
            b.close()
        assert info["planes_queries"] > 0 or "n_planes" not in kinds, (opts, info)
        assert info["fused_queries"] > 0 or not ("n_fused" in kinds or "n_fused16" in kinds), (opts, info)


@pytest.mark.parametrize("oset", SCORED_SETS)
@pytest.mark.parametrize("which", WHICH)
def test_full_score_streams(worlds, which, oset):
    """topk = 0: the score of EVERY match (what consider(id, score) receives) of the same queries, under the same option sets."""
    w = worlds(which)
    opts, _ = S.SCORED_OPTION_SETS[oset]
    queries = PC.docs_queries(w.c, which)
    progs, want, _ = w.want("docs", queries)
    ref = w.scores(("docs", 0, False), progs)
    with options(w.dev, **opts):
        b = w.T.Batch(w.ix, progs, w.T.FLAG_ACCUMULATED_SCORE, topk=0)
    try:
        b.run()
        b.sync()
        counts = b.counts()
        for i, (text, _) in enumerate(queries):
            docs, scores = ref[i]
            assert int(counts[i]) == len(docs) == len(want[i]), (opts, text)
            assert np.array_equal(b.docset(i, len(docs)), want[i]), (opts, text)
            np.testing.assert_allclose(b.scores(i, len(docs)), scores, rtol=S.RTOL, atol=0, err_msg=str((opts, text)))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ the default mode
def rich_lists(c, which):
    return [n for n in PC.lists_of(c, which) if int(c.lists[n][1].max()) <= RICH_MAX_FREQ]


@pytest.mark.parametrize("which", WHICH)
def test_default_mode_terms_and_frequencies(worlds, which):
    """Conjunctions of a catalogue list with the sparse partner (every third document of the list): the matched terms, frequencies and positions of every match
    equal the oracle's records, and the frequencies equal the INPUT frequencies of those documents — the 0-frequency documents of the width-0 lists among them.
    Left out (RICH_MAX_FREQ: the records are compared hit by hit): f_w12 .. f_w16, f_x_4x16 and mixed_f — k_rich never sees a freqs group wider than 11 bits, an
    exception of 16 bits, or freqs shapes that differ from lane to lane; it reads freqs through LValStream, which k_decode and k_score run over those lists."""
    w = worlds(which)
    c = w.c
    names = rich_lists(c, which)
    queries = [(c.q(f"{{{n}}} {{p_sparse}}"), 1) for n in names]
    progs, want, _ = w.want("rich", queries)
    zero_freq_docs = 0
    for n, (text, _), p, exp, (docs, terms, present, freq, pos) in zip(names, queries, progs, want, run_rich(w, progs)):
        wdocs, wflat, tt, ht = w.ora.exec_rich(p)
        assert np.array_equal(docs, exp) and np.array_equal(docs, wdocs) and len(docs) >= c.lists[n][0].size // 3, (text, len(docs), len(exp))
        assert int(freq.sum()) == ht and int(sum(bin(int(x)).count("1") for x in present)) == tt, text
        assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), text
        k = terms.tolist().index(c.tid[n])
        d, f = c.lists[n]
        assert np.array_equal(freq[:, k], f[np.searchsorted(d, docs)]) and all((int(x) >> k) & 1 for x in present), text
        if n.startswith("f_x_w0"):
            zero_freq_docs += int((freq[:, k] == 0).sum())
    if which == "narrow":  # (a width-0 list keeps 87 of its 261 documents in the conjunction, all but a few of them at frequency 0)
        assert {"f_x_w0_e1", "f_x_w0_e9", "f_eq0", "mixed_d", "x_both"} <= set(names) and zero_freq_docs > 150, zero_freq_docs
        assert sorted(set(PC.lists_of(c, which)) - set(names)) == sorted([f"f_w{b}" for b in range(12, 17)] + ["f_x_4x16", "mixed_f"])


# ------------------------------------------------------------------------------------------ hits.data
def test_decode_hits_equals_the_positions(worlds):
    """tri_decode_hits over every list of the narrow corpus (the hits lists' groups of widths 1 .. 14, all-equal groups, 1 / 9 / 17 exceptions in a quarter, a
    document across two groups; the frequency lists' documents of up to 65535 hits) and tri_decode_hits_at for every document of the hits lists."""
    w = worlds("narrow")
    c = w.c
    order = list(c.names)
    want_pos, want_offs = DC.expected(c, order)
    pos, _, _, offs = w.ix.decode_hits([c.tid[n] for n in order])
    assert offs.tolist() == want_offs.tolist()
    bad = np.nonzero(pos != want_pos)[0]
    assert bad.size == 0, (int(bad[0]), order[int(np.searchsorted(want_offs, bad[0], side="right")) - 1])
    for n in [x for x in PC.catalogue("narrow") if x.startswith("h_")]:
        d, f = c.lists[n]
        sl = DC.doc_slices(c, n)
        pick = d[::-1]  # (in reverse order: every pair finds its document on its own)
        freqs, p, _, _, o = w.ix.decode_hits_at([c.tid[n]] * pick.size, pick)
        assert freqs.tolist() == f[::-1].tolist(), n
        for i, x in enumerate(pick.tolist()):
            a, k = sl[x]
            assert np.array_equal(p[int(o[i]) : int(o[i + 1])], c.positions[n][a : a + k]), (n, x)
    assert w.ix.decode_hits_at([c.tid["h_w5"]] * 2, [1, 2])[0].tolist() == [0xFFFFFFFF] * 2  # documents the list does not hold


def phrase_queries(c):
    hs = [n for n in PC.catalogue("narrow") if n.startswith("h_")]
    out = [f'"{{{n}}} {{n_{n}}}"' for n in hs] + [f'"{{n_{n}}} {{{n}}}"' for n in hs[::4]] + [f'"{{{n}}} {{n_{n}}}" {{p_sparse}}' for n in hs[::3]]
    return [(c.q(t), 1) for t in out]


def test_phrases_over_the_hits_lists(worlds):
    """ "h n_h": the partner's one hit sits right behind the document's first hit of h on even ranks and two behind on odd ones — DocumentsOnly against numpy
    under the planner's choice and the forced windows, then the default mode: positions of both terms equal the oracle's records and the input positions."""
    w = worlds("narrow")
    c = w.c
    queries = phrase_queries(c)
    progs, want, hashes = w.want("phrase", queries)
    nh = len([n for n in PC.catalogue("narrow") if n.startswith("h_")])
    assert nh >= 19 and all(60 <= len(x) < c.lists["h_w2"][0].size for x in want[:nh]), [len(x) for x in want[:nh]]  # about half of a list's documents start the phrase
    for opts in ({}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}):
        info = check_docsets(w, queries, progs, want, hashes, opts)
        if not OVERRIDDEN:
            assert info["phrase_queries"] > 0
    hs = [n for n in PC.catalogue("narrow") if n.startswith("h_")]
    rq = queries[: len(hs)] + [(c.q(f"{{{n}}} {{n_{n}}}"), 1) for n in hs]
    rprogs, rwant, _ = w.want("phrase_rich", rq)
    for i, ((text, _), p, exp, (docs, terms, present, freq, pos)) in enumerate(zip(rq, rprogs, rwant, run_rich(w, rprogs))):
        wdocs, wflat, tt, ht = w.ora.exec_rich(p)
        assert np.array_equal(docs, exp) and np.array_equal(docs, wdocs), (text, len(docs), len(exp))
        assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), text
        if i >= len(hs):  # the conjunction holds every document of h: its reported positions are the input positions, list order
            n = hs[i - len(hs)]
            assert docs.size == c.lists[n][0].size, text
            k = terms.tolist().index(c.tid[n])
            at, got = 0, []
            for r in range(docs.size):
                for j in range(len(terms)):
                    if j == k:
                        got.append(pos[at : at + int(freq[r, j])])
                    at += int(freq[r, j])
            assert np.array_equal(np.concatenate(got), c.positions[n]), text
