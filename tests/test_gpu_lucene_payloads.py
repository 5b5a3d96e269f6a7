"""Hit payloads of the Lucene-shaped codec on the device (run with -m gpu on an MI355X): tri_encode_lucene_payloads / tri_commit_lucene_payloads, the upload's payload
directory, tri_decode_hits / tri_decode_hits_at, the default mode's tri_batch_matched_payloads and tri_merge_lucene.  The expected bytes and hits never come from the
engine: tests/lucene_payload_cases.py restates the writer and the reader (tests/test_lucene_payload_cases.py holds the host encoder against it on the CPU).  Everything
is an integer and compares exactly."""
import ctypes as C

import numpy as np
import pytest

import lucene_payload_cases as LP
import oracle_lib as O
import write_cases as W
from merge_restated import merge_term
from test_gpu_parity import options
from trinity_amd import hostplan as HP

pytestmark = pytest.mark.gpu
NAMES = sorted(LP.FAMILIES)
ABSENT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    O.lib()
    return trinity_amd


@pytest.fixture(scope="module")
def dev(T):
    from conftest import apply_test_options

    d = apply_test_options(T.Device(0))
    yield d
    d.close()


@pytest.fixture(scope="module")
def written():
    made = {}

    def get(name):
        if name not in made:
            postings = LP.FAMILIES[name]()
            made[name] = (postings, LP.write(postings))
        return made[name]

    return get


def u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def upload(T, dev, index, hits, table):
    return T.Index(dev, u8(index), np.array(table, dtype=np.uint32).reshape(-1, 3), 1 << 20, codec=2, hits=u8(hits))


def flat_hits(term):
    """(positions, lengths, words) of a term's hits in ordinal order."""
    hs = [h for _, doc_hits in term for h in doc_hits if h[0] or h[1]]
    return (np.array([h[0] for h in hs], np.uint16), np.array([h[1] for h in hs], np.uint8), np.array([h[2] for h in hs], np.uint64))


def same_segment(got, index, hits, table, what):
    gi, gh, gt = got
    assert [tuple(r) for r in np.asarray(gt).tolist()] == [tuple(r) for r in table], what
    assert gi.tobytes() == bytes(index), (what, "index")
    assert gh.tobytes() == bytes(hits), (what, "hits.data")


# ---- 1. encode and commit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_encode_and_commit_write_the_restated_bytes(dev, written, name):
    postings, (index, hits, table) = written(name)
    d, f, p, pl, pv, tf = LP.arrays(postings)
    same_segment(dev.encode_lucene(d, f, p, tf, pl, pv), index, hits, table, name)
    # the same postings as a session: term k is termID k + 1 (commit's order for ids below 32), inserted last posting first
    tids = np.repeat(np.arange(1, tf.size, dtype=np.uint32), np.diff(tf.astype(np.int64)))
    order = np.arange(d.size)[::-1]
    hit0 = np.concatenate([[0], np.cumsum(f.astype(np.int64))])
    take = W.hit_slices(hit0, order)
    ci, ch, ctids, ct, stats = dev.commit_lucene(tids[order], d[order], f[order], p[take], pl[take], pv[take])
    assert ctids.tolist() == list(range(1, tf.size))
    same_segment((ci, ch, ct), index, hits, table, name + " (commit)")
    assert stats["sum_term_hits"] == int(p.size) and stats["sum_terms_docs"] == int(d.size)


def test_commit_on_the_reference_sessions(dev):
    """The sessions of tests/golden/ref_commit.json (documents, hits, lengths and words are in the fixture) through the Lucene-shaped encoder: the device's commit
    against the restated commit walk followed by the host encoder."""
    seen = 0
    for rec, s in W.golden_commit_sessions():
        tids, (d, f, p, tf, pl, pv), _ = W.commit_reference(s, True)
        wi, wh, wt = HP.lucene_encode(d, f, p, tf, payload_lens=pl, payloads=pv)
        ci, ch, ctids, ct, _ = dev.commit_lucene(s.tids, s.docs, s.freqs, s.pos, s.plen, s.pval)
        assert np.array_equal(ctids, tids), rec["seed"]
        same_segment((ci, ch, ct), wi.tobytes(), wh.tobytes(), wt.tolist(), rec["seed"])
        seen += int(pl.any())
    assert seen


# ---- 2. round trip --------------------------------------------------------------------------------------------------------------------------------
def check_round_trip(T, dev, postings, index, hits, table, what):
    ix = upload(T, dev, index, hits, table)
    try:
        want = [flat_hits(term) for term in LP.expected(postings)]
        nt = len(table)
        for order in (list(range(nt)), list(range(nt))[::-1] + [0]):
            pos, lens, words, offs = ix.decode_hits(order, want_payloads=True)
            assert np.diff(offs.astype(np.int64)).tolist() == [want[t][0].size for t in order], what
            assert np.array_equal(pos, np.concatenate([want[t][0] for t in order])), what
            bad = np.flatnonzero(lens != np.concatenate([want[t][1] for t in order]))
            assert bad.size == 0, (what, "lengths", int(bad[0]))
            bad = np.flatnonzero(words != np.concatenate([want[t][2] for t in order]))
            assert bad.size == 0, (what, "words", int(bad[0]))
            assert np.array_equal(ix.decode_hits(order)[0], pos)  # (positions only: nothing new runs)
        # pairs: every document of every term, shuffled, some twice, and documents the lists do not hold
        pairs = [(t, doc) for t, term in enumerate(postings) for doc, _ in term]
        rng = np.random.default_rng(3)
        pairs = [pairs[i] for i in rng.permutation(len(pairs))[:600]]
        pairs += pairs[:9] + [(t, 0) for t in range(nt)] + [(t, postings[t][-1][0] + 1) for t in range(nt)]
        by_doc = [{doc: [h for h in doc_hits if h[0] or h[1]] for doc, doc_hits in term} for term in postings]
        freqs, pos, lens, words, offs = ix.decode_hits_at([t for t, _ in pairs], [doc for _, doc in pairs], want_payloads=True)
        for i, (t, doc) in enumerate(pairs):
            a, b = int(offs[i]), int(offs[i + 1])
            if doc not in by_doc[t]:
                assert int(freqs[i]) == ABSENT and a == b, (what, t, doc)
                continue
            hs = by_doc[t][doc]
            assert int(freqs[i]) == len(hs) == b - a, (what, t, doc)
            assert list(zip(pos[a:b].tolist(), lens[a:b].tolist(), words[a:b].tolist())) == hs, (what, t, doc)
    finally:
        ix.close()


@pytest.mark.parametrize("name", NAMES)
def test_round_trip(T, dev, written, name):
    postings, (index, hits, table) = written(name)
    check_round_trip(T, dev, postings, index, hits, table, name)


def test_round_trip_through_the_fastpfor_container(T, dev):
    postings = LP.fastpfor_postings()
    index, hits, table = LP.write_fastpfor(postings)
    assert hits != LP.write(postings)[1]
    check_round_trip(T, dev, postings, index, hits, table, "fastpfor")


# ---- sessions for the cross-codec, default-mode and merge tests ---------------------------------------------------------------------------------------
NTERMS, NDOCS = 24, 400


def session(agree, salt, payloads=True, docs=range(1, NDOCS + 1), nterms=NTERMS):
    """postings of nterms terms (term k = termID k + 1) over `docs`: about a quarter of the documents each, 1 .. 3 hits a document.  agree: a document's non-zero
    lengths never fall (the two codecs' readers then answer the same); else they fall on purpose."""
    out = []
    for k in range(nterms):
        term, h = [], 0
        for doc in docs:
            if (doc * 7 + k * 13 + salt) % 4:
                continue
            n = 1 + (doc + k) % 3
            lens = sorted((3 * doc + 5 * j + k + salt) % 9 for j in range(n))
            if not agree:
                lens = lens[::-1]
            mine = []
            for j in range(n):
                length = lens[j] if payloads else 0
                mine.append((2 + 3 * j + (doc + k) % 2, length, LP.word_of(h, length, salt + k)))
                h += 1
            term.append((doc, mine))
        out.append(term)
    return out


def session_arrays(postings):
    """the session in insertion order: document after document, a document's terms ascending"""
    rows = sorted((doc, k, doc_hits) for k, term in enumerate(postings) for doc, doc_hits in term)
    flat = [h for _, _, hs in rows for h in hs]
    return (np.array([k + 1 for _, k, _ in rows], np.uint32), np.array([doc for doc, _, _ in rows], np.uint32), np.array([len(hs) for _, _, hs in rows], np.uint32),
            np.array([h[0] for h in flat], np.uint16), np.array([h[1] for h in flat], np.uint8), np.array([h[2] for h in flat], np.uint64))  # fmt: skip


def commit_both(T, dev, postings):
    tids, docs, freqs, pos, pl, pv = session_arrays(postings)
    gi, gtids, gt, _ = dev.commit_google(tids, docs, freqs, pos, pl, pv)
    li, lh, ltids, lt, _ = dev.commit_lucene(tids, docs, freqs, pos, pl, pv)
    assert gtids.tolist() == ltids.tolist() == list(range(1, len(postings) + 1))
    return T.Index(dev, gi, gt, NDOCS), T.Index(dev, li, lt, NDOCS, codec=2, hits=lh)


def or_of(terms):
    return np.array(list(terms) + [O.tok(O.OP_OR, len(terms))], dtype=np.uint32)


def matched(b, q):
    n = int(b.counts()[q])
    docs = b.docset(q, n)
    terms, present, freq, pos = b.matched_terms_wide(q, n)
    lens, words = b.matched_payloads(q)
    return docs, terms, present, freq, pos, lens, words


def want_matched(postings, docs, terms, present, freq):
    """(positions, lengths, words) the default mode must deliver: match after match, the query's terms in the engine's order, a present term's hits."""
    by_doc = [{doc: doc_hits for doc, doc_hits in term} for term in postings]
    out = []
    for i, doc in enumerate(docs.tolist()):
        for k, t in enumerate(terms.tolist()):
            holds = doc in by_doc[t]
            assert bool((int(present[i]) >> k) & 1) == holds and int(freq[i, k]) == (len(by_doc[t][doc]) if holds else 0), (doc, t)
            if holds:
                out += by_doc[t][doc]
    return [h[0] for h in out], [h[1] for h in out], [h[2] for h in out]


QUERIES = [or_of([0, 5, 9]), np.array([2], np.uint32), or_of(range(20))]  # narrow, one term, a wide-report query (20 reportable terms)
WIDE = {"rich_max_terms": 64, "tree_max_nodes": 1024}


def run_default(T, dev, ix):
    with options(dev, **WIDE):
        b = T.Batch(ix, QUERIES, T.FLAG_MATCHED_TERMS | T.FLAG_HIT_PAYLOADS)
    try:
        b.run()
        b.sync()
        return [matched(b, q) for q in range(len(QUERIES))]
    finally:
        b.close()


# ---- 3. cross-codec -------------------------------------------------------------------------------------------------------------------------------
def test_the_codecs_agree_where_the_rule_says_so(T, dev):
    postings = session(True, 1)
    assert LP.agree_with_google(postings) and any(h[1] for term in postings for _, hs in term for h in hs)
    gix, lix = commit_both(T, dev, postings)
    try:
        order = list(range(NTERMS))
        g, l = gix.decode_hits(order, want_payloads=True), lix.decode_hits(order, want_payloads=True)
        for a, b in zip(g, l):
            assert np.array_equal(a, b)
        want = [flat_hits(term) for term in postings]
        assert np.array_equal(l[1], np.concatenate([w[1] for w in want])) and np.array_equal(l[2], np.concatenate([w[2] for w in want]))
        for rg, rl in zip(run_default(T, dev, gix), run_default(T, dev, lix)):
            for a, b in zip(rg, rl):
                assert np.array_equal(a, b)
            assert rl[5].any()
    finally:
        gix.close()
        lix.close()


def test_the_codecs_differ_where_the_rule_is_broken(T, dev):
    postings = session(False, 2)
    assert not LP.agree_with_google(postings)
    gix, lix = commit_both(T, dev, postings)
    try:
        order = list(range(NTERMS))
        g, l = gix.decode_hits(order, want_payloads=True), lix.decode_hits(order, want_payloads=True)
        want = [flat_hits(term) for term in postings]
        assert np.array_equal(l[0], g[0]) and np.array_equal(l[1], g[1])
        assert np.array_equal(l[1], np.concatenate([w[1] for w in want])) and np.array_equal(l[2], np.concatenate([w[2] for w in want]))
        assert np.count_nonzero(l[2] != g[2]) >= 1
    finally:
        gix.close()
        lix.close()


# ---- 4. default mode ------------------------------------------------------------------------------------------------------------------------------
def test_default_mode_reports_the_restated_payloads(T, dev):
    postings = session(False, 3)
    index, hits, table = LP.write(postings)
    ix = upload(T, dev, index, hits, table)
    try:
        for q, (docs, terms, present, freq, pos, lens, words) in enumerate(run_default(T, dev, ix)):
            wpos, wlens, wwords = want_matched(postings, docs, terms, present, freq)
            assert len(docs) and pos.tolist() == wpos, q
            assert lens.tolist() == wlens and words.tolist() == wwords, q
        assert len(QUERIES[2]) == 21
    finally:
        ix.close()


def test_default_mode_over_a_collection(T, dev):
    """A tri_cbatch of two Lucene segments, the second with payloads: the rows of the parts, source after source."""
    older, newer = session(True, 4, payloads=False, docs=range(1, 200)), session(False, 5, docs=range(200, NDOCS + 1))
    ixs = [upload(T, dev, *LP.write(p)) for p in (older, newer)]
    parts, cb = [], None
    try:
        with options(dev, **WIDE):
            parts = [T.Batch(ix, QUERIES, T.FLAG_MATCHED_TERMS | T.FLAG_HIT_PAYLOADS) for ix in ixs]
        cb = T.CollectionBatch(parts)
        cb.run()
        cb.sync()
        for q in range(len(QUERIES)):
            wlens, wwords = [], []
            for b, postings in zip(parts, (older, newer)):
                docs, terms, present, freq, _, _, _ = matched(b, q)
                _, ln, wd = want_matched(postings, docs, terms, present, freq)
                wlens += ln
                wwords += wd
            lens, words = cb.matched_payloads(q)
            assert lens.tolist() == wlens and words.tolist() == wwords, q
            assert any(wlens)
    finally:
        if cb is not None:
            cb.close()
        for b in parts:
            b.close()
        for ix in ixs:
            ix.close()


# ---- 5. merge -------------------------------------------------------------------------------------------------------------------------------------
def test_merge_carries_the_payloads(T, dev):
    """Three participants with payloads, most recent first, overlapping documents, masks on two of them; one output term is absent from a participant."""
    nt = 5
    parts = [session(False, 6, docs=range(150, 330), nterms=nt), session(True, 7, docs=range(60, 260), nterms=nt), session(False, 8, docs=range(1, 210), nterms=nt)]
    masks = [set(range(150, 330, 7)), None, set(range(1, 210, 5))]
    ixs = [upload(T, dev, *LP.write(p)) for p in parts]
    try:
        for ix, m in zip(ixs, masks):
            if m is not None:
                ix.set_masked(np.array(sorted(m), dtype=np.uint32))
        part_terms = np.array([[k, k, k] for k in range(nt)], dtype=np.uint32)
        part_terms[3, 1] = ABSENT
        merged = []
        for row in part_terms.tolist():
            merged.append(merge_term([None if k == ABSENT else p[k] for k, p in zip(row, parts)], masks))
        assert all(merged) and any(d in masks[0] for d, _ in parts[0][0])
        index, hits, table = LP.write(merged)
        mi, mh, mt, stats = dev.merge_lucene(ixs, part_terms)
        same_segment((mi, mh, mt), index, hits, table, "merge")
        assert stats["sum_term_hits"] == sum(len(hs) for term in merged for _, hs in term)
        check_round_trip(T, dev, merged, mi.tobytes(), mh.tobytes(), table, "merged")
    finally:
        for ix in ixs:
            ix.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LP.refusals()))
def test_upload_refuses_damaged_payloads(T, dev, name):
    index, hits, table, word = LP.refusals()[name]
    with pytest.raises(T.TrinityError, match=word):
        upload(T, dev, index, hits, table)


def test_the_abi_refuses(T, dev):
    d, f, p, pl, pv, tf = LP.arrays([[(1, [(1, 8, 5), (2, 3, 5)])]])
    with pytest.raises(T.TrinityError, match="null argument"):  # payload_lens without payloads
        dev.encode_lucene(d, f, p, tf, pl, None)
    tids = np.ones(d.size, np.uint32)
    with pytest.raises(T.TrinityError, match="null argument"):
        dev.commit_lucene(tids, d, f, p, pl, None)
    nine = pl.copy()
    nine[1] = 9
    with pytest.raises(T.TrinityError, match="at most 8"):
        dev.encode_lucene(d, f, p, tf, nine, pv)
    with pytest.raises(T.TrinityError, match="more than 8"):
        dev.commit_lucene(tids, d, f, p, nine, pv)
    zero = p.copy()
    zero[0] = 0
    with pytest.raises(T.TrinityError):  # a position-0 hit without a payload
        dev.encode_lucene(d, f, zero, tf, np.zeros_like(pl), pv)


# ---- 7. null arrays -------------------------------------------------------------------------------------------------------------------------------
def test_null_arrays_are_the_existing_calls(T, dev, written):
    L = T.engine.hip_lib()
    for name in ("hits_at_block_edges", "documents_start_everywhere"):
        postings, _ = written(name)
        bare = [[(doc, [(pos, 0, 0) for pos, _, _ in doc_hits if pos]) for doc, doc_hits in term] for term in postings]
        d, f, p, pl, pv, tf = LP.arrays(bare)
        index, hits, table = LP.write(bare)
        same_segment(dev.encode_lucene(d, f, p, tf), index, hits, table, name)
        same_segment(dev.encode_lucene(d, f, p, tf, None, None), index, hits, table, name)
        same_segment(dev.encode_lucene(d, f, p, tf, pl, pv), index, hits, table, name + " (zero lengths)")
        # the new export itself with null arrays
        io, ho = np.zeros(len(index) + 8, np.uint8), np.zeros(len(hits) + 8, np.uint8)
        terms = np.zeros((len(table), 3), np.uint32)
        il, hl = C.c_size_t(), C.c_size_t()
        rc = L.tri_encode_lucene_payloads(dev.h, d.ctypes.data, f.ctypes.data, p.ctypes.data, None, None, p.size, tf.ctypes.data, len(table), io.ctypes.data, io.size, C.byref(il),
                                          ho.ctypes.data, ho.size, C.byref(hl), terms.ctypes.data)  # fmt: skip
        assert rc == 0
        same_segment((io[: il.value], ho[: hl.value], terms), index, hits, table, name + " (null arrays)")
