"""tri_decode_hits / tri_decode_hits_at on the device (csrc/k_decode_hits.hpp): the hits of whole postings lists and of chosen (term, document) pairs, in both
codecs.  Expected values: the input positions of tests/decode_hits_cases.py (independent of either codec), the oracle's PLI walk (payloads; the synthetic corpus),
and the genuine reference's own `hits` hashes over the segment it wrote (tests/golden/ref_edge.json).  Everything is an integer and compares exactly."""
import base64
import json
import os

import numpy as np
import pytest

import decode_hits_cases as DC
import oracle_lib as O
import structured as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ABSENT = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF
TRI_ERR_INVALID = -1


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
def cases(T, dev):
    c = DC.corpus()
    ixs = {codec: c.upload(T, dev, codec) for codec in (1, 2)}
    yield c, ixs
    for ix in ixs.values():
        ix.close()


# ---- 1. the structured cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [1, 2])
def test_structured_cases(T, cases, codec):
    c, ixs = cases
    ix = ixs[codec]
    names = list(c.names)
    rng = np.random.default_rng(5)
    shuffled = [names[i] for i in rng.permutation(len(names))]
    for order in (names, shuffled, ["mid300", "n33", "mid300", "empty", "at100", "mid300"]):
        terms = [c.tid[n] for n in order]
        want_pos, want_offs = DC.expected(c, order)
        pos, lens, words, offs = ix.decode_hits(terms, want_payloads=True)
        assert offs.tolist() == want_offs.tolist(), order
        bad = np.nonzero(pos != want_pos)[0]
        assert bad.size == 0, (order, int(bad[0]), [order[int(np.searchsorted(want_offs, bad[0], side="right")) - 1]])
        assert not lens.any() and not words.any()  # no payloads in these segments
        # offsets = the cumulative sums of the frequencies tri_decode_terms returns
        _, freqs, doffs = ix.decode_terms(terms, [c.lists[n][0].size for n in order])
        assert [int(freqs[int(doffs[i]) : int(doffs[i + 1])].sum()) for i in range(len(order))] == np.diff(want_offs.astype(np.int64)).tolist()
        # the sizing call; a positions-only call
        sized = np.zeros(len(terms) + 1, dtype=np.uint64)
        t = np.array(terms, dtype=np.uint32)
        assert T.engine.hip_lib().tri_decode_hits(ix.h, t.ctypes.data, t.size, None, None, None, 0, sized.ctypes.data) == 0
        assert sized.tolist() == want_offs.tolist()
        pos2, lens2, words2, offs2 = ix.decode_hits(terms)
        assert lens2 is None and words2 is None and np.array_equal(pos2, pos) and np.array_equal(offs2, offs)
    # one term at a time
    for n in names:
        pos, _, _, offs = ix.decode_hits([c.tid[n]])
        assert np.array_equal(pos, c.positions[n]) and offs.tolist() == [0, c.positions[n].size], n
    pos, _, _, offs = ix.decode_hits([])
    assert pos.size == 0 and offs.tolist() == [0]


# ---- 2. payloads ------------------------------------------------------------------------------------------------------------------------------
def test_payload_case_equals_the_oracle(T, dev):
    index, terms, docs_cnt, postings, hits = DC.payload_case()
    ora = O.Index.wrap(index, terms, docs_cnt, postings, hits)
    ix = T.Index(dev, index, terms, docs_cnt)
    try:
        want = [DC.oracle_hits(ora, t) for t in range(3)]
        for order in ([0, 1, 2], [2, 0, 0, 1]):
            pos, lens, words, offs = ix.decode_hits(order, want_payloads=True)
            assert np.diff(offs.astype(np.int64)).tolist() == [int(want[t][0].sum()) for t in order]
            assert np.array_equal(pos, np.concatenate([want[t][1] for t in order]))
            assert np.array_equal(lens, np.concatenate([want[t][2] for t in order]))
            assert np.array_equal(words, np.concatenate([want[t][3] for t in order]))
            assert np.array_equal(ix.decode_hits(order)[0], pos)
        assert want[0][2].any() and want[1][2].any()
        # pairs: every document of the payload-bearing terms (walked blocks: the hits before the document are parsed), in reverse order
        for t in (0, 1):
            docs, _ = ora.decode_term(t)
            freqs, pos, lens, words, offs = ix.decode_hits_at([t] * docs.size, docs[::-1], want_payloads=True)
            f, p, ln, w = want[t]
            ends = np.cumsum(f.astype(np.int64))
            assert freqs.tolist() == f[::-1].tolist()
            for i, j in enumerate(range(docs.size - 1, -1, -1)):
                a, b, lo, hi = int(offs[i]), int(offs[i + 1]), int(ends[j] - f[j]), int(ends[j])
                assert pos[a:b].tolist() == p[lo:hi].tolist() and lens[a:b].tolist() == ln[lo:hi].tolist() and words[a:b].tolist() == w[lo:hi].tolist(), (t, j)
    finally:
        ix.close()


# ---- 3. the segment the reference wrote ---------------------------------------------------------------------------------------------------------
def _walk_google_chunk(index, terms, t):
    """(stored frequencies, positions) of term t by a plain walk of the chunk's bytes: u16 skiplist entries; per block varbyte last-document
    delta, varbyte block length, u8 n, n - 1 document deltas, n frequencies, then per document freq x { varbyte (posDelta << 1 | newLen) [u8 len] len payload bytes };
    position and payload length restart with every document, the position is a u16."""
    off, size = int(terms[t][1]), int(terms[t][2])
    b = index
    p, end = off + 2, off + size - 8 * (int(b[off]) | (int(b[off + 1]) << 8))
    freqs, pos = [], []
    while p != end:
        _, k = S._vb(b, p)
        p += k
        blen, k = S._vb(b, p)
        p += k
        n = int(b[p])
        p += 1
        bend = p + blen
        for _ in range(n - 1):
            p += S._vb(b, p)[1]
        fr = []
        for _ in range(n):
            f, k = S._vb(b, p)
            p += k
            fr.append(f)
        for f in fr:
            at, plen = 0, 0
            for _ in range(f):
                v, k = S._vb(b, p)
                p += k
                if v & 1:
                    plen = int(b[p])
                    p += 1
                p += plen
                at = (at + (v >> 1)) & 0xFFFF
                pos.append(at)
        assert p == bend
        freqs += fr
    return np.array(freqs, dtype=np.uint32), np.array(pos, dtype=np.uint16)


def test_reference_written_edge_segment(T, dev):
    g = json.load(open(os.path.join(GOLDEN, "ref_edge.json")))
    index = np.frombuffer(base64.b64decode(g["index_b64"]), dtype=np.uint8)
    terms = np.array(g["terms"], dtype=np.uint32)
    ix = T.Index(dev, index, terms, g["docsCnt"])
    try:
        recs = [r for r in g["results"] if r["cmd"] == "hits" and r["term"] != 2]
        assert sorted(r["term"] for r in recs) == [0, 1, 3, 4, 5, 6, 7]
        with_payload = 0
        for r in recs:
            t = r["term"]
            df = int(terms[t][0])
            docs, freqs, _ = ix.decode_terms([t], [df])
            pos, lens, pl, offs = ix.decode_hits([t], want_payloads=True)
            assert int(offs[1]) == int(freqs.sum()) == len(pos)
            h, at = 1469598103934665603, 0
            for d, f in zip(docs.tolist(), freqs.tolist()):
                h = O.fnv1a_u32s([f, d], h)
                for k in range(at, at + f):
                    h = O.fnv1a_u32s([int(pos[k]), int(lens[k]), int(pl[k]) & 0xFFFFFFFF, int(pl[k]) >> 32], h)
                at += f
            assert df == r["docs"] and str(h) == r["fnv"], t
            with_payload += int(lens.any())
        assert with_payload >= 1
        # term 2 holds a document of 70 000 hits, behind which the reference's own walk loses its place (the fixture has no usable hash): all of its hits, and the
        # documents after it, against a walk of the bytes
        df = int(terms[2][0])
        docs, freqs, _ = ix.decode_terms([2], [df])
        pos, _, _, offs = ix.decode_hits([2])
        wf, wp = _walk_google_chunk(index, terms, 2)
        assert int(freqs.max()) == 70000 and docs.tolist().index(100) < df - 1  # (documents follow the long one)
        assert int(offs[1]) == int(freqs.astype(np.int64).sum()) == wp.size and np.array_equal(freqs, wf)
        assert np.array_equal(pos, wp)
        # ... and the long document, and the one behind it, as pairs
        j = docs.tolist().index(100)
        ends = np.cumsum(freqs.astype(np.int64))
        f2, p2, _, _, o2 = ix.decode_hits_at([2, 2], [int(docs[j + 1]), 100])
        assert f2.tolist() == [int(freqs[j + 1]), 70000]
        assert np.array_equal(p2[: int(o2[1])], wp[int(ends[j]) : int(ends[j + 1])]) and np.array_equal(p2[int(o2[1]) :], wp[int(ends[j]) - 70000 : int(ends[j])])
    finally:
        ix.close()


# ---- 4. the synthetic corpus ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [1, 2])
def test_synthetic_corpus_equals_the_oracle(T, dev, codec):
    D, V, slots, seed = 20000, 2000, 10, 42  # the `small` world
    seg = T.Segment(D, V, slots, seed, codec=codec)
    ora = O.Index.wrap(seg.index, seg.terms, seg.docs_cnt, seg.sum_terms_docs, seg.sum_term_hits) if codec == 1 else O.Index.generate(D, V, slots, seed, codec="lucene")
    ix = T.Index.from_segment(dev, seg)
    try:
        pick, budget = [], 8000  # documents the Python loop of the oracle's walk visits
        for t in (40, 9, 150, 600, 1999, 3, 0):
            if int(seg.terms[t, 0]) <= budget:
                pick.append(t)
                budget -= int(seg.terms[t, 0])
        assert len(pick) >= 4 and max(int(seg.terms[t, 0]) for t in pick) > 256
        want = [DC.oracle_hits(ora, t) for t in pick]
        pos, lens, words, offs = ix.decode_hits(pick, want_payloads=True)
        assert np.diff(offs.astype(np.int64)).tolist() == [int(w[0].sum()) for w in want]
        assert np.array_equal(pos, np.concatenate([w[1] for w in want]))
        assert not lens.any() and not words.any()
    finally:
        ix.close()


# ---- 5. pairs ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs(c):
    """[(list, docid)]: block ends and starts, list ends, absent documents between, below and above, docIDs 0 and UINT32_MAX, duplicates, terms mixed."""
    out = []
    for n in ("n33", "n65", "n129", "n261", "n8197", "h257", "at100", "at90", "mid300", "d64", "d8192", "last", "zeros", "ones"):
        d = c.lists[n][0].astype(np.int64)
        have = set(d.tolist())
        for k in (0, 31, 32, 63, 64, 127, 128, d.size - 1):
            if k < d.size:
                out.append((n, int(d[k])))
        for x in (int(d[0]) - 1, int(d[0]) + 1, int(d[min(31, d.size - 1)]) + 1, int(d[-1]) + 1, int(d[-1]) + 1000, 0, U32_MAX):
            if x not in have and x >= 0:
                out.append((n, x))
    for n in ("at100", "at90", "mid300"):  # the long documents and their neighbours
        d, f = c.lists[n]
        k = int(np.argmax(f))
        out += [(n, int(d[k + 1])), (n, int(d[k])), (n, int(d[k - 1])), (n, int(d[k]))]
    out += [("empty", 5), ("empty", 0), ("n1", int(c.lists["n1"][0][0])), ("n1", 1)]
    rng = np.random.default_rng(11)
    return [out[i] for i in rng.permutation(len(out))] + out[:7]


@pytest.mark.parametrize("codec", [1, 2])
def test_pairs(T, cases, codec):
    c, ixs = cases
    ix = ixs[codec]
    pairs = _pairs(c)
    assert len(set(pairs)) < len(pairs)  # duplicates
    freqs, pos, lens, words, offs = ix.decode_hits_at([c.tid[n] for n, _ in pairs], [d for _, d in pairs], want_payloads=True)
    slices = {n: DC.doc_slices(c, n) for n in c.names}
    absent = present = 0
    for i, (n, d) in enumerate(pairs):
        a, b = int(offs[i]), int(offs[i + 1])
        if d in slices[n]:
            lo, f = slices[n][d]
            assert int(freqs[i]) == f and pos[a:b].tolist() == c.positions[n][lo : lo + f].tolist(), (n, d)
            present += 1
        else:
            assert int(freqs[i]) == ABSENT and a == b, (n, d)
            absent += 1
    assert present > 60 and absent > 40 and int(offs[-1]) == pos.size
    assert not lens.any() and not words.any()
    f2, p2, l2, w2, o2 = ix.decode_hits_at([c.tid[n] for n, _ in pairs], [d for _, d in pairs])
    assert l2 is None and w2 is None and np.array_equal(f2, freqs) and np.array_equal(p2, pos) and np.array_equal(o2, offs)
    f0, p0, _, _, o0 = ix.decode_hits_at([], [])
    assert f0.size == 0 and p0.size == 0 and o0.tolist() == [0]


GUARD16, GUARD8, GUARD64, GUARD32 = 0xA5A5, 0x5A, 0x1234567812345678, 0x0BADF00D


def test_refusals_leave_the_outputs_untouched(T, dev, cases):
    c, ixs = cases
    L = T.engine.hip_lib()
    lucene_without_hits = T.Index(dev, c.l_index, c.l_terms, c.docs_cnt, codec=2)
    try:
        nterms = len(c.names)
        good = np.array([c.tid["h257"], c.tid["n33"]], dtype=np.uint32)
        docs = np.array([int(c.lists["h257"][0][0]), int(c.lists["n33"][0][0])], dtype=np.uint32)
        total = 257 + 33
        at_total = int(c.lists["h257"][1][0]) + 1

        def attempt(ix, terms, cap, lens_given=True, words_given=True):
            terms = np.ascontiguousarray(terms, dtype=np.uint32)
            for at in (False, True):
                pos, lens, words = np.full(400, GUARD16, dtype=np.uint16), np.full(400, GUARD8, dtype=np.uint8), np.full(400, GUARD64, dtype=np.uint64)
                offs, freqs = np.full(terms.size + 1, GUARD64, dtype=np.uint64), np.full(terms.size, GUARD32, dtype=np.uint32)
                lp, wp = lens.ctypes.data if lens_given else None, words.ctypes.data if words_given else None
                if at:
                    rc = L.tri_decode_hits_at(ix.h, terms.ctypes.data, docs.ctypes.data, terms.size, freqs.ctypes.data, pos.ctypes.data, lp, wp, min(cap, at_total - 1) if cap < total else cap,
                                              offs.ctypes.data)  # fmt: skip
                else:
                    rc = L.tri_decode_hits(ix.h, terms.ctypes.data, terms.size, pos.ctypes.data, lp, wp, cap, offs.ctypes.data)
                assert rc == TRI_ERR_INVALID, (at, rc)
                assert L.tri_last_error()
                assert np.all(pos == GUARD16) and np.all(lens == GUARD8) and np.all(words == GUARD64) and np.all(offs == GUARD64) and np.all(freqs == GUARD32), at

        for codec in (1, 2):
            ix = ixs[codec]
            attempt(ix, [good[0], nterms], 400)  # a term index >= the index's terms
            attempt(ix, [U32_MAX, good[1]], 400)
            attempt(ix, good, total - 1)  # cap smaller than the total
            attempt(ix, good, 0)
            attempt(ix, good, 400, lens_given=True, words_given=False)  # one of the payload pointers without the other
            attempt(ix, good, 400, lens_given=False, words_given=True)
            # ... and the same calls go through once the arguments are right
            pos, _, _, offs = ix.decode_hits(good)
            assert offs.tolist() == [0, 257, total] and np.array_equal(pos, DC.expected(c, ["h257", "n33"])[0])
        attempt(lucene_without_hits, good, 400)  # a LUCENE index uploaded without hits.data
    finally:
        lucene_without_hits.close()
