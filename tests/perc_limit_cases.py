"""The percolator at the edges its first suite never reached (a helper module: tests/test_perc_limit_cases.py checks on the CPU that the cases say what they claim,
tests/test_gpu_perc_limits.py runs them on the device): documents of more than 64 postings (the second pass of k_perc_docs / k_perc_rows: the carry into pos_first,
dsum), calls that are a window into larger arrays (doc_first[0] != 0), phrases at MAX_PHRASE_TERMS words and at the top of u16, and the compaction / scan shapes of a
full-width batch (PERC_SEG edges with more than one tile, a second round of k_perc_scan_tops).  The yardstick is perc_cases.match_batch throughout; nothing here is
expected from the engine.

A document is {term: positions} as in perc_cases, or — where it holds terms unknown to the dictionary, which a dict cannot name twice — a list of POSTINGS
(term, positions), the unknown ones (NONE) last."""
import functools

import numpy as np

import perc_cases as PC
import trinity_amd as T

NONE = PC.NONE
PASS = 64  # csrc/k_perc.hpp: postings of a document a wave of k_perc_docs / k_perc_rows takes per pass
SEG = 1024  # PERC_SEG: hit queries per segment of the document-major fill
SCAN_BLOCK, SCAN_WG = 2048, 256  # PERC_SCAN_BLOCK elements a workgroup, PERC_WG blocks a round of k_perc_scan_tops
DENSE = 1 << 24  # ndocs * nq above which the expected pairs come from pairs_of_sparse (perc_cases.pairs_of goes through a dense nq x ndocs byte matrix)
READ_MUTANTS = ("lost_carry", "dsum_known_only", "window_from_zero")  # deliberately WRONG readers of a call's positions (read_docs), in perc_cases.MUTANTS' style


def pairs_of_sparse(bits, ndocs):
    """perc_cases.pairs_of without the dense matrix: per query only its own bitset is unpacked."""
    nbytes = (ndocs + 7) // 8
    qs, ds = [], []
    for q, b in enumerate(bits):
        if b:
            d = np.flatnonzero(np.unpackbits(np.frombuffer(b.to_bytes(nbytes, "little"), dtype=np.uint8), bitorder="little")[:ndocs])
            ds.append(d.astype(np.uint32))
            qs.append(np.full(d.size, q, dtype=np.uint32))
    q1 = np.concatenate(qs) if qs else np.zeros(0, np.uint32)
    d1 = np.concatenate(ds) if ds else np.zeros(0, np.uint32)
    order = np.lexsort((q1, d1))  # document-major: by document, then by query
    return (q1, d1), (q1[order], d1[order]), np.bincount(d1, minlength=ndocs).astype(np.uint32)


def expected_pairs(bits, ndocs):
    return pairs_of_sparse(bits, ndocs) if ndocs * max(1, len(bits)) > DENSE else PC.pairs_of(bits, ndocs)


# ---- the device against the restatement: one call (moved here from tests/test_gpu_perc.py, which still uses them)
def cut(arrays, ndocs):
    doc_first, terms, freqs, pos = arrays
    n = int(doc_first[ndocs])
    return doc_first[: ndocs + 1], terms[:n], freqs[:n], pos[: int(freqs[:n].sum())]


def check(T, p, programs, arrays, docs=None, bits=None):
    """One call; both orders and the per-document counts equal the restatement's, the document-major keys d * nq + q ascend strictly.  Returns the result's info."""
    ndocs = len(arrays[0]) - 1
    if bits is None:
        bits = PC.match_batch(programs, docs if docs is not None else PC.docs_of(*arrays))
    (q1, d1), (q2, d2), counts = expected_pairs(bits, ndocs)
    r = p.match(*arrays)
    try:
        gq, gd = r.pairs(T.PERC_BY_QUERY)
        assert gd.size == 0 or int(gd.max()) < ndocs
        assert np.array_equal(gq, q1) and np.array_equal(gd, d1)
        gq, gd = r.pairs(T.PERC_BY_DOCUMENT)
        assert gd.size == 0 or int(gd.max()) < ndocs
        assert np.array_equal(gq, q2) and np.array_equal(gd, d2)
        assert np.all(np.diff(gd.astype(np.int64) * len(programs) + gq) > 0)
        assert np.array_equal(r.doc_counts(), counts)
        info = r.info
        assert info["pairs"] == q1.size and info["ndocs"] == ndocs and info["hit_queries"] == sum(1 for b in bits if b)
        return info
    finally:
        r.close()


# ---- documents as postings
def postings_of(doc):
    return doc if isinstance(doc, list) else [(t, doc[t]) for t in sorted(doc)]


def dict_of(doc):
    """what the restatement reads of a document: its known terms"""
    return {t: list(ps) for t, ps in postings_of(doc) if t != NONE}


def arrays_of(docs):
    """perc_cases.arrays_of over documents that may be lists of postings."""
    doc_first, terms, freqs, pos = [0], [], [], []
    for doc in docs:
        for t, ps in postings_of(doc):
            terms.append(t)
            freqs.append(len(ps))
            pos.extend(ps)
        doc_first.append(len(terms))
    return np.array(doc_first, np.uint64), np.array(terms, np.uint32), np.array(freqs, np.uint32), np.array(pos, np.uint16)


def read_docs(doc_first, terms, freqs, positions, mutant=None):
    """The documents of a CALL as tri_perc_match reads them (include/trinity_hip.h tri_perc_docs): doc_first may begin anywhere in terms / freqs, and positions runs beside
    freqs from ITS first entry — the call's positions begin after those of the postings before doc_first[0]; a posting's positions begin after those of every posting before
    it.  mutant: one of READ_MUTANTS —
      lost_carry        posting i of a document starts at the frequencies of the postings of its own pass of 64 only (k_perc_rows without `run += tot`)
      dsum_known_only   a document's length leaves out its unknown terms' positions (k_perc_docs summing freqs under `t < nterms`)
      window_from_zero  the call's positions are read from positions[0] (tri_perc_match without `skip`)"""
    p0 = int(doc_first[0])
    base = 0 if mutant == "window_from_zero" else int(np.asarray(freqs[:p0], dtype=np.int64).sum())
    out = []
    for d in range(len(doc_first) - 1):
        lo, hi = int(doc_first[d]), int(doc_first[d + 1])
        doc, length = {}, 0
        for i in range(lo, hi):
            first = lo + PASS * ((i - lo) // PASS) if mutant == "lost_carry" else lo
            at = base + sum(int(f) for f in freqs[first:i])
            f = int(freqs[i])
            if int(terms[i]) != NONE:
                doc[int(terms[i])] = [int(x) for x in positions[at : at + f]]
            if int(terms[i]) != NONE or mutant != "dsum_known_only":
                length += f
        base += length
        out.append(doc)
    return out


# ---- family_long: documents of more than 64 postings
LONG_TERMS = 400
LONG_IS = (0, 62, 63, 64, 65, 126, 127, 128, 129, 298)
UNKNOWN_KNOWN, UNKNOWN_MORE = 10, 70


def stream(n):
    """A document of the distinct terms 0 .. n-1 written as a token stream in three rounds: round r emits term t (ascending) iff r < 1 + t % 3, positions consecutive from 1
    — frequencies cycle 1, 2, 3 (a posting's position start is no multiple of its index), and term t + 1 directly follows term t in round 0."""
    doc, pos = {t: [] for t in range(n)}, 1
    for r in range(3):
        for t in range(n):
            if r < 1 + t % 3:
                doc[t].append(pos)
                pos += 1
    return doc, pos


def unknown_doc():
    """stream(10), then 70 postings of unknown terms of frequency 2 (each written once in each of two more rounds: positions [p, p + 70]): 80 postings, and 140 of its
    159 positions belong to postings past the dictionary"""
    doc, pos = stream(UNKNOWN_KNOWN)
    return postings_of(doc) + [(NONE, [pos + u, pos + UNKNOWN_MORE + u]) for u in range(UNKNOWN_MORE)]


# (n of stream(n), or 0): the empty document first and the longest last, so that a window of the LAST document alone (family_window) still has positions to misread;
# the short document directly behind the one with the unknown terms: its phrase holds only if that document's whole length was summed
LONG_N = (0, 63, 64, 65, 127, 128, 129, UNKNOWN_KNOWN, 0, 300)
LONG_UNKNOWN, LONG_SHORT = 7, 8


def family_long():
    """(programs, documents, dictionary size, names).  names[q]: ("fwd" | "swap" | "term" | "tri" | "short" | "not", the words)."""
    docs = [stream(n)[0] for n in LONG_N]
    docs[LONG_UNKNOWN] = unknown_doc()
    docs[LONG_SHORT] = {1: [5], 2: [6]}
    progs, names = [], []
    for i in LONG_IS:
        progs += [PC.phrase(i, i + 1), PC.phrase(i + 1, i), PC.tk(i + 1)]
        names += [("fwd", (i, i + 1)), ("swap", (i + 1, i)), ("term", (i + 1,))]
    progs += [PC.phrase(63, 64, 65), PC.phrase(127, 128, 129), PC.phrase(1, 2), PC.tk(299) + [T.tok(T.OP_NOT, 1)]]
    names += [("tri", (63, 64, 65)), ("tri", (127, 128, 129)), ("short", (1, 2)), ("not", (299,))]
    return progs, docs, LONG_TERMS, names


# ---- family_window: a call that is a window into larger arrays
WINDOW_KS = (1, 5, 14)  # and len(docs) - 1


def family_window():
    """(programs, documents, dictionary size, the window starts k): family_phrase's documents followed by family_long's, both families' programs; a call passes
    doc_first[k:] with terms, freqs and positions WHOLE.  Expected: match_batch over documents[k:], numbered from 0."""
    p1, d1, _ = PC.family_phrase()
    p2, d2, nterms, _ = family_long()
    docs = d1 + d2
    assert len(d1) == 14
    return p1 + p2, docs, nterms, WINDOW_KS + (len(docs) - 1,)


def window(arrays, k):
    return (arrays[0][k:],) + tuple(arrays[1:])


# ---- family_phrase_limits
LIMIT_TERMS = 32
WORDS16 = tuple(range(10, 26))  # 16 distinct words
ALT16 = (1, 2) * 8  # 1 2 1 2 ...: two leaves, sixteen lanes
FIRST_COUNTS = (64, 128, 129)  # positions of a first word of which only the last starts phrase(1, 2): one pass of k_perc_phrases exactly, two, two and one more


def both16(start, last=None):
    """the 16 distinct words and the alternation, each consecutive from `start` (word j at start + j; the 16th at `last` if given)"""
    at = [start + j for j in range(15)] + [start + 15 if last is None else last]
    doc = {w: [at[j]] for j, w in enumerate(WORDS16)}
    doc[1] = sorted(at[0::2])
    doc[2] = sorted(at[1::2])
    return doc


def merged(a, b):
    return {t: sorted(a.get(t, []) + b.get(t, [])) for t in sorted(set(a) | set(b))}


def family_phrase_limits():
    """(programs, documents, dictionary size).  Programs: the 16 distinct words, the alternation, phrase(1, 2), phrase(2, 1).  Documents, in order: consecutive from 7;
    the 16th word one late; from 0 (position 0 starts no phrase); from 0 and again from 40; ending at 65535; a run from 65521 whose 16th word would stand at 65536 — it is
    given position 0, which is where a sum kept in 16 bits would look; equal repeated positions (check_docs' comparison is non-strict); a first word of 64 / 128 / 129
    positions of which only the last starts phrase(1, 2)."""
    progs = [PC.phrase(*WORDS16), PC.phrase(*ALT16), PC.phrase(1, 2), PC.phrase(2, 1)]
    docs = [both16(7), both16(7, 23), both16(0), merged(both16(0), both16(40)), both16(65520), both16(65521, 0), {1: [5, 5, 6], 2: [6, 6, 7, 7]}]
    docs += [{1: list(range(1, c + 1)), 2: [c + 1]} for c in FIRST_COUNTS]
    return progs, docs, LIMIT_TERMS


def phrase_rows_of(programs, docs):
    """the distinct stored phrases (of two words or more) all of whose words occur in the batch: info["phrase_rows"]"""
    held = {t for doc in docs for t in dict_of(doc)}
    phrases = set()
    for prog in programs:
        for i, t in enumerate(prog):
            if int(t) >> 28 == T.OP_PHRASE and (int(t) & 0x0FFFFFFF) > 1:
                n = int(t) & 0x0FFFFFFF
                phrases.add(tuple(int(x) & 0x0FFFFFFF for x in prog[i - n : i]))
    return sum(1 for ph in phrases if all(w in held for w in ph))


# ---- grid: compaction and scan shapes
GRID = ((2049, 1023), (2049, 1024), (2049, 1025), (2049, 2048), (2049, 2049), (65536, 8193), (65535, 8193))
GRID_PHRASE_DOCS = (0, 31, 32, 2047, 2048)  # and ndocs - 1


def grid_phrase_docs(ndocs):
    return tuple(sorted(set(GRID_PHRASE_DOCS + (ndocs - 1,))))  # (at 2049 documents the last one IS 2048)


@functools.lru_cache(maxsize=None)
def grid(ndocs, nhit):
    """(programs, documents, dictionary size, arrays, bits) — made once per parameter; treat as read-only.  Q = nhit + 100 term programs, program q = TERM(q); three are
    NOT(1) TERM(q) instead — the first, the one in the middle of the hit list (q = nhit / 2), the last: dense rows that cross every segment and word.  Two phrase programs
    over two more terms a = Q, b = Q + 1, phrase(a, b) and phrase(b, a), stand before the last negation, so that the LAST hit is a dense row too.  Document j holds
    {j % H, (7 j + 3) % H} at position 1; the documents 0, 31, 32, 2047, 2048 and ndocs - 1 carry a and b adjacent besides, alternately as `a b` and as `b a`.  With
    ndocs >= H every term below H is held, so the programs that hit are: q < H (the two negations among them hold on the documents without their term), both phrases, the
    last negation — H = nhit - 3 makes them exactly nhit."""
    Q, H = nhit + 100, nhit - 3
    assert 2 < H <= ndocs and ndocs > 2048
    a, b = Q, Q + 1
    progs = [PC.tk(q) for q in range(Q)]
    for q in (0, nhit // 2, Q - 1):
        progs[q] = PC.tk(q) + [T.tok(T.OP_NOT, 1)]
    progs = progs[:-1] + [PC.phrase(a, b), PC.phrase(b, a)] + progs[-1:]
    docs = [{j % H: [1], (7 * j + 3) % H: [1]} for j in range(ndocs)]
    for k, j in enumerate(grid_phrase_docs(ndocs)):
        docs[j][a], docs[j][b] = ([2], [3]) if k % 2 == 0 else ([3], [2])
    return progs, docs, Q + 2, PC.arrays_of(docs), PC.match_batch(progs, docs)
