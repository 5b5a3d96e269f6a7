"""CPU checks of the percolator's limit cases (tests/perc_limit_cases.py) that tests/test_gpu_perc_limits.py runs on the device: the cases say what they claim to say.
The long documents' phrases equal their closed form; a reader of the call's positions that loses the carry between a document's passes of 64 postings, one that leaves
the unknown terms' positions out of a document's length and one that reads a window's positions from index 0 are each told from the right reader by the cases named for
them; the grid's parameters hit exactly the queries they name and the full-width ones need a second round of the scan's top level; pairs_of_sparse equals
perc_cases.pairs_of wherever both can run.

What the lost carry changes (test_a_lost_carry_is_told_apart prints it): every posting at index 64 or later of every long document is read at other positions, none
before; of the 10 stored phrases that hold somewhere and have a word there, 7 change their answer.  phrase(64, 65), phrase(128, 129) and phrase(298, 299) do not: both
words lie in one pass, the misplaced reads of two neighbouring postings are neighbouring slices of the document's positions, and round 0 of the stream leaves `t + 1` and
`t + 2` at the heads of neighbouring postings — the phrase holds on the wrong positions by the same adjacency.  The phrases that straddle a pass (63 64, 127 128), the
three-word phrases and 65 66, 126 127, 129 130 cannot be right by that accident."""
import ctypes as C

import numpy as np
import pytest

import perc_cases as PC
import perc_limit_cases as L
import trinity_amd as T


def dicts(docs):
    return [L.dict_of(d) for d in docs]


def set_bits(b):
    """the documents of a bitset, ascending — through its binary digits, not through numpy (pairs_of_sparse's way)"""
    return [d for d, c in enumerate(bin(b)[:1:-1]) if c == "1"]


def test_pairs_of_sparse_equals_pairs_of():
    """on the four FAMILIES, on every small case of this file, and on a set with an empty program and no programs at all"""
    cases = [fam()[:2] for fam in PC.FAMILIES.values()]
    cases += [L.family_long()[:2], L.family_phrase_limits()[:2], ([[]] + PC.family_not()[0], PC.family_not()[1]), ([], [{1: [1]}, {}])]
    progs, docs, _, ks = L.family_window()
    cases += [(progs, docs[k:]) for k in (0,) + ks]
    cases += [L.grid(nd, nh)[:2] for nd, nh in L.GRID if nd * (nh + 102) <= L.DENSE]
    assert len(cases) == 4 + 4 + 5 + 5
    for progs, docs in cases:
        bits = PC.match_batch(progs, dicts(docs))
        a, b = PC.pairs_of(bits, len(docs)), L.pairs_of_sparse(bits, len(docs))
        for (x, y), (u, v) in zip(a[:2], b[:2]):
            assert x.dtype == u.dtype == y.dtype == v.dtype == np.uint32 and np.array_equal(x, u) and np.array_equal(y, v)
        assert b[2].dtype == np.uint32 and np.array_equal(a[2], b[2])
    assert L.expected_pairs is not PC.pairs_of and all(nd * (nh + 102) > L.DENSE for nd, nh in L.GRID[5:])  # (the full-width grids: pairs_of_sparse alone)


# ---- family_long
@pytest.fixture(scope="module")
def long_case():
    progs, docs, nterms, names = L.family_long()
    arrays = L.arrays_of(docs)
    return progs, docs, names, arrays, PC.match_batch(progs, dicts(docs))


def test_long_documents_are_what_the_family_says(long_case):
    progs, docs, names, arrays, bits = long_case
    doc_first, terms, freqs, pos = arrays
    assert [len(L.postings_of(d)) for d in docs] == [0, 63, 64, 65, 127, 128, 129, 80, 2, 300] and int(terms[terms != L.NONE].max()) < L.LONG_TERMS == 400
    for d, n in enumerate(L.LONG_N):
        if n and d != L.LONG_UNKNOWN:
            lo = int(doc_first[d])
            assert terms[lo : lo + n].tolist() == list(range(n)) and freqs[lo : lo + n].tolist() == [1 + t % 3 for t in range(n)]
            at = int(freqs[:lo].sum())
            assert sorted(pos[at : at + int(freqs[lo : lo + n].sum())].tolist()) == list(range(1, 1 + sum(1 + t % 3 for t in range(n))))  # consecutive from 1
    lo, hi = int(doc_first[L.LONG_UNKNOWN]), int(doc_first[L.LONG_UNKNOWN + 1])
    assert terms[lo:hi].tolist() == list(range(10)) + [L.NONE] * 70 and freqs[lo + 10 : hi].tolist() == [2] * 70 and int(freqs[lo + L.PASS : hi].sum()) == 32  # past the first pass
    assert L.dict_of(docs[L.LONG_SHORT]) == {1: [5], 2: [6]} and docs[0] == {} and L.LONG_SHORT == L.LONG_UNKNOWN + 1
    assert L.read_docs(*arrays) == dicts(docs) == PC.docs_of(*arrays)


def test_long_documents_closed_form(long_case):
    """phrase(i, i + 1) holds exactly on the documents of n > i + 1 terms, the swapped phrase on none; the rest by hand"""
    progs, docs, names, arrays, bits = long_case
    seen = 0
    for (kind, words), b in zip(names, bits):
        if kind == "fwd":
            assert b == sum(1 << d for d, n in enumerate(L.LONG_N) if n > words[1]) and b, words
            seen += 1
        elif kind == "swap":
            assert b == 0, words
        elif kind == "term":
            assert b == sum(1 << d for d, n in enumerate(L.LONG_N) if n > words[0]) | ((1 << L.LONG_SHORT) if words[0] in (1, 2) else 0), words
        elif kind == "tri":
            assert b == sum(1 << d for d, n in enumerate(L.LONG_N) if n > words[2]) and b, words
    assert seen == len(L.LONG_IS) == 10
    assert bits[names.index(("short", (1, 2)))] == sum(1 << d for d, n in enumerate(L.LONG_N) if n > 2) | 1 << L.LONG_SHORT
    assert bits[names.index(("not", (299,)))] == (1 << 9) - 1  # every document but the one of 300 terms
    for q in range(len(progs)):  # (and the per-pair form agrees)
        assert bits[q] == sum(1 << d for d, doc in enumerate(dicts(docs)) if PC.match_one(progs[q], doc)), names[q]


def test_a_lost_carry_is_told_apart(long_case):
    progs, docs, names, arrays, bits = long_case
    right, wrong = L.read_docs(*arrays), L.read_docs(*arrays, mutant="lost_carry")
    for d, (a, b) in enumerate(zip(right, wrong)):  # every posting from the 65th on is misread, none before (the unknown terms' positions are read by nobody)
        assert {t for t in a if a[t] != b[t]} == {t for i, (t, _) in enumerate(L.postings_of(docs[d])) if i >= L.PASS and t != L.NONE}, d
    mbits = PC.match_batch(progs, wrong)
    changed = {names[q] for q in range(len(progs)) if bits[q] != mbits[q]}
    print("lost_carry changes", sorted(changed))
    assert all(kind in ("fwd", "tri") and max(words) >= L.PASS for kind, words in changed)  # none before posting 64, no term, no negation
    late = {(kind, words) for kind, words in names if kind in ("fwd", "tri") and max(words) >= L.PASS}
    assert len(late) == 10 and late - changed == {("fwd", (64, 65)), ("fwd", (128, 129)), ("fwd", (298, 299))}  # (the module's docstring: right by the stream's own adjacency)
    assert {("fwd", (63, 64)), ("fwd", (127, 128)), ("tri", (63, 64, 65)), ("tri", (127, 128, 129))} <= changed  # a word on either side of a pass
    for d, n in enumerate(L.LONG_N):  # every document of more than 64 postings answers some stored phrase differently
        if n > L.PASS:
            assert any((bits[q] ^ mbits[q]) >> d & 1 for q in range(len(progs))), n


def test_a_length_without_the_unknown_terms_is_told_apart(long_case):
    progs, docs, names, arrays, bits = long_case
    wrong = L.read_docs(*arrays, mutant="dsum_known_only")
    assert wrong[: L.LONG_UNKNOWN + 1] == dicts(docs)[: L.LONG_UNKNOWN + 1] and wrong[L.LONG_SHORT] == {1: [20], 2: [90]}
    mbits = PC.match_batch(progs, wrong)
    q = names.index(("short", (1, 2)))
    assert bits[q] ^ mbits[q] == 1 << L.LONG_SHORT
    assert all((bits[k] ^ mbits[k]) & ((1 << L.LONG_SHORT) - 1) == 0 for k in range(len(progs)))  # no document before the short one changes


# ---- family_window
def test_windows(long_case):
    progs, docs, nterms, ks = L.family_window()
    assert ks == (1, 5, 14, len(docs) - 1) and len(docs) == 24 and len(progs) == 9 + len(long_case[0]) and nterms == 400
    arrays = L.arrays_of(docs)
    whole = dicts(docs)
    for k in ks:
        w = L.window(arrays, k)
        assert int(w[0][0]) != 0 and w[1] is arrays[1] and w[3] is arrays[3] and int(arrays[2][: int(w[0][0])].sum()) > 0  # positions to skip
        assert L.read_docs(*w) == whole[k:]
        want = PC.match_batch(progs, whole[k:])
        assert any(want)
        wrong = PC.match_batch(progs, L.read_docs(*w, mutant="window_from_zero"))
        assert any(a != b and any(int(t) >> 28 == T.OP_PHRASE for t in p) for a, b, p in zip(want, wrong, progs)), k
    assert whole[-1] and max(len(v) for v in whole[-1].values()) == 3  # the last window is one document, and not the empty one


# ---- family_phrase_limits
def test_phrase_limits():
    T.build.build_host()
    progs, docs, nterms = L.family_phrase_limits()
    assert [len(p) for p in progs] == [17, 17, 3, 3] and len(set(L.WORDS16)) == 16 and L.ALT16 == (1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2)
    bits = PC.match_batch(progs, docs)
    hold16 = 1 << 0 | 1 << 3 | 1 << 4  # from 7; from 0 and from 40; ending at 65535 — not: a late 16th word, from 0 alone, a run that needs 65536
    assert bits[0] == bits[1] == hold16
    assert docs[4][25] == [65535] and docs[4][10] == [65520] and docs[5][10] == [65521] and docs[5][25] == [0] and docs[5][2][0] == 0 and docs[2][10] == [0] and docs[1][25] == [23]
    assert docs[6] == {1: [5, 5, 6], 2: [6, 6, 7, 7]} and bits[2] >> 6 & 1 and not bits[3] >> 6 & 1
    for k, c in enumerate(L.FIRST_COUNTS):
        d = docs[7 + k]
        assert len(d[1]) == c and d[2] == [d[1][-1] + 1] and bits[2] >> (7 + k) & 1 and not bits[3] >> (7 + k) & 1
        assert not PC.phrase_holds({1: d[1][:-1], 2: d[2]}, (1, 2))  # only the last position starts it
    assert L.FIRST_COUNTS == (PC.PHRASE_PASS, 2 * PC.PHRASE_PASS, 2 * PC.PHRASE_PASS + 1) and L.phrase_rows_of(progs, docs) == 4
    assert L.phrase_rows_of(progs, docs[6:]) == 3 and L.phrase_rows_of(progs + [PC.phrase(5), PC.phrase(1, 2)], docs) == 4
    for q in range(4):
        assert bits[q] == sum(1 << d for d, doc in enumerate(docs) if PC.match_one(progs[q], doc))
    # MAX_PHRASE_TERMS (csrc/dev_structs.hpp) is still 16: a phrase of 16 words is lowered, one of 17 refused by name
    for n, rc, what in ((16, 0, b""), (17, -1, b"a phrase of 17 words (at most 16)")):
        flat, q = T.engine.flatten([PC.phrase(*range(n))])
        status, info, err = np.full(1, 99, dtype=np.int32), np.zeros(6, dtype=np.uint64), C.create_string_buffer(512)
        assert T.engine.host_lib().tri_host_perc_lower(flat.ctypes.data, flat.size, q.ctypes.data, 1, nterms, status.ctypes.data, info.ctypes.data, err, 512) == rc and what in err.value
        assert rc or (status[0] == 0 and info[2] == 1)  # lowered: one phrase leaf


# ---- grid
@pytest.mark.parametrize("ndocs,nhit", L.GRID)
def test_grid(ndocs, nhit):
    progs, docs, nterms, arrays, bits = L.grid(ndocs, nhit)
    Q = nhit + 100
    assert len(docs) == ndocs and len(progs) == Q + 2 and nterms == Q + 2 and len(arrays[0]) == ndocs + 1
    assert sum(1 for b in bits if b) == nhit
    hits = [q for q, b in enumerate(bits) if b]
    dense = [q for q, p in enumerate(progs) if len(p) == 2]
    nseg = -(-nhit // L.SEG)
    assert dense == [0, nhit // 2, Q + 1] and [hits.index(q) for q in dense] == [0, nhit // 2, nhit - 1] and nseg == (nhit - 1) // L.SEG + 1  # the first hit, the middle one, the last
    full = (1 << ndocs) - 1
    for q in dense:  # dense rows: all but the few documents that hold the term — every word, the partly filled last one too
        t = int(progs[q][0]) & 0x0FFFFFFF
        same = bits[q] == full ^ sum(1 << j for j, doc in enumerate(docs) if t in doc)  # (a name: pytest would print the integers)
        assert same and t == min(q, Q - 1) and bin(bits[q]).count("1") >= ndocs - 32 and bits[q] >> (ndocs - 1) & 1
    on = [set_bits(bits[q]) for q in (Q - 1, Q)]  # the two phrases
    js = L.grid_phrase_docs(ndocs)
    assert js == ((0, 31, 32, 2047, 2048, ndocs - 1) if ndocs > 2049 else (0, 31, 32, 2047, 2048)) and on == [list(js[0::2]), list(js[1::2])] and bits[5] == sum(1 << j for j, doc in enumerate(docs) if 5 in doc)
    W = (ndocs + 31) // 32
    assert (nseg * W * 32 > L.SCAN_WG * L.SCAN_BLOCK) == (ndocs > 2049)  # the segment table's scan: a second round of k_perc_scan_tops at full width alone
    if ndocs > 2049:
        assert W == 2048 and -(-nhit // 1024) * W * 32 > 256 * 2048
    (q1, d1), (q2, d2), counts = L.expected_pairs(bits, ndocs)
    assert q1.size == d2.size == int(counts.sum()) == sum(b.bit_count() for b in bits) and int(counts.min()) >= 1
    key = d2.astype(np.int64) * len(progs) + q2
    assert np.all(np.diff(key) > 0) and np.all(np.diff(q1.astype(np.int64) * ndocs + d1) > 0) and np.array_equal(np.sort(d1.astype(np.int64) * len(progs) + q1), key)
    for q in (0, 5, dense[1], Q - 2, Q - 1, Q, Q + 1):
        assert d1[q1 == q].tolist() == set_bits(bits[q])
