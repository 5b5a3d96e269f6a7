"""The cases of the hit decode (tri_decode_hits / tri_decode_hits_at; a helper module, imported by tests/test_decode_hits_cases.py and
tests/test_gpu_decode_hits.py).

corpus() writes explicit postings WITH explicit positions through structured.build, which encodes them with both host encoders.  What the
device must hand back is the input `positions` array of every list, document after document — independent of either codec and of the
oracle.  payload_case() is a GOOGLE segment with payloads (engine.host_encode_google(..., payload_lens, payloads)); its expected words come
from the oracle's PLI walk, which the CPU suite pins to the reference fixture.

Why each list is there (k_decode_hits.hpp: a wave takes 64 directory blocks, a workgroup 256; a lane per document where a block's hits can be
addressed, a walking lane per block where not; a document above DH_SPLIT hits is shared by the wave):
  n<k>      k documents of frequency 1 — GOOGLE block ends (31 .. 33, 64, 65), the LUCENE 128-document block and its varbyte tail
            (127 .. 129, 261), and 32 * 256 + 5: past a workgroup's chunk of 256 blocks
  h<k>      k hits in all — the ends of LUCENE's 128-hit groups, with and without a varbyte tail
  ones      every hit at position 1 in frequency-1 documents: all-equal ints() groups in hits.data
  at100     a document of 200 hits that begins at the term's hit ordinal 100 (it straddles a hit group; above DH_SPLIT: shared by the wave)
  at90      ... of 100 hits at ordinal 90 (it straddles too; below DH_SPLIT: one lane crosses the group's end)
  mid300    a document of 300 hits between frequency-1 neighbours inside one GOOGLE block
  d<k>      96 documents of two hits; document 40 (in the middle block) has a position delta of k: 63 is the last one-byte hit varbyte, 64 and
            8191 take two bytes, 8192 three — BLK_HITS_PLAIN goes off for that block only
  last      a last position of 16383
  zeros     frequencies 0, 1, 2, 0, 3 in turn: documents that own no hits
  empty     no documents
"""
import numpy as np

import oracle_lib as O
import structured as S

DH_SPLIT = 128  # csrc/k_decode_hits.hpp (test_decode_hits_cases.py checks the mirror)
BLK_HITS_PLAIN = 0x80000000
DOC_COUNTS = [1, 31, 32, 33, 64, 65, 127, 128, 129, 261, 32 * 256 + 5]
HIT_TOTALS = [1, 127, 128, 129, 255, 256, 257, 384]
DELTAS = [63, 64, 8191, 8192]


def _docs(n, start=3, step=3):
    return start + step * np.arange(n, dtype=np.int64)


def _positions(freqs, seed):
    """Ascending positions >= 1 per document, deltas 1 .. 5 (single-byte hits)."""
    rng = np.random.default_rng(seed)
    out = []
    for f in freqs:
        out.append(np.cumsum(rng.integers(1, 6, size=int(f))))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def lists():
    L, P = {}, {}
    for i, n in enumerate(DOC_COUNTS):
        L[f"n{n}"] = (_docs(n, 1 + i, 2), np.ones(n, dtype=np.int64))
        P[f"n{n}"] = 1 + (np.arange(n) * 7 + i) % 60
    for i, h in enumerate(HIT_TOTALS):  # documents of three hits, the last one of what is left
        f = np.array([3] * (h // 3) + ([h % 3] if h % 3 else []), dtype=np.int64)
        L[f"h{h}"] = (_docs(f.size, 2 + i, 5), f)
        P[f"h{h}"] = _positions(f, 100 + i)
    L["ones"] = (_docs(300, 7, 1), np.ones(300, dtype=np.int64))
    P["ones"] = np.ones(300, dtype=np.int64)
    for name, before, big in (("at100", 100, 200), ("at90", 90, 100)):
        f = np.array([1] * before + [big] + [1] * 40, dtype=np.int64)
        L[name] = (_docs(f.size, 4, 2), f)
        P[name] = _positions(f, before)
    f = np.array([1] * 10 + [300] + [1] * 10, dtype=np.int64)
    L["mid300"] = (_docs(f.size, 9, 4), f)
    P["mid300"] = _positions(f, 300)
    for k in DELTAS:
        f = np.full(96, 2, dtype=np.int64)
        p = np.tile(np.array([1, 2], dtype=np.int64), 96)
        p[2 * 40 + 1] = 1 + k
        L[f"d{k}"] = (_docs(96, 5, 3), f)
        P[f"d{k}"] = p
    L["last"] = (_docs(3, 11, 9), np.array([1, 2, 1], dtype=np.int64))
    P["last"] = np.array([5, 1, 16383, 2], dtype=np.int64)
    f = np.array([0, 1, 2, 0, 3] * 20, dtype=np.int64)
    L["zeros"] = (_docs(f.size, 2, 2), f)
    P["zeros"] = _positions(f, 7)
    L["empty"] = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    P["empty"] = np.zeros(0, dtype=np.int64)
    return L, P


def corpus():
    L, P = lists()
    return S.build({k: (np.asarray(d, dtype=np.uint32), f) for k, (d, f) in L.items()}, positions={k: np.asarray(p, dtype=np.uint16) for k, p in P.items()}, docs_cnt=70000)


def expected(c, names):
    """(positions, offsets in hits) of the named lists one after the other."""
    pos = [c.positions[n] for n in names]
    offs = np.concatenate([[0], np.cumsum([p.size for p in pos])]).astype(np.uint64)
    return (np.concatenate(pos) if pos else np.zeros(0, dtype=np.uint16)).astype(np.uint16), offs


def doc_slices(c, name):
    """{docid: (first hit, hits)} within the list's own hit stream."""
    d, f = c.lists[name]
    ends = np.cumsum(f.astype(np.int64))
    return {int(x): (int(e - k), int(k)) for x, e, k in zip(d, ends, f)}


# ---- GOOGLE with payloads -----------------------------------------------------------------------------------------------------------------------
def payload_case():
    """-> (index bytes, term table, docs_cnt, postings, hits).  Term 0: documents whose payload length changes 0 -> 3 -> 8 -> 1 -> 0 from hit to hit, then a
    document that starts again at length 0 after one that ended on a payload (the state restarts at the document's boundary); term 1: 40 documents (a full
    block and a short one) whose every hit carries a 4-byte payload (the length stays constant over a block); term 2: plain hits next to them."""
    docs, freqs, pos, lens, words, tf = [], [], [], [], [], [0]
    cyc = [0, 3, 8, 1, 0]
    for d in range(1, 38):  # term 0
        f = 5 if d % 2 else 3
        ln = cyc[:f] if d % 2 else [8, 8, 2]
        docs.append(3 * d)
        freqs.append(f)
        pos += [2 + 3 * k for k in range(f)]
        lens += ln
        words += [(0x1122334455667788 + 0x0101010101010101 * (d + k)) & ((1 << (8 * n)) - 1) if n else 0 for k, n in enumerate(ln)]
    tf.append(len(docs))
    for d in range(1, 41):  # term 1
        docs.append(2 * d + 1)
        freqs.append(2)
        pos += [d % 50 + 1, d % 50 + 70]
        lens += [4, 4]
        words += [0xA0B0C000 + d, 0x0D0E0F00 + d]
    tf.append(len(docs))
    for d in range(1, 71):  # term 2
        docs.append(d)
        freqs.append(1 + d % 3)
        pos += list(range(1, 2 + d % 3))
        lens += [0] * (1 + d % 3)
        words += [0] * (1 + d % 3)
    tf.append(len(docs))
    from trinity_amd import engine as E

    index, terms = E.host_encode_google(np.array(docs, dtype=np.uint32), np.array(freqs, dtype=np.uint32), np.array(pos, dtype=np.uint16), np.array(tf, dtype=np.uint64),
                                        np.array(lens, dtype=np.uint8), np.array(words, dtype=np.uint64))  # fmt: skip
    return index, terms, 200, len(docs), len(pos)


def oracle_hits(ora, term):
    """(freqs, positions, payload lengths, payload words) of a whole list by the oracle's PLI walk (next() + materialize_hits on every document)."""
    it = O.PLI(ora, term)
    fr, pos, ln, pl = [], [], [], []
    while it.next() != O.DOCIDS_END:
        p, l, w = it.hits()
        fr.append(len(p))
        pos += p
        ln += l
        pl += w
    return np.array(fr, dtype=np.uint32), np.array(pos, dtype=np.uint16), np.array(ln, dtype=np.uint8), np.array(pl, dtype=np.uint64)
