"""Hit payloads in the Lucene-shaped codec, in plain Python (a helper module: tests/test_lucene_payload_cases.py holds the host encoder, the device encoder's units and the
upload walk against it on the CPU; tests/test_gpu_lucene_payloads.py compares the device with it).

The bytes (lucene_codec.cpp:163-388 writer, 401-443 and 767-856 reader).  A term's chunk in `index` is a 14-byte header {u32 hits.data offset, u32 hits, u32 bytes of its
hits.data chunk, u16 skiplist entries}, full blocks of 128 documents as ints(deltas) ints(frequencies), a varbyte (delta, frequency) tail, and one 22-byte skiplist entry per full
block.  A term's hits are ONE stream in hits.data, independent of documents and document blocks:

  full block of 128 hits : ints(position deltas) ints(payload lengths) varbyte(sum of the lengths) the payloads' bytes, in hit order
  tail (< 128 hits)      : per hit varbyte(delta << 1 | flag) [u8 length] — flag: the length differs from the tail's previous hit's, 0 before the first, whatever document the
                           hits belong to — and, behind the last hit, all payload bytes of the tail

A position-0 hit with a payload is a counted hit; one without is no hit.  The reader (materialize_hits) sets payload = 0 and copies `length` bytes for EVERY hit: a hit's
(length, word) depends on that hit alone — not the Google codec's rule, which carries the word's high bytes from hit to hit within a document (google_codec.cpp:547-583).

write() and read() restate that; only the ints() groups go through the oracle (oracle_lib: to_ints_encode / to_ints_decode, pinned by tests/test_oracle.py).  read(mutant=...)
is a deliberately WRONG reader; FAMILIES names, per mutant, a family that tells it from the right one.

Postings: [term, ...], a term = [(document, [(position, length, word), ...]), ...] with word < 2 ** (8 * length)."""
import ctypes as C

import numpy as np

import oracle_lib as O

BLOCK = 128
HEADER = 14
SKIP_BYTES = 22
SKIP_CAP = 65535
MUTANTS = ("carry_high_bytes", "tail_state_per_document", "payload_pointer_not_restarted", "payload_area_after_positions")


# ---- the two integer forms ------------------------------------------------------------------------------------------------------------------------
def varbyte(v):
    """Prefix varint (Switch/switch_compiler_aux.h:23-51)."""
    if v < 1 << 7:
        return bytes([v])
    if v < 1 << 14:
        return bytes([0x80 | v >> 8, v & 255])
    if v < 1 << 21:
        return bytes([0xC0 | v >> 16, v & 255, (v >> 8) & 255])
    if v < 1 << 28:
        return bytes([0xE0 | v >> 24, (v >> 16) & 255, (v >> 8) & 255, v & 255])
    return bytes([0xF0]) + int(v).to_bytes(4, "little")


def varbyte_get(b, at):
    """-> (value, the offset behind it)."""
    x = b[at]
    if not x & 0x80:
        return x, at + 1
    if not x & 0x40:
        return (x & 0x3F) << 8 | b[at + 1], at + 2
    if not x & 0x20:
        return (x & 0x1F) << 16 | b[at + 1] | b[at + 2] << 8, at + 3
    if not x & 0x10:
        return (x & 0x0F) << 24 | b[at + 1] << 16 | b[at + 2] << 8 | b[at + 3], at + 4
    return int.from_bytes(b[at + 1 : at + 5], "little"), at + 5


_buf = np.zeros(2048, np.uint8)


def ints(values):
    v = np.ascontiguousarray(values, dtype=np.uint32)
    assert v.size == BLOCK
    n = O.lib().to_ints_encode(v.ctypes.data, _buf.ctypes.data)
    return _buf[:n].tobytes()


def ints_get(b, at):
    """-> (128 values, the offset behind the group)."""
    src = np.zeros(1 + 4 * 255 + 8, np.uint8)
    piece = np.frombuffer(b[at : at + src.size - 8], dtype=np.uint8)
    src[: piece.size] = piece
    out = np.zeros(BLOCK, np.uint32)
    n = O.lib().to_ints_decode(src.ctypes.data, out.ctypes.data)
    return out.tolist(), at + n


# ---- the writer -----------------------------------------------------------------------------------------------------------------------------------
def write(postings):
    """-> (index bytes, hits.data bytes, term table [(documents, offset, size), ...])."""
    index, hits, table = bytearray(), bytearray(), []
    for term in postings:
        term_start, pos_start = len(index), len(hits)
        index += bytes(HEADER)
        skiplist, cur = [], None
        deltas, freqs, hpos, hlen, pay = [], [], [], [], bytearray()
        last_doc = sum_hits = ndocs = 0
        last_block_offset = last_block_total = 0
        for doc, doc_hits in term:
            assert doc > last_doc
            if len(deltas) == BLOCK:
                if len(skiplist) < SKIP_CAP:
                    skiplist.append(cur)
                index += ints(deltas) + ints(freqs)
                deltas, freqs = [], []
            if not deltas:  # what the encoder remembers at a block's first document
                cur = (len(index) - term_start, last_doc, last_block_offset, ndocs, last_block_total, len(hpos))
            deltas.append(doc - last_doc)
            freqs.append(0)
            ndocs += 1
            last_doc, last_pos = doc, 0
            for pos, length, word in doc_hits:
                if not pos and not length:
                    continue
                assert pos >= last_pos and length <= 8 and word < 1 << (8 * length)
                freqs[-1] += 1
                hpos.append(pos - last_pos)
                hlen.append(length)
                pay += int(word).to_bytes(8, "little")[:length]
                last_pos = pos
                if len(hpos) == BLOCK:
                    sum_hits += BLOCK
                    hits += ints(hpos) + ints(hlen) + varbyte(len(pay)) + pay
                    hpos, hlen, pay = [], [], bytearray()
                    last_block_total, last_block_offset = sum_hits, len(hits) - pos_start
        sum_hits += len(hpos)
        if len(deltas) == BLOCK:
            if len(skiplist) < SKIP_CAP:
                skiplist.append(cur)
            index += ints(deltas) + ints(freqs)
        else:
            for d, f in zip(deltas, freqs):
                index += varbyte(d) + varbyte(f)
        last_len = 0
        for d, length in zip(hpos, hlen):
            if length != last_len:
                last_len = length
                hits += varbyte(d << 1 | 1) + bytes([length])
            else:
                hits += varbyte(d << 1)
        hits += pay
        index[term_start : term_start + HEADER] = (
            pos_start.to_bytes(4, "little") + sum_hits.to_bytes(4, "little") + (len(hits) - pos_start).to_bytes(4, "little") + len(skiplist).to_bytes(2, "little")
        )
        for e in skiplist:
            index += b"".join(int(x).to_bytes(4, "little") for x in e[:5]) + int(e[5]).to_bytes(2, "little")
        table.append((ndocs, term_start, len(index) - term_start))
    return bytes(index), bytes(hits), table


def write_fastpfor(postings):
    """write() with FastPFor<4> words in every ints() group that is not all-equal, as the reference's own build leaves them (lucene_codec.cpp:57-64: u8 word count, the
    words).  The container is the restatement above; the words come from the product's csrc/fastpfor128.hpp (parity-unpinned, tests/test_fastpfor.py)."""
    global ints
    from trinity_amd import hostplan as HP

    L = HP._lib()
    L.tri_host_fastpfor_encode.restype = C.c_uint32
    L.tri_host_fastpfor_encode.argtypes = [C.c_void_p, C.c_void_p]
    plain = ints

    def fast(values):
        v = np.ascontiguousarray(values, dtype=np.uint32)
        if np.all(v == v[0]):
            return plain(v)
        out = np.zeros(160, dtype=np.uint32)
        n = L.tri_host_fastpfor_encode(v.ctypes.data, out.ctypes.data)
        return bytes([n]) + out[:n].tobytes()

    ints = fast
    try:
        return write(postings)
    finally:
        ints = plain


def fastpfor_postings():
    """A term of 130 documents with uneven deltas first (the upload tells a FastPFor segment by its first full document block), then the length-group shapes and the
    documents that start on every side of a quarter."""
    docs = np.cumsum(1 + np.arange(130) % 3).tolist()
    first = [(d, [(1 + k, (i + 3 * k) % 9, word_of(2 * i + k, (i + 3 * k) % 9, 20)) for k in range(2)]) for i, d in enumerate(docs)]
    return [first] + length_group_shapes() + documents_start_everywhere()


# ---- the reader -----------------------------------------------------------------------------------------------------------------------------------
def read_documents(index, entry):
    """[(document, frequency), ...] of one term, and its header (hits.data offset, hits, chunk bytes, skiplist entries)."""
    ndocs, off, size = entry
    hits_off, sum_hits, chunk, nskip = (int.from_bytes(index[off + a : off + b], "little") for a, b in ((0, 4), (4, 8), (8, 12), (12, 14)))
    at, out, doc = off + HEADER, [], 0
    left = ndocs
    while left >= BLOCK:
        d, at = ints_get(index, at)
        f, at = ints_get(index, at)
        for dd, ff in zip(d, f):
            doc += dd
            out.append((doc, ff))
        left -= BLOCK
    for _ in range(left):
        dd, at = varbyte_get(index, at)
        ff, at = varbyte_get(index, at)
        doc += dd
        out.append((doc, ff))
    assert at == off + size - SKIP_BYTES * nskip, "the chunk's blocks and tail end where its skiplist starts"
    return out, (hits_off, sum_hits, chunk, nskip)


def read_hit_stream(hits, hits_off, sum_hits, chunk, freqs=None, mutant=None):
    """The term's hits in ordinal order, [(position delta, length, word), ...] (refill_hits + the per-hit copy of materialize_hits); asserts that the walk ends with the chunk.
    freqs: the documents' frequencies — only the mutant that restarts the tail's length state with every document needs them."""
    at, out = hits_off, []
    stale = None  # (payload_pointer_not_restarted: where the previous block's payloads ended)
    for _ in range(sum_hits // BLOCK):
        deltas, after_positions = ints_get(hits, at)
        lens, at = ints_get(hits, after_positions)
        nbytes, at = varbyte_get(hits, at)
        assert nbytes == sum(lens)
        p = at
        if mutant == "payload_pointer_not_restarted" and stale is not None:
            p = stale
        if mutant == "payload_area_after_positions":
            p = after_positions
        for d, length in zip(deltas, lens):
            out.append((d, length, int.from_bytes(hits[p : p + length], "little")))
            p += length
        stale = p
        at += nbytes
    tail, length = [], 0
    starts = set()
    if mutant == "tail_state_per_document":
        h = 0
        for f in freqs:
            starts.add(h)
            h += f
    for k in range(sum_hits % BLOCK):
        if sum_hits // BLOCK * BLOCK + k in starts:
            length = 0
        v, at = varbyte_get(hits, at)
        if v & 1:
            length = hits[at]
            at += 1
        tail.append((v >> 1, length))
    for d, length in tail:
        out.append((d, length, int.from_bytes(hits[at : at + length], "little")))
        at += length
    if mutant is None:
        assert at == hits_off + chunk, "the hits walk ends where the term's chunk ends"
    return out


def read(index, hits, table, mutant=None):
    """-> postings: per term [(document, [(position, length, word), ...]), ...] — term_hit {pos, payloadLen, payload} per hit."""
    out = []
    for entry in table:
        docs, (hits_off, sum_hits, chunk, _) = read_documents(index, entry)
        assert sum(f for _, f in docs) == sum_hits
        stream = read_hit_stream(hits, hits_off, sum_hits, chunk, [f for _, f in docs], mutant)
        term, h = [], 0
        for doc, f in docs:
            pos, word, mine = 0, 0, []
            for d, length, w in stream[h : h + f]:
                pos += d
                if mutant == "carry_high_bytes":  # google_codec.cpp:563-567: the copy overwrites the low bytes of the document's previous word
                    w = (word >> (8 * length) << (8 * length) | w) if length else 0
                    word = w
                mine.append((pos, length, w))
            term.append((doc, mine))
            h += f
        out.append(term)
    return out


def skiplist(index, entry):
    """[(indexOffset, lastDocID, lastHitsBlockOffset, totalDocumentsSoFar, lastHitsBlockTotalHits, curHitsBlockHits), ...] of one term."""
    _, off, size = entry
    n = int.from_bytes(index[off + 12 : off + 14], "little")
    out = []
    for k in range(n):
        e = index[off + size - SKIP_BYTES * (n - k) : off + size - SKIP_BYTES * (n - k - 1)]
        out.append(tuple(int.from_bytes(e[4 * i : 4 * i + 4], "little") for i in range(5)) + (int.from_bytes(e[20:22], "little"),))
    return out


def agree_with_google(postings):
    """Do the two codecs' readers answer the same for these postings?  Exactly when, within every document, no non-zero length is shorter than an earlier non-zero length
    since the last zero-length hit (the Google reader then has no high bytes left over to carry)."""
    for term in postings:
        for _, doc_hits in term:
            longest = 0
            for _, length, _ in doc_hits:
                if length == 0:
                    longest = 0
                elif length < longest:
                    return False
                longest = max(longest, length)
    return True


# ---- arrays for the encoders' entry points ----------------------------------------------------------------------------------------------------------
def arrays(postings):
    """-> (docs u32, freqs u32, positions u16, payload_lens u8, payloads u64, term_first u64): what the host and device encoders take.  Position-0 hits without a payload
    are left out here (the encoders' entry points refuse them; the writer above drops them, as the reference's does)."""
    docs, freqs, pos, plen, pval, tf = [], [], [], [], [], [0]
    for term in postings:
        for doc, doc_hits in term:
            kept = [h for h in doc_hits if h[0] or h[1]]
            docs.append(doc)
            freqs.append(len(kept))
            pos += [h[0] for h in kept]
            plen += [h[1] for h in kept]
            pval += [h[2] for h in kept]
        tf.append(len(docs))
    return (np.array(docs, np.uint32), np.array(freqs, np.uint32), np.array(pos, np.uint16), np.array(plen, np.uint8), np.array(pval, np.uint64), np.array(tf, np.uint64))


# ---- the families -----------------------------------------------------------------------------------------------------------------------------------
def word_of(h, length, salt=0):
    """A payload of `length` bytes for hit h: no byte zero, every hit's different (a reader that looks in the wrong place reads something else)."""
    x = (h + 1) * 0x9E3779B97F4A7C15 + (salt + 1) * 0xC2B2AE3D27D4EB4F
    b = bytes(1 + ((x >> (8 * i)) + 37 * i) % 255 for i in range(8))
    return int.from_bytes(b[:length], "little")


def term_of(freqs, lens, first_doc=1, step=2, salt=0, positions=None):
    """A term whose document i holds freqs[i] hits at positions 1, 2, ... (or positions[h]); hit h of the term carries lens[h] bytes."""
    assert sum(freqs) == len(lens)
    term, h = [], 0
    for i, f in enumerate(freqs):
        mine = []
        for k in range(f):
            mine.append((positions[h] if positions is not None else k + 1, lens[h], word_of(h, lens[h], salt)))
            h += 1
        term.append((first_doc + step * i, mine))
    return term


def _threes(n):
    return [3] * (n // 3) + ([n % 3] if n % 3 else [])


def _mixed(n, salt=0):
    return [(5 * h + salt) % 9 for h in range(n)]


def hits_at_block_edges():
    """Terms of 127, 128, 129, 255, 256 and 257 hits, lengths 0 .. 8 mixed (width 4): the last full block, the first tail hit, an empty tail."""
    return [term_of(_threes(n), _mixed(n, n), salt=n) for n in (127, 128, 129, 255, 256, 257)]


def document_straddles_a_block():
    """A document whose hits lie on both sides of hit 128: its payloads are read from two blocks' areas (and a third document from the tail's)."""
    return [term_of([120, 20, 5], _mixed(145, 1), salt=1), term_of([100, 200, 3], [8] * 303, salt=2)]


def documents_start_everywhere():
    """Documents that begin at hit ordinals 31, 32, 33, 95, 96, 97, 127 and 128: every side of a quarter's and a block's first hit."""
    freqs = [31, 1, 1, 62, 1, 1, 30, 1, 40]
    starts = np.concatenate([[0], np.cumsum(freqs)[:-1]]).tolist()
    assert starts == [0, 31, 32, 33, 95, 96, 97, 127, 128]
    return [term_of(freqs, _mixed(sum(freqs), 3), salt=3), term_of(freqs, [1 + h % 8 for h in range(sum(freqs))], salt=4)]


def length_group_shapes():
    """One term of four full blocks and a tail: lengths all 8 (the all-equal form, 1024 payload bytes: the two-byte varint), all 0 (today's three bytes, inside a term that
    carries payloads), mostly 0 with five 8s (width 0 plus exceptions, 40 payload bytes: the one-byte varint), mixed 0 .. 8 (width 4)."""
    sparse = [8 if h in (0, 31, 32, 100, 127) else 0 for h in range(128)]
    lens = [8] * 128 + [0] * 128 + sparse + _mixed(128, 2) + [3, 3, 0]
    return [term_of(_threes(len(lens)), lens, salt=5)]


def payload_pointer_restarts_per_block():
    """Three full blocks of equal lengths: a reader that goes on where the previous block's payloads ended reads the next block's position group as payloads."""
    return [term_of([1] * 384, [2] * 384, salt=6, positions=[7] * 384)]


def payload_area_follows_the_lengths():
    """One full block: the payloads start behind ints(lengths) and the byte count, not behind the position group."""
    return [term_of([128], [4] * 128, salt=7)]


def tail_state_runs_across_documents():
    """Two documents in the tail with the same non-zero length — the second document's first hit carries no flag —, a tail that opens with length 0 and then changes, a
    tail that opens with length 5."""
    return [term_of([2, 2], [3, 3, 3, 3], salt=8), term_of([2, 1, 2], [0, 0, 6, 6, 0], salt=9), term_of([1, 3], [5, 5, 2, 5], salt=10),
            term_of([128, 2, 2], [1] * 128 + [7, 7, 7, 7], salt=11)]  # fmt: skip


def position_zero_with_payload():
    """A position-0 hit with a payload is a counted hit (and the document's next hit's delta is its position); one without is none."""
    w = lambda h, n: word_of(h, n, 12)
    return [[(3, [(0, 2, w(0, 2)), (4, 0, 0), (9, 1, w(2, 1))]), (5, [(0, 8, w(3, 8))]), (9, [(0, 0, 0), (1, 0, 0)]), (11, [(0, 1, w(4, 1)), (0, 1, w(5, 1))])]]


def every_byte_has_its_top_bit():
    """Words with the top bit of every byte set, at each length 1 .. 8 — in a full block and in a tail: a reader that sign-extends, or that masks a byte, shows."""
    lens = [1 + h % 8 for h in range(136)]
    term, h = [], 0
    for i, f in enumerate(_threes(136)):
        mine = []
        for k in range(f):
            mine.append((k + 1, lens[h], int.from_bytes(bytes(0x80 | (h + 3 * j) % 128 for j in range(lens[h])), "little")))
            h += 1
        term.append((1 + i, mine))
    return [term]


def shorter_after_longer():
    """Within a document a shorter non-zero payload follows a longer one: the Lucene reader zero-extends it, the Google reader keeps the longer one's high bytes."""
    return [term_of([3, 2], [8, 3, 1, 4, 2], salt=13), term_of([130], [8 - h % 8 for h in range(130)], salt=14)]


def payloadless_term_between():
    """A term without payloads between two that carry some: its bytes are today's, and it gets no directory row."""
    return [term_of(_threes(200), _mixed(200, 4), salt=15), term_of(_threes(200), [0] * 200, salt=16), term_of(_threes(140), [8] * 140, salt=17)]


def skiplist_past_payload_blocks():
    """A term of 129 document blocks (two hits a document, lengths mixed): every skiplist entry's lastHitsBlockOffset counts the payload bytes of the hit blocks before it."""
    n = 129 * 128 + 5
    return [term_of([2] * n, _mixed(2 * n, 5), salt=18, step=1)]


FAMILIES = {
    "hits_at_block_edges": hits_at_block_edges,
    "document_straddles_a_block": document_straddles_a_block,
    "documents_start_everywhere": documents_start_everywhere,
    "length_group_shapes": length_group_shapes,
    "payload_pointer_restarts_per_block": payload_pointer_restarts_per_block,
    "payload_area_follows_the_lengths": payload_area_follows_the_lengths,
    "tail_state_runs_across_documents": tail_state_runs_across_documents,
    "position_zero_with_payload": position_zero_with_payload,
    "every_byte_has_its_top_bit": every_byte_has_its_top_bit,
    "shorter_after_longer": shorter_after_longer,
    "payloadless_term_between": payloadless_term_between,
    "skiplist_past_payload_blocks": skiplist_past_payload_blocks,
}
# the family that tells each wrong reader from the right one
CATCHES = {
    "carry_high_bytes": "shorter_after_longer",
    "tail_state_per_document": "tail_state_runs_across_documents",
    "payload_pointer_not_restarted": "payload_pointer_restarts_per_block",
    "payload_area_after_positions": "payload_area_follows_the_lengths",
}


def expected(postings):
    """What a reader must answer for `postings`: the same, less the position-0 hits without a payload."""
    return [[(doc, [h for h in doc_hits if h[0] or h[1]]) for doc, doc_hits in term] for term in postings]


# ---- damaged segments the upload must refuse (each a copy of a family's bytes with one thing wrong) ---------------------------------------------------
def _one_block_and_tail(lens_tail=(2, 2)):
    postings = [term_of([128, len(lens_tail)], [1 + h % 4 for h in range(128)] + list(lens_tail), salt=19)]
    return postings, write(postings)


def refusals():
    """{name: (index, hits, table, a word of the message the upload walk must give)}."""
    out = {}
    postings, (index, hits, table) = _one_block_and_tail()
    hits_off = 0
    _, after_positions = ints_get(hits, hits_off)
    lens, after_lens = ints_get(hits, after_positions)
    nbytes, pay = varbyte_get(hits, after_lens)
    # a length of 9 inside a full block (the byte count is kept right, so that only the length is wrong)
    bad = [9 if i == 5 else v for i, v in enumerate(lens)]
    grown = hits[:after_positions] + ints(bad) + varbyte(sum(bad)) + hits[pay : pay + nbytes] + bytes(sum(bad) - nbytes) + hits[pay + nbytes :]
    out["length_9_in_a_block"] = (_rechunk(index, table, len(grown)), grown, table, "at most 8")
    # a block whose byte count disagrees with its lengths
    wrong = hits[:after_lens] + varbyte(nbytes + 1) + hits[pay:] + b"\0"
    out["payload_bytes_disagree"] = (_rechunk(index, table, len(wrong)), wrong, table, "add up")
    # a tail whose payload bytes overrun the chunk: the chunk is one byte short
    out["tail_payload_overruns"] = (_rechunk(index, table, len(hits) - 1), hits[:-1], table, "overrun")
    # stray bytes behind the tail
    out["stray_bytes_behind_the_tail"] = (_rechunk(index, table, len(hits) + 2), hits + b"\x01\x02", table, "stray")
    # a length of 9 in the tail
    tail_at = pay + nbytes
    assert hits[tail_at + 1] == 2  # (the first tail hit: varbyte(1 << 1 | 1), then its length byte)
    nine = hits[: tail_at + 1] + b"\x09" + hits[tail_at + 2 :] + bytes(14)
    out["length_9_in_the_tail"] = (_rechunk(index, table, len(nine)), nine, table, "at most 8")
    return out


def _rechunk(index, table, chunk):
    """The one-term index with its header's positionsChunkSize set to `chunk`."""
    assert len(table) == 1 and table[0][1] == 0
    return index[:8] + int(chunk).to_bytes(4, "little") + index[12:]
