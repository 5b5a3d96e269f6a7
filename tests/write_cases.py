"""Structured inputs for the WRITE side (a helper module, imported by tests/test_write_cases.py and tests/test_gpu_write_structured.py).

random_postings / lucene_postings draw i.i.d. sizes, small termIDs and documentIDs below a few million: nothing lands on the boundaries the write-side kernels have.  The
cases here are written posting by posting so that they do: every length class of every varint the GOOGLE encoder writes, every phase of the skiplist countdown against
every way a term can end around a marked block, the 65535-entry cap, the scan's chunk and round sizes for postings and for blocks, the Lucene-shaped codec's 128-document
and 128-hit cadences, termIDs whose high bits wrap in the commit key, sessions in hostile insertion orders, sessions commit must refuse, and merges whose participants,
masks and term mappings sit on k_merge_select's edges.

Every case carries `reaches`: the classes (CLASSES below) it is there for.  The *_classes functions RECOMPUTE the classes a case reaches from its arrays;
tests/test_write_cases.py holds every declaration against them and the union against CLASSES, so a case that stops reaching its boundary fails on the CPU.

The plain references: commit_reference — sorted(key = (id & 31, id)) over the terms, ascending documents within a term, the walk tests/golden/ref_commit.json pins —
and merge_reference — merge_restated.merge_term with masks, the walk ref_merge.json pins —, both followed by the host encoders."""
import json
import os

import numpy as np

import pfor_cases
from merge_restated import encoder_arrays, merge_term

ENC_SCAN_CHUNK = 32768  # (k_encode.hpp; tests/test_write_cases.py::test_constants_mirror_the_headers parses the header)
SCAN_SIZES = [0, 1, 1023, 1024, 1025, 32767, 32768, 32769, 65536, 65537]
SKIP_CAP = 65535
VEDGES = [1 << 7, 1 << 14, 1 << 21, 1 << 28]
TOP_DOC = 2**32 - 2
COMMIT_TERM_IDS = [1, 31, 32, 33, 63, 2**27 - 1, 2**27, 2**27 + 32, 2**31, 2**31 + 31, 2**32 - 1]
COMMIT_DOC_IDS = [1, 2, 2**31, TOP_DOC]
COMMIT_SIZES = [32767, 32768, 32769, 65537]
LUCENE_DOCS = [0, 1, 127, 128, 129, 255, 256, 257, 384]
LUCENE_HITS = [0, 1, 2, 127, 128, 129]
LUCENE_DELTAS = [1, 1 << 20]
MERGE_LENS = [31, 32, 33, 127, 128, 129]
MERGE_PARTS = [1, 2, 5, 17]
MERGE_PART_DOCS = {1: [31, 32, 33, 64, 65], 2: [127, 128, 129, 300]}  # by codec
ABSENT = 0xFFFFFFFF


def vlen(v):
    """Bytes of the prefix varint of v (Switch/switch_compiler_aux.h:23-51), elementwise."""
    return np.searchsorted(np.array(VEDGES, dtype=np.int64), np.asarray(v, dtype=np.int64), side="right") + 1


def ramp(f):
    """Positions 1 .. f for every document of frequencies f."""
    f = np.asarray(f, dtype=np.int64)
    ends = np.cumsum(f)
    return (np.arange(int(ends[-1]) if f.size else 0, dtype=np.int64) - np.repeat(ends - f, f) + 1).astype(np.uint16)


def hit_slices(hit0, idx):
    """The hit indices of the postings idx, one posting after the other (hit0: hits before every posting)."""
    idx = np.asarray(idx, dtype=np.int64)
    n = (hit0[idx + 1] - hit0[idx]).astype(np.int64)
    return (np.repeat(hit0[idx] - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))).astype(np.int64) if idx.size else np.zeros(0, np.int64)


def random_postings(rng, nterms):
    """Postings that reach every corner of the encoder: empty terms, 1 / 31 / 32 / 33 / 64 / 65 documents, runs long enough for skiplist
    entries, deltas of every varint length, frequencies 0 .. 300, positions up to 65535 with repeats."""
    docs, freqs, pos, tf = [], [], [], [0]
    sizes = [0, 1, 31, 32, 33, 64, 65, 300, 1000, 2, 5]
    for t in range(nterms):
        n = sizes[t % len(sizes)] if t < 3 * len(sizes) else int(rng.integers(0, 200))
        scale = [1, 3, 200, 20000, 3_000_000][t % 5]
        d = np.cumsum(rng.integers(1, scale + 1, size=n, dtype=np.int64))
        d = d[d < 2**32 - 1]
        f = np.where(rng.random(d.size) < 0.1, 0, rng.integers(1, 4, size=d.size))
        if d.size and t % 7 == 0:
            f[int(rng.integers(0, d.size))] = 300
        for k in f.tolist():
            p = np.sort(rng.integers(1, [12, 200, 65536][t % 3], size=k))
            pos += p.tolist()
        docs += d.tolist()
        freqs += f.tolist()
        tf.append(len(docs))
    return np.array(docs, dtype=np.uint32), np.array(freqs, dtype=np.uint32), np.array(pos, dtype=np.uint16), np.array(tf, dtype=np.uint64)


# ---- the classes --------------------------------------------------------------------------------------------------------------------------------
def _edge_classes(q, n):
    return [f"{q}_vlen:{k}|{k + 1}" for k in range(1, n + 1)]


GOOGLE_CLASSES = (_edge_classes("delta", 4) + _edge_classes("hdr", 4) + _edge_classes("freq", 2) + _edge_classes("hit", 2) + _edge_classes("body", 3)
                  + ["doc:2^32-2", "freq:65535", "hit_delta:65534", "hit:position0_with_payload"]
                  + [f"skip_phase:{r}/{w}" for r in range(8) for w in ("before", "on", "after")] + ["skip_cap"]
                  + [f"scan:{n}" for n in SCAN_SIZES] + [f"block_scan:{n}" for n in SCAN_SIZES])  # fmt: skip
LUCENE_CLASSES = ([f"lucene_docs:{n}" for n in LUCENE_DOCS] + [f"lucene_hits:{n}" for n in LUCENE_HITS] + [f"lucene_delta:{d}" for d in LUCENE_DELTAS]
                  + ["lucene_exception", "lucene_equal:deltas", "lucene_equal:freqs", "lucene_equal:hits", "lucene_pos:65535"] + [f"lucene_hb:{k}" for k in (0, 1, 127)])  # fmt: skip
COMMIT_CLASSES = (["commit_term:>=2^27", "commit_term:2^31", "commit_term:2^32-1", "commit_term:low5_equal", "commit_doc:2^32-2", "commit_order:sorted", "commit_order:reversed",
                   "commit_order:document_major", "commit_one_term_everywhere", "commit_one_document_all_terms", "commit_no_hits"] + [f"commit_scan:{n}" for n in COMMIT_SIZES]
                  + ["refuse:document0_before_duplicate", "refuse:duplicate_before_document0", "refuse:duplicate_first_and_last_inserted", "refuse:duplicate_last_two_sorted",
                     "refuse:duplicate_across_chunk", "refuse:positions", "refuse:payload9"])  # fmt: skip
MERGE_CLASSES = (["empty_participant_between", "unmasked_next_to_masked"] + [f"participants:{n}" for n in MERGE_PARTS]
                 + ["every_document_everywhere", "winner_masked_loser_unmasked", "everything_masked", "every_term_empty"] + [f"merged_len:{n}" for n in MERGE_LENS]
                 + ["mask_bit:31", "mask_bit:32", "mask_bit:last_document", "part_terms_not_monotone", "winner_freq0_loser_hits", "row_without_hits", "term_without_hits"])  # fmt: skip
MERGE_GOOGLE_CLASSES = [f"g:{c}" for c in MERGE_CLASSES] + ["g:payload_8_then_none"] + [f"g:part_docs:{n}" for n in MERGE_PART_DOCS[1]]
MERGE_LUCENE_CLASSES = [f"l:{c}" for c in MERGE_CLASSES] + ["l:row_inside_hit_block"] + [f"l:part_docs:{n}" for n in MERGE_PART_DOCS[2]]
CLASSES = GOOGLE_CLASSES + LUCENE_CLASSES + COMMIT_CLASSES + MERGE_GOOGLE_CLASSES + MERGE_LUCENE_CLASSES


# ---- encoder cases ------------------------------------------------------------------------------------------------------------------------------
class EncCase:
    """Postings term after term: .arrays = (docs, freqs, pos, term_first, plen, pval) (plen / pval None: no hit has a payload).  upload: the documentIDs are small enough
    for the read side's per-document bitmaps; oracle: the CPU test decodes the host encoder's bytes back through the oracle."""

    def __init__(self, name, terms, reaches, payloads=False, upload=False, oracle=True):
        self.name, self.reaches, self.upload, self.oracle = name, set(reaches), upload, oracle
        docs, freqs, pos, plen, pval, tf = [], [], [], [], [], [0]
        for term in terms:
            d, f, p = (np.asarray(x, dtype=np.int64) for x in term[:3])
            assert d.size == f.size and p.size == int(f.sum()), name
            docs.append(d)
            freqs.append(f)
            pos.append(p)
            plen.append(np.asarray(term[3], dtype=np.int64) if len(term) > 3 else np.zeros(p.size, np.int64))
            pval.append(np.asarray(term[4], dtype=np.uint64) if len(term) > 3 else np.zeros(p.size, np.uint64))
            tf.append(tf[-1] + d.size)
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        self.docs, self.freqs, self.pos, self.tf = cat(docs, np.uint32), cat(freqs, np.uint32), cat(pos, np.uint16), np.array(tf, dtype=np.uint64)
        self.plen, self.pval = (cat(plen, np.uint8), cat(pval, np.uint64)) if payloads else (None, None)

    @property
    def arrays(self):
        return self.docs, self.freqs, self.pos, self.tf, self.plen, self.pval

    @property
    def nterms(self):
        return self.tf.size - 1


def _plain(docs, freqs):
    return (np.asarray(docs, dtype=np.int64), np.asarray(freqs, dtype=np.int64), ramp(freqs))


def _words(n, salt):
    """n deterministic 64-bit payload words."""
    return (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64((salt * 0xC2B2AE3D27D4EB4F) & (2**64 - 1))


def google_varints():
    """One term per quantity.  `delta`: interior deltas 2^7k - 1 and 2^7k; `hdr`: eight full blocks whose last - previous last are those values; `top`: documentID 2^32 - 2;
    `freq`: 127 / 128 / 16383 / 16384 / 65535 hits at one repeated position (the oracle's hit buffer holds 65536: make_golden.py); `hit`: position delta << 1 | flag on 127 /
    128, 16383 / 16384, a delta of 65534, a counted position-0 hit with a payload; four one-document terms whose block bodies are 127 / 128 / 16383 / 16384 bytes; two
    32-document blocks of 8-byte-payload hits whose bodies are 2^21 - 1 and 2^21 bytes (127 + 9 hits + one byte per document whose first hit sits at position 64)."""
    terms = []
    edges = [e - s for e in VEDGES for s in (1, 0)]
    terms.append(_plain(np.cumsum(edges + [1] * 32), [1] * 40))  # (the edge deltas are documents 0 .. 7 of the first block: interior)
    hdr, last = [], 0
    for h in edges:
        hdr += [last + h - 31 + i for i in range(32)]
        last += h
    terms.append(_plain(hdr + [last + 1], [1] * (len(hdr) + 1)))
    terms.append(_plain([5, TOP_DOC], [2, 1]))
    f = [127, 128, 16383, 16384, 65535, 0, 1]
    terms.append((np.arange(1, 8), np.array(f), np.full(sum(f), 7)))
    # (document: [(position, payload length)])
    hit_docs = [[(63, 3)], [(64, 0)], [(8191, 2)], [(8192, 0)], [(65534, 0)], [(1, 0), (65535, 0)], [(65535, 1)], [(0, 1), (5, 1), (5, 0), (9, 8), (9, 8)], [(3, 8)], [(4, 0)]]
    hp = [p for d in hit_docs for p, _ in d]
    hl = [l for d in hit_docs for _, l in d]
    hv = _words(len(hp), 3)
    terms.append((np.arange(10, 10 + len(hit_docs)), np.array([len(d) for d in hit_docs]), np.array(hp), np.array(hl), hv))
    for f1 in (126, 127, 16381, 16382):
        terms.append(_plain([9], [f1]))
    for k in (6, 7):  # 127 + 9 * 233002 + k = 2^21 - 1, 2^21
        fr = np.full(32, 7281)
        fr[-1] = 233002 - 31 * 7281
        first = np.cumsum(fr) - fr
        p = np.ones(int(fr.sum()), np.int64)
        p[:] = np.repeat(np.where(np.arange(32) < k, 64, 1), fr)
        terms.append((np.arange(1, 33), fr, p, np.full(p.size, 8), _words(p.size, k)))
        assert first[-1] + fr[-1] == 233002
    reaches = _edge_classes("delta", 4) + _edge_classes("hdr", 4) + _edge_classes("freq", 2) + _edge_classes("hit", 2) + _edge_classes("body", 3)
    return EncCase("google_varints", terms, reaches + ["doc:2^32-2", "freq:65535", "hit_delta:65534", "hit:position0_with_payload"], payloads=True)


def _blocks_term(first_doc, nblocks, last_n, salt):
    """A term of nblocks blocks, the last of last_n documents: documents from first_doc two apart, frequencies 0 .. 2 by rank."""
    n = 32 * (nblocks - 1) + last_n if nblocks else 0
    return _plain(first_doc + 2 * np.arange(n), (np.arange(n) + salt) % 3)


def google_skip_phases(r):
    """A filler term of r blocks in front (the countdown survives terms), then terms of 1 .. 17 blocks whose last block holds 1 and 32 documents."""
    terms = [_blocks_term(1, r, 32, 0)]
    for nb in range(1, 18):
        for last_n in (1, 32):
            terms.append(_blocks_term(1 + nb, nb, last_n, nb))
    c = EncCase(f"google_skip_phases_r{r}", terms, [], upload=True)
    c.reaches = skip_classes(c.tf)[0]  # (which of the 24 a filler length reaches is arithmetic: the union is what the CPU test pins)
    return c


def google_skip_cap():
    """One term of (65535 + 2) * 8 blocks after a 3-block filler: 65537 marked blocks, 65535 entries kept.  Delta 1, frequency 0."""
    n = (SKIP_CAP + 2) * 8 * 32
    z = np.zeros(0, np.int64)
    return EncCase("google_skip_cap", [_blocks_term(1, 3, 32, 0), (np.arange(1, n + 1, dtype=np.int64), np.zeros(n, np.int64), z)], ["skip_cap"], upload=True, oracle=False)


def scan_sizes(n):
    """n one-document terms (n postings, n blocks: both of the encoder's scans run over n values), frequencies 0 .. 2; n = 0: one empty term."""
    if n == 0:
        return EncCase("scan_0", [_plain([], [])], ["scan:0", "block_scan:0"], upload=True)
    i = np.arange(n, dtype=np.int64)
    c = EncCase(f"scan_{n}", [], [f"scan:{n}", f"block_scan:{n}"], upload=True)
    f = i % 3
    c.docs, c.freqs, c.pos, c.tf = (1 + i % 1000).astype(np.uint32), f.astype(np.uint32), ramp(f), np.arange(n + 1, dtype=np.uint64)
    return c


def lucene_blocks():
    """Terms of LUCENE_DOCS documents x LUCENE_HITS hits a document x deltas 1 and 2^20; one huge delta inside a block; groups of equal deltas / frequencies / hit
    deltas; position 65535; full document blocks whose first hit is hit 0 / 1 / 127 (mod 128) of its term."""
    terms = []
    for n in LUCENE_DOCS:
        for h in LUCENE_HITS:
            for d in LUCENE_DELTAS:
                terms.append(_plain(d * np.arange(1, n + 1, dtype=np.int64), np.full(n, h)))
    dl = np.ones(256, np.int64)
    dl[[40, 200]] = [1 << 30, 3]
    fr = 1 + np.arange(256) % 3
    terms.append((np.cumsum(dl), fr, (3 * ramp(fr).astype(np.int64))))  # an exception in block 0; hit deltas all 3
    terms.append((np.arange(1, 4), np.array([1, 2, 1]), np.array([65535, 1, 65535, 65535])))
    for first in (128, 1, 127):  # block 1 of the term starts at hit `first` of the term
        fr = np.concatenate([[first], np.zeros(127, np.int64), 1 + np.arange(130) % 2])
        terms.append(_plain(np.arange(1, fr.size + 1), fr))
    return EncCase("lucene_blocks", terms, LUCENE_CLASSES)


def google_classes(c):
    """The GOOGLE_CLASSES the case's arrays reach, recomputed: varint values per quantity, block bodies from the lengths of their parts, skip phases from block counts,
    scan sizes from array lengths.  Also leaves c.chunk_sizes: per term 2 + blocks + 8 * entries, what the host encoder's term table must say."""
    docs, freqs, pos, tf = c.docs.astype(np.int64), c.freqs.astype(np.int64), c.pos.astype(np.int64), c.tf.astype(np.int64)
    npst, nt = docs.size, tf.size - 1
    out = set()
    df = np.diff(tf)
    nb = (df + 31) // 32
    g0 = np.concatenate([[0], np.cumsum(nb)])
    nblocks = int(g0[-1])
    if npst in SCAN_SIZES:
        out.add(f"scan:{npst}")
    if nblocks in SCAN_SIZES:
        out.add(f"block_scan:{nblocks}")
    term_of = np.repeat(np.arange(nt), df)
    rank = np.arange(npst) - tf[term_of]
    prev = np.where(rank == 0, 0, np.concatenate([[0], docs[:-1]])) if npst else docs
    delta = docs - prev
    last_in_block = (rank % 32 == 31) | (rank == df[term_of] - 1) if npst else np.zeros(0, bool)
    blk = g0[term_of] + rank // 32 if npst else np.zeros(0, np.int64)
    hit0 = np.concatenate([[0], np.cumsum(freqs)])
    post_of = np.repeat(np.arange(npst), freqs)
    hrank = np.arange(pos.size) - hit0[post_of]
    plen = c.plen.astype(np.int64) if c.plen is not None else np.zeros(pos.size, np.int64)
    ppos = np.where(hrank == 0, 0, np.concatenate([[0], pos[:-1]])) if pos.size else pos
    pplen = np.where(hrank == 0, 0, np.concatenate([[0], plen[:-1]])) if pos.size else plen
    chg = (plen != pplen).astype(np.int64)
    hv = ((pos - ppos) << 1) | chg
    hdr = np.zeros(nblocks, np.int64)
    np.add.at(hdr, blk, delta)
    body = np.zeros(nblocks, np.int64)
    if npst:
        np.add.at(body, blk, np.where(last_in_block, 0, vlen(delta)) + vlen(freqs))
    if pos.size:
        np.add.at(body, blk[post_of], vlen(hv) + chg + plen)
    for q, vals, n in (("delta", delta[~last_in_block], 4), ("hdr", hdr, 4), ("freq", freqs, 2), ("hit", hv, 2), ("body", body, 3)):
        have = set(np.unique(vals).tolist())
        for k in range(1, n + 1):
            if VEDGES[k - 1] - 1 in have and VEDGES[k - 1] in have:
                out.add(f"{q}_vlen:{k}|{k + 1}")
    if npst and int(docs.max()) == TOP_DOC:
        out.add("doc:2^32-2")
    if npst and int(freqs.max()) == 65535:
        out.add("freq:65535")
    if pos.size and np.any(pos - ppos == 65534):
        out.add("hit_delta:65534")
    if pos.size and np.any((pos == 0) & (plen > 0)):
        out.add("hit:position0_with_payload")
    boff = np.concatenate([[0], np.cumsum(vlen(hdr) + vlen(body) + 1 + body)]) if nblocks else np.zeros(1, np.int64)
    skip, entries = skip_classes(c.tf)
    c.chunk_sizes = [2 + int(boff[g0[t + 1]] - boff[g0[t]]) + 8 * entries[t] for t in range(nt)]
    return out | skip


def skip_classes(tf):
    """(the skip_phase / skip_cap classes, the skiplist entries per term) from the terms' block counts alone: blocks are counted ACROSS terms, every 8th is marked."""
    nb = (np.diff(np.asarray(tf, dtype=np.int64)) + 31) // 32
    g0 = np.concatenate([[0], np.cumsum(nb)])
    out, entries = set(), []
    for t in range(nb.size):
        a, b = int(g0[t]), int(g0[t + 1])
        kept = 0
        if b > a:
            first_marked = (a + 8) // 8 * 8 - 1
            last = b - 1
            marked = (last - first_marked) // 8 + 1 if last >= first_marked else 0
            kept = min(marked, SKIP_CAP)
            if marked > SKIP_CAP:
                out.add("skip_cap")
            r = a & 7
            if (last + 1) % 8 == 0:
                out.add(f"skip_phase:{r}/on")
            if (last + 2) % 8 == 0:
                out.add(f"skip_phase:{r}/before")
            if last % 8 == 0 and last - 1 >= a:
                out.add(f"skip_phase:{r}/after")
        entries.append(kept)
    return out, entries


def lucene_classes(c):
    """The LUCENE_CLASSES the case's arrays reach."""
    docs, freqs, pos, tf = c.docs.astype(np.int64), c.freqs.astype(np.int64), c.pos.astype(np.int64), c.tf.astype(np.int64)
    hit0 = np.concatenate([[0], np.cumsum(freqs)])
    out = set()
    for t in range(tf.size - 1):
        a, b = int(tf[t]), int(tf[t + 1])
        n = b - a
        d, f = docs[a:b], freqs[a:b]
        delta = np.diff(np.concatenate([[0], d]))
        if n in LUCENE_DOCS:
            out.add(f"lucene_docs:{n}")
        if n and np.all(f == f[0]) and int(f[0]) in LUCENE_HITS:
            out.add(f"lucene_hits:{int(f[0])}")
        if n and np.all(delta == delta[0]) and int(delta[0]) in LUCENE_DELTAS:
            out.add(f"lucene_delta:{int(delta[0])}")
        h = pos[hit0[a] : hit0[b]]
        first = np.zeros(h.size, bool)
        first[(hit0[a:b] - hit0[a])[f > 0]] = True
        hd = h - np.where(first, 0, np.concatenate([[0], h[:-1]]))
        if h.size and int(h.max()) == 65535:
            out.add("lucene_pos:65535")
        for j in range(n // 128):
            bd, bf = delta[128 * j : 128 * j + 128], f[128 * j : 128 * j + 128]
            if np.all(bd == bd[0]):
                out.add("lucene_equal:deltas")
            if np.all(bf == bf[0]):
                out.add("lucene_equal:freqs")
            if int(bd.max()) >= 1 << 20 and int(np.sort(bd)[-2]) <= 3:
                out.add("lucene_exception")
            hb = int(hit0[a + 128 * j] - hit0[a])
            if j and hb % 128 in (0, 1, 127) and hb:
                out.add(f"lucene_hb:{hb % 128}")
        for k in range(h.size // 128):
            if np.all(hd[128 * k : 128 * k + 128] == hd[128 * k]):
                out.add("lucene_equal:hits")
    return out


def encoder_cases():
    """{name: builder} of every encoder case (built on demand: the cap case alone is 16.8 M postings)."""
    out = {"google_varints": google_varints, "google_skip_cap": google_skip_cap, "lucene_blocks": lucene_blocks}
    out.update({f"google_skip_phases_r{r}": (lambda r=r: google_skip_phases(r)) for r in range(8)})
    out.update({f"scan_{n}": (lambda n=n: scan_sizes(n)) for n in SCAN_SIZES})
    out.update({f"pfor_{w}": (lambda w=w: pfor_cases.EncoderCase(w)) for w in ("narrow", "wide")})  # the chosen PFOR128 group shapes (tests/pfor_cases.py)
    return out


GOOGLE_ENCODER_CASES = ["google_varints"] + [f"google_skip_phases_r{r}" for r in range(8)] + [f"scan_{n}" for n in SCAN_SIZES] + ["google_skip_cap"]
LUCENE_ENCODER_CASES = ["lucene_blocks"] + [f"scan_{n}" for n in SCAN_SIZES] + [f"google_skip_phases_r{r}" for r in (0, 5)] + ["pfor_narrow", "pfor_wide"]


def oracle_read_back(name, arrays, index, terms):
    """Every posting of (docs, freqs, pos, term_first, plen, pval) read back from GOOGLE bytes through the oracle: decode_term for documents and frequencies, PLI.next /
    materialize_hits for positions, payload lengths and payload bytes (masked to each payload's own length: term_hit::payload keeps the bytes a shorter payload does not
    overwrite).  Returns the oracle's index."""
    import ctypes as C

    import oracle_lib as O

    docs, freqs, cpos, tf, cplen, cpval = arrays
    L = O.lib()
    ora = O.Index.wrap(index, terms, int(docs.max()) if docs.size else 1, int(docs.size), int(cpos.size))
    hit0 = np.concatenate([[0], np.cumsum(freqs.astype(np.int64))])
    pos, ln, pl = (C.c_uint16 * 65536)(), (C.c_uint8 * 65536)(), (C.c_uint64 * 65536)()
    vpos, vln, vpl = np.frombuffer(pos, dtype=np.uint16), np.frombuffer(ln, dtype=np.uint8), np.frombuffer(pl, dtype=np.uint64)
    plen = cplen if cplen is not None else np.zeros(cpos.size, np.uint8)
    pval = cpval if cpval is not None else np.zeros(cpos.size, np.uint64)
    mask = np.where(plen >= 8, ~np.uint64(0), (np.uint64(1) << (np.uint64(8) * np.minimum(plen, 7).astype(np.uint64))) - np.uint64(1))
    for t in range(tf.size - 1):
        a, b = int(tf[t]), int(tf[t + 1])
        d, f = ora.decode_term(t)
        assert np.array_equal(d, docs[a:b]) and np.array_equal(f, freqs[a:b]), (name, t)
        if not int(hit0[b] - hit0[a]):
            continue
        it = O.PLI(ora, t)
        for i in range(a, b):
            assert L.to_pli_next(it.p) == int(docs[i]), (name, t, i)
            n = L.to_pli_materialize_hits(it.p, pos, ln, pl)
            h0, h1 = int(hit0[i]), int(hit0[i + 1])
            assert n == h1 - h0, (name, t, i, n)
            assert np.array_equal(vpos[:n], cpos[h0:h1]) and np.array_equal(vln[:n], plen[h0:h1]) and np.array_equal(vpl[:n] & mask[h0:h1], pval[h0:h1] & mask[h0:h1]), (name, t, i)
        assert L.to_pli_next(it.p) == O.DOCIDS_END
    return ora


# ---- commit sessions ----------------------------------------------------------------------------------------------------------------------------
class Session:
    """A session's postings in INSERTION order: .arrays = (term_ids, doc_ids, freqs, pos, plen, pval).  refusal: None, or the reason commit must give (a word of its
    message); the sorted posting it must name is first_offence()'s.  needs_payloads: the case only exists with payloads."""

    def __init__(self, name, tids, docs, freqs, pos, plen, pval, reaches, refusal=None, needs_payloads=False):
        self.name, self.reaches, self.refusal, self.needs_payloads = name, set(reaches), refusal, needs_payloads
        self.tids, self.docs, self.freqs = np.asarray(tids, dtype=np.uint32), np.asarray(docs, dtype=np.uint32), np.asarray(freqs, dtype=np.uint32)
        self.pos, self.plen, self.pval = np.asarray(pos, dtype=np.uint16), np.asarray(plen, dtype=np.uint8), np.asarray(pval, dtype=np.uint64)
        assert self.tids.size == self.docs.size == self.freqs.size and self.pos.size == self.plen.size == self.pval.size == int(self.freqs.astype(np.int64).sum()), name

    @property
    def arrays(self):
        return self.tids, self.docs, self.freqs, self.pos, self.plen, self.pval

    def permuted(self, name, order, reaches, **kw):
        order = np.asarray(order, dtype=np.int64)
        hit0 = np.concatenate([[0], np.cumsum(self.freqs.astype(np.int64))])
        take = hit_slices(hit0, order)
        return Session(name, self.tids[order], self.docs[order], self.freqs[order], self.pos[take], self.plen[take], self.pval[take], reaches, **kw)


def _session(name, tids, docs, reaches, salt=0, **kw):
    """Postings (tids[i], docs[i]) with frequencies 0 .. 3 and payload lengths 0 .. 8 by rank, positions 1 .. f."""
    tids, docs = np.asarray(tids, dtype=np.int64), np.asarray(docs, dtype=np.int64)
    f = (np.arange(tids.size) + salt) % 4
    pos = ramp(f)
    plen = (np.arange(pos.size) * 5 + salt) % 9
    pval = np.where(plen == 0, np.uint64(0), _words(pos.size, salt + 1) >> (np.uint64(8) * (np.uint64(8) - np.maximum(plen, 1).astype(np.uint64))))
    return Session(name, tids, docs, f, pos, plen, pval, reaches, **kw)


def commit_sort_order(tids, docs):
    """The walk of SegmentIndexSession::commit: buckets by id & 31, (id, document) ascending inside a bucket; equal (id, document) stay in insertion order."""
    t, d = np.asarray(tids, dtype=np.int64), np.asarray(docs, dtype=np.int64)
    return np.lexsort((d, t, t & 31))


def commit_sessions():
    out = []
    T_, D_ = np.array(COMMIT_TERM_IDS, dtype=np.int64), np.array(COMMIT_DOC_IDS, dtype=np.int64)
    tt, dd = np.repeat(T_, D_.size), np.tile(D_, T_.size)  # every term in every document, term-major
    ids = ["commit_term:>=2^27", "commit_term:2^31", "commit_term:2^32-1", "commit_term:low5_equal", "commit_doc:2^32-2"]
    base = _session("ids_any", tt, dd, [])
    srt = commit_sort_order(tt, dd)
    out.append(base.permuted("ids_sorted", srt, ids + ["commit_order:sorted"]))
    out.append(base.permuted("ids_reversed", srt[::-1], ids + ["commit_order:reversed"]))
    rng = np.random.default_rng(7)
    dm = np.lexsort((rng.random(tt.size), rng.permutation(D_.size)[np.tile(np.arange(D_.size), T_.size)]))
    out.append(base.permuted("ids_document_major", dm, ids + ["commit_order:document_major"]))
    out.append(_session("one_term_everywhere", np.full(100, 2**31 + 31), np.arange(100, 0, -1), ["commit_one_term_everywhere"], salt=1))
    out.append(_session("one_document_all_terms", (np.arange(100, 0, -1) * 0x01000193) % 2**32, np.full(100, 77), ["commit_one_document_all_terms"], salt=2))
    nh = _session("no_hits", tt, dd, ["commit_no_hits"])
    out.append(Session("no_hits", nh.tids, nh.docs, np.zeros(tt.size), [], [], [], ["commit_no_hits"]))
    for n in COMMIT_SIZES:  # 97 terms (ids spread over all 32 bits), every document holds all of them, documents inserted in descending order
        i = np.arange(n, dtype=np.int64)
        out.append(_session(f"postings_{n}", ((i % 97 + 1) * 0x9E3779B1) % 2**32, n // 97 + 1 - i // 97, [f"commit_scan:{n}"], salt=n))
    # ---- refusals
    out.append(_session("refuse_document0_first", [40, 40, 8, 8], [3, 3, 0, 9], ["refuse:document0_before_duplicate"], refusal="document 0"))  # (bucket 8 before bucket 8 + 32)
    out.append(_session("refuse_duplicate_first", [8, 8, 40, 40], [3, 3, 0, 9], ["refuse:duplicate_before_document0"], refusal="twice"))
    t50, d50 = np.concatenate([[33], 1 + np.arange(48) % 7, [33]]), np.concatenate([[500], 1 + np.arange(48) // 7, [500]])
    out.append(_session("refuse_duplicate_far_apart", t50, d50, ["refuse:duplicate_first_and_last_inserted"], refusal="twice"))
    out.append(_session("refuse_duplicate_last", [5, 31, 2**32 - 1, 2**32 - 1, 31], [1, TOP_DOC, TOP_DOC, TOP_DOC, 2], ["refuse:duplicate_last_two_sorted"], refusal="twice"))
    i = np.arange(ENC_SCAN_CHUNK + 40, dtype=np.int64)  # one term, documents descending; the copy of sorted posting 32767 is inserted last
    out.append(_session("refuse_duplicate_across_chunk", np.full(i.size + 1, 64), np.concatenate([i.size - i, [ENC_SCAN_CHUNK]]), ["refuse:duplicate_across_chunk"], refusal="twice"))
    ok = _session("x", [9, 9, 9], [1, 2, 3], [])
    out.append(Session("refuse_positions", ok.tids, ok.docs, [1, 2, 3], [4, 9, 3, 1, 2, 3], [0, 0, 0, 0, 0, 0], [0] * 6, ["refuse:positions"], refusal="positions"))
    out.append(Session("refuse_payload9", ok.tids, ok.docs, [1, 2, 3], [4, 3, 9, 1, 2, 3], [0, 0, 8, 0, 9, 0], [0, 0, 5, 0, 6, 0], ["refuse:payload9"], refusal="payload of more than 8",
                       needs_payloads=True))  # fmt: skip
    return out


def first_offence(s, payloads):
    """(sorted posting, why) of the smallest sorted posting commit refuses — why 1: document 0; 2: the same (term, document) as the posting before; 3: positions; 4: a payload
    of more than 8 bytes (a posting's first offending hit decides between 3 and 4) — or None."""
    order = commit_sort_order(s.tids, s.docs)
    t, d, f = s.tids[order].astype(np.int64), s.docs[order].astype(np.int64), s.freqs[order].astype(np.int64)
    hit0 = np.concatenate([[0], np.cumsum(s.freqs.astype(np.int64))])
    take = hit_slices(hit0, order)
    pos = s.pos[take].astype(np.int64)
    plen = s.plen[take].astype(np.int64) if payloads else np.zeros(pos.size, np.int64)
    why = np.zeros(t.size, np.int64)
    o0 = np.concatenate([[0], np.cumsum(f)])
    post_of = np.repeat(np.arange(t.size), f)
    hrank = np.arange(pos.size) - o0[post_of]
    ppos = np.where(hrank == 0, 0, np.concatenate([[0], pos[:-1]])) if pos.size else pos
    code = np.where(plen > 8, 4, np.where(((pos == 0) & (plen == 0)) | (pos < ppos), 3, 0))
    bad = np.flatnonzero(code)
    if bad.size:
        p, at = np.unique(post_of[bad], return_index=True)
        why[p] = code[bad[at]]
    dup = np.concatenate([[False], (t[1:] == t[:-1]) & (d[1:] == d[:-1])])
    why = np.where(d == 0, 1, np.where(dup, 2, why))
    j = np.flatnonzero(why)
    return (int(j[0]), int(why[j[0]])) if j.size else None


def commit_reference(s, payloads):
    """(termIDs in commit order, encoder arrays (docs, freqs, pos, term_first, plen, pval), stats) of an accepted session."""
    order = commit_sort_order(s.tids, s.docs)
    t = s.tids[order]
    hit0 = np.concatenate([[0], np.cumsum(s.freqs.astype(np.int64))])
    take = hit_slices(hit0, order)
    opens = np.flatnonzero(np.concatenate([[True], t[1:] != t[:-1]])) if t.size else np.zeros(0, np.int64)
    tf = np.concatenate([opens, [t.size]]).astype(np.uint64)
    runs = int(1 + np.count_nonzero(s.docs[1:] != s.docs[:-1])) if s.docs.size else 0  # (a session inserts document after document: one run of postings each)
    stats = {"docs_cnt": runs, "sum_terms_docs": int(t.size), "sum_term_hits": int(s.freqs.astype(np.int64).sum()), "total_terms": int(opens.size)}
    return t[opens], (s.docs[order], s.freqs[order], s.pos[take], tf, s.plen[take] if payloads else None, s.pval[take] if payloads else None), stats


def commit_classes(s):
    """The COMMIT_CLASSES the session's arrays reach."""
    out = set()
    t, d = s.tids.astype(np.int64), s.docs.astype(np.int64)
    n = t.size
    order = commit_sort_order(t, d)
    off = first_offence(s, True)
    if off is None:
        ut = np.unique(t)
        if np.any((ut >= 2**27) & (ut < 2**31)):
            out.add("commit_term:>=2^27")
        if 2**31 in ut:
            out.add("commit_term:2^31")
        if 2**32 - 1 in ut:
            out.add("commit_term:2^32-1")
        if any(np.unique(ut[(ut & 31) == b] >> 5).size > 1 for b in np.unique(ut & 31)):
            out.add("commit_term:low5_equal")
        if TOP_DOC in d:
            out.add("commit_doc:2^32-2")
        if n > 1 and np.unique(t).size > 1 and np.unique(d).size > 1:
            if np.array_equal(order, np.arange(n)):
                out.add("commit_order:sorted")
            if np.array_equal(order, np.arange(n)[::-1]):
                out.add("commit_order:reversed")
            runs = 1 + np.count_nonzero(d[1:] != d[:-1])
            if runs == np.unique(d).size and not np.array_equal(order, np.arange(n)) and np.any(np.diff(d) < 0):
                out.add("commit_order:document_major")
        if n > 1 and np.unique(t).size == 1:
            out.add("commit_one_term_everywhere")
        if n > 1 and np.unique(d).size == 1:
            out.add("commit_one_document_all_terms")
        if n and not s.freqs.any():
            out.add("commit_no_hits")
        if n in COMMIT_SIZES:
            out.add(f"commit_scan:{n}")
        return out
    j, why = off
    st, sd = t[order], d[order]
    dup = np.flatnonzero(np.concatenate([[False], (st[1:] == st[:-1]) & (sd[1:] == sd[:-1])]))
    zero = np.flatnonzero(sd == 0)
    if why == 1 and dup.size and j < dup[0]:
        out.add("refuse:document0_before_duplicate")
    if why == 2 and zero.size and j < zero[0]:
        out.add("refuse:duplicate_before_document0")
    if why == 2 and {int(order[j - 1]), int(order[j])} == {0, n - 1} and n > 32:
        out.add("refuse:duplicate_first_and_last_inserted")
    if why == 2 and j == n - 1:
        out.add("refuse:duplicate_last_two_sorted")
    if why == 2 and j == ENC_SCAN_CHUNK and abs(int(order[j]) - int(order[j - 1])) > 1024:
        out.add("refuse:duplicate_across_chunk")
    if why == 3:
        out.add("refuse:positions")
    if why == 4 and first_offence(s, False) is None:
        out.add("refuse:payload9")
    return out


# ---- merges -------------------------------------------------------------------------------------------------------------------------------------
class Part:
    """One participant: its terms' postings (encoder arrays), its masked documents (None: no mask installed) and the docs_cnt it is uploaded with."""

    def __init__(self, terms, masked, codec):
        c = EncCase("part", terms, [], payloads=codec == 1)
        self.docs, self.freqs, self.pos, self.tf, self.plen, self.pval = c.arrays
        self.masked = None if masked is None else np.unique(np.asarray(masked, dtype=np.uint32))
        self.docs_cnt = max(64, int(self.docs.max()) if self.docs.size else 0)
        self.hit0 = np.concatenate([[0], np.cumsum(self.freqs.astype(np.int64))])

    def lists(self, k):
        """Term k as merge_restated wants it: [(doc, [(pos, payload length, payload), ...]), ...]."""
        out = []
        for i in range(int(self.tf[k]), int(self.tf[k + 1])):
            a, b = int(self.hit0[i]), int(self.hit0[i + 1])
            hits = [(int(self.pos[h]), int(self.plen[h]) if self.plen is not None else 0, int(self.pval[h]) if self.pval is not None else 0) for h in range(a, b)]
            out.append((int(self.docs[i]), hits))
        return out


class MergeCase:
    def __init__(self, name, codec, parts, part_terms, reaches):
        self.name, self.codec, self.parts, self.reaches = name, codec, parts, {("g:" if codec == 1 else "l:") + r for r in reaches}
        self.part_terms = np.asarray(part_terms, dtype=np.uint32).reshape(-1, len(parts))


def _mterm(codec, docs, freqs, salt=0):
    """A participant's term: positions 1 .. f; GOOGLE: payload lengths 0 .. 8 by hit rank on every other term."""
    d, f, p = _plain(docs, freqs)
    if codec == 2:
        return (d, f, p)
    plen = (np.arange(p.size) * 7 + salt) % 9 if salt % 2 == 0 else np.zeros(p.size, np.int64)
    pval = _words(p.size, salt + 11) >> (np.uint64(8) * (np.uint64(8) - np.maximum(plen, 1).astype(np.uint64)))
    return (d, f, p, plen, np.where(plen == 0, np.uint64(0), pval))


def merge_cases(codec):
    """The merge rows of the issue's table for one codec (1: GOOGLE, 2: LUCENE).  documentIDs below 100 000."""
    sizes = MERGE_PART_DOCS[codec]
    out = []
    M = lambda d, f, salt=0: _mterm(codec, d, f, salt)
    # every document in every participant; the most recent one has no hits where the older has some; participant 0 has no mask installed, participant 1 masks a few
    t0 = [M(3 * np.arange(1, n + 1), np.where(np.arange(n) % 2, 0, 1), salt=k) for k, n in enumerate(sizes)]
    t1 = [M(3 * np.arange(1, n + 1), np.full(n, 2), salt=k + 1) for k, n in enumerate(sizes)]
    out.append(MergeCase("everywhere", codec, [Part(t0, None, codec), Part(t1, [3, 6, 9], codec)], [[k, k] for k in range(len(sizes))],
                         ["every_document_everywhere", "winner_freq0_loser_hits", "unmasked_next_to_masked", "participants:2"] + [f"part_docs:{n}" for n in sizes]))  # fmt: skip
    # the winner masked, an older participant holds the document unmasked: dropped.  Masks on documents 31, 32 and the participant's last; merged lists of exactly L
    t0 = [M(1000 * k + np.arange(1, L + 4), 1 + np.arange(L + 3) % 3, salt=L) for k, L in enumerate(MERGE_LENS)]  # (term k lives in documents 1000 k + 1 ...)
    t1 = [M([1000 * k + 31, 1000 * k + 32, 1000 * k + L + 3], [1, 1, 1], salt=L + 1) for k, L in enumerate(MERGE_LENS)]
    m0 = [1000 * k + x for k, L in enumerate(MERGE_LENS) for x in (31, 32, L + 3)]
    out.append(MergeCase("winner_masked", codec, [Part(t0, m0, codec), Part(t1, None, codec)], [[k, k] for k in range(len(MERGE_LENS))],
                         ["winner_masked_loser_unmasked", "mask_bit:31", "mask_bit:32", "mask_bit:last_document"] + [f"merged_len:{L}" for L in MERGE_LENS]))  # fmt: skip
    a, b = np.arange(1, 70), np.arange(40, 140)
    out.append(MergeCase("everything_masked", codec, [Part([M(a, 1 + a % 2)], a, codec), Part([M(b, 1 + b % 3, 1)], np.arange(1, 200), codec)], [[0, 0]], ["everything_masked"]))
    out.append(MergeCase("every_term_empty", codec, [Part([M([], []), M([], [])], [5], codec), Part([M([], [])], None, codec)], [[0, 0], [1, ABSENT]], ["every_term_empty"]))
    # five participants; 1 (its only named term is empty) and 3 (names nothing) have no job and mask everything; 2 has no mask installed
    everything = np.arange(1, 2000)
    parts = [Part([M(np.arange(5, 500, 5), np.arange(99) % 3)], [10, 100], codec), Part([M([], []), M([7, 8], [1, 1])], everything, codec),
             Part([M(np.arange(10, 600, 10), 1 + np.arange(59) % 2, 2)], None, codec), Part([M(np.arange(1, 50), np.ones(49, np.int64))], everything, codec),
             Part([M(np.arange(3, 900, 3), np.arange(299) % 2, 4)], [3, 30, 300, 897], codec)]  # fmt: skip
    out.append(MergeCase("empty_between", codec, parts, [[0, 0, 0, ABSENT, 0]], ["empty_participant_between", "unmasked_next_to_masked", "participants:5"]))
    # seventeen participants, each with three terms in its own order: part_terms falls where the output terms rise
    parts, pt = [], np.full((3, 17), ABSENT, dtype=np.int64)
    for p in range(17):
        terms = [M(np.arange(1 + p, 400, 2 + (p + k) % 5), (np.arange(len(range(1 + p, 400, 2 + (p + k) % 5))) + p) % 3, salt=p + k) for k in range(3)]
        parts.append(Part(terms, None if p % 3 == 0 else np.arange(p, 400, 7 + p), codec))
        for k in range(3):
            if (p + k) % 4:
                pt[2 - k, p] = k
    out.append(MergeCase("seventeen", codec, parts, pt, ["participants:17", "part_terms_not_monotone", "unmasked_next_to_masked"]))
    # one participant; a 32-document row without hits; a term with documents and no hits
    n = 200
    f = np.where((np.arange(n) >= 32) & (np.arange(n) < 64), 0, 1 + np.arange(n) % 4)
    terms = [M(7 * np.arange(1, n + 1), f, salt=1), M(np.arange(1, 71), np.zeros(70, np.int64))]
    extra = []
    if codec == 1:  # a document whose last hit carries 8 bytes, then one whose first hit carries none
        pl = [0, 8, 0, 8, 8, 0, 3, 8, 0]
        terms.append((np.array([4, 5, 6, 9]), np.array([2, 3, 1, 3]), np.array([1, 2, 1, 5, 5, 2, 7, 9, 9]), np.array(pl), np.where(np.array(pl) > 0, _words(9, 5), np.uint64(0))))
        extra = ["payload_8_then_none"]
    else:
        extra = ["row_inside_hit_block"]
    out.append(MergeCase("single", codec, [Part(terms, [14, 7 * n], codec)], [[k] for k in range(len(terms))], ["participants:1", "row_without_hits", "term_without_hits"] + extra))
    return out


def merge_reference(c):
    """(merged lists per output term, encoder arrays, stats): merge_restated.merge_term over the participants' lists, most recent first, each with its own masked set."""
    masks = [None if p.masked is None else set(p.masked.tolist()) for p in c.parts]
    merged = []
    for row in c.part_terms.tolist():
        merged.append(merge_term([None if k == ABSENT else p.lists(k) for k, p in zip(row, c.parts)], masks))
    arrays = encoder_arrays(merged)
    stats = {"docs_cnt": 0, "sum_terms_docs": int(arrays[0].size), "sum_term_hits": int(arrays[1].astype(np.int64).sum()), "total_terms": sum(1 for m in merged if m)}
    return merged, arrays, stats


def merge_classes(c, merged):
    """The merge classes the case reaches, recomputed from its participants, masks, part_terms and the reference's merged lists."""
    out = set()
    nparts = len(c.parts)
    pt = c.part_terms.astype(np.int64)
    df = [np.diff(p.tf.astype(np.int64)) for p in c.parts]
    jobs = [[(t, int(k)) for t, k in enumerate(pt[:, p].tolist()) if k != ABSENT and df[p][k] > 0] for p in range(nparts)]
    has = [bool(j) for j in jobs]
    if nparts in MERGE_PARTS:
        out.add(f"participants:{nparts}")
    for p in range(1, nparts - 1):
        if not has[p] and any(has[:p]) and any(has[p + 1 :]) and c.parts[p].masked is not None and c.parts[p].masked.size > 100:
            out.add("empty_participant_between")
    if any(c.parts[p].masked is None and has[p] and (c.parts[q].masked is not None) for p in range(nparts) for q in (p - 1, p + 1) if 0 <= q < nparts):
        out.add("unmasked_next_to_masked")
    if not any(has):
        out.add("every_term_empty")
    elif not any(merged):
        out.add("everything_masked")
    for p in range(nparts):
        col = pt[:, p][pt[:, p] != ABSENT]
        if np.any(np.diff(col) < 0):
            out.add("part_terms_not_monotone")
        for t, k in jobs[p]:
            if int(df[p][k]) in MERGE_PART_DOCS[c.codec]:
                out.add(f"part_docs:{int(df[p][k])}")
        m = c.parts[p].masked
        if m is not None and has[p]:
            held = c.parts[p].docs
            for bit in (31, 32):
                if bit in m and bit in held:
                    out.add(f"mask_bit:{bit}")
            if held.size and int(held.max()) in m:
                out.add("mask_bit:last_document")
    for t, row in enumerate(pt.tolist()):
        held = [(p, c.parts[p].lists(k)) for p, k in enumerate(row) if k != ABSENT and df[p][k] > 0]
        if len(held) > 1 and len(held) == nparts and all([d for d, _ in l] == [d for d, _ in held[0][1]] for _, l in held):
            out.add("every_document_everywhere")
        kept = {d for d, _ in merged[t]}
        if len(merged[t]) in MERGE_LENS and any(c.parts[p].masked is not None for p, _ in held):
            out.add(f"merged_len:{len(merged[t])}")
        seen = {}
        for p, l in held:
            for d, hits in l:
                if d in seen:
                    p0, h0 = seen[d]
                    m0, m1 = c.parts[p0].masked, c.parts[p].masked
                    if d not in kept and m0 is not None and d in m0 and (m1 is None or d not in m1):
                        out.add("winner_masked_loser_unmasked")
                    if d in kept and not h0 and hits:
                        out.add("winner_freq0_loser_hits")
                else:
                    seen[d] = (p, hits)
            f = [len(h) for _, h in l]
            if f and not sum(f):
                out.add("term_without_hits")
            before = 0
            for r in range(0, len(f), 32):
                if len(f) - r >= 32 and sum(f) and not sum(f[r : r + 32]):
                    out.add("row_without_hits")
                if r and before % 128 and sum(f[r : r + 32]):
                    out.add("row_inside_hit_block")
                before += sum(f[r : r + 32])
            for (_, ha), (_, hb) in zip(l[:-1], l[1:]):
                if ha and hb and ha[-1][1] == 8 and hb[0][1] == 0:
                    out.add("payload_8_then_none")
    return {("g:" if c.codec == 1 else "l:") + x for x in out}


# ---- the reference's own fixtures as sessions and merges (tests/golden/ref_commit.json, ref_merge.json) --------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture_hits(hs):
    return [(int(h[0]), int(h[1]), int(h[2])) for h in hs]


def golden_commit_sessions():
    """[(fixture record, Session)]: every session of ref_commit.json in its insertion order (document after document, a document's terms as the fixture lists them)."""
    with open(os.path.join(GOLDEN, "ref_commit.json")) as f:
        fixture = json.load(f)
    out = []
    for rec in fixture["results"]:
        tids, docs, freqs, hits = [], [], [], []
        for d in rec["docs"]:
            for t in d["terms"]:
                hs = _fixture_hits(t["hits"])
                tids.append(t["id"])
                docs.append(d["d"])
                freqs.append(len(hs))
                hits += hs
        out.append((rec, Session(f"ref_commit_{rec['seed']}", tids, docs, freqs, [h[0] for h in hits], [h[1] for h in hits], np.array([h[2] for h in hits], dtype=np.uint64), [])))
    return out


def golden_merge_cases():
    """[(fixture record, MergeCase)]: every case of ref_merge.json — the participants' input postings term after term (ascending `g`), nothing masked; output term t is
    rec["out"][t]."""
    with open(os.path.join(GOLDEN, "ref_merge.json")) as f:
        fixture = json.load(f)
    out = []
    for rec in fixture["results"]:
        parts, index_of = [], []
        for part in rec["parts"]:
            held = sorted(part, key=lambda t: t["g"])
            terms = []
            for t in held:
                hs = [_fixture_hits(x) for x in t["hits"]]
                flat = [h for x in hs for h in x]
                terms.append((t["docs"], [len(x) for x in hs], [h[0] for h in flat], [h[1] for h in flat], np.array([h[2] for h in flat], dtype=np.uint64)))
            parts.append(Part(terms, None, 1))
            index_of.append({t["g"]: k for k, t in enumerate(held)})
        pt = [[ix.get(o["g"], ABSENT) for ix in index_of] for o in rec["out"]]
        out.append((rec, MergeCase(f"ref_merge_{rec['seed']}", 1, parts, pt, [])))
    return out
