"""Lists whose PFOR128 groups have CHOSEN shapes (a helper module, imported by tests/test_pfor_cases.py, tests/test_gpu_pfor.py and tests/write_cases.py).

Every kernel that reads a Lucene-shaped segment decodes ints() groups (include/pfor128.md) with LValStream (csrc/codec_streams.hpp), PfRegs<8> (deltas) or
PfRegs<4> (freqs; both csrc/k_fused.hpp).  The other corpora of the suite never choose the widths they feed them.  Here every 128-value group is written value by
value so that the cost rule of the encoders picks an intended (b, nexc, eb) with intended exception counts per quarter; tests/test_pfor_cases.py parses the header
word of every group out of the host encoder's bytes and holds it against SHAPES below, because nothing on the device reports which decoder path ran.

The yardstick is the input: explicit postings (and explicit positions), encoded through structured.build.  plan() restates the encoders' cost rule only to
CONSTRUCT groups (make() refuses a shape the rule would not pick); nothing here comes from the engine.

Two corpora, so that only the lists that need a large docID space pay for one:
  narrow  D = 3 SPAN_BITS + 37.  Every freqs shape, every hits.data shape, the deltas shapes whose values stay below 2^11.
  wide    D = 2^26 + 37.  Deltas widths 12 .. 20, an all-equal group of a 3-byte varint, exceptions of 16, 17 and 25 bits.
A term is G whole 128-document blocks of ONE shape (salted: the same header, other values) and a varbyte tail of five documents.  `mixed_d` / `mixed_f` string
every deltas / freqs shape of their corpus block after block: the lanes of one wave then carry different b, cnt and eb at once (PfRegs::next branches on wave
ballots and selects per lane).  `x_both` has exceptions on both sides of a block.  `p_dense` / `p_sparse` are the partners of the queries: a grid over the
docID space plus every second / third document of every catalogue list, so that a conjunction keeps a known part of the list.

Every list carries hits.data: both encoders count a frequency from the positions they are handed, so a frequency cannot be written without its hits.  The freqs
lists of widths up to 16 therefore hold documents of up to 65535 hits (about 6 M hits in the narrow corpus, non-decreasing positions 1 .. 16381 where a
document has more hits than positions); make() keeps them few by using the fewest large values a width needs.

What the value ranges do NOT admit (the CPU file states the same in its table):
  * a deltas (or position) group of width 1 without exceptions: values >= 1 below 2 are all equal, which is the all-equal form.  Width 1 is reached with exceptions
    (`d_x_4x16`, `d_x_4x17`, `d_x_ebmax`), and in hits.data with repeated positions (`h_w1`: deltas 0 and 1);
  * freqs: a frequency is below 2^16 (tokenpos_t), so b + eb <= 16: no 4 x 17 on that side, the largest eb is 16 (at b = 0);
  * deltas: D <= 2^26 + 37, so widths 21 .. 32 and eb > 25 are out of reach (eb = 25 once, at b = 1: 2^25 .. 2^26 - 1 is one delta of the whole list);
  * an exception width of 1 needs at most 12 exceptions in the GROUP (13 cost more than one more packed bit), 17 in a quarter need eb >= 2, 32 need eb >= 3 (33 in the group: eb >= 4);
  * positions stay below MaxPosition = 2^14, so hits.data widths end at 14.
"""
import numpy as np

import structured as S

BLOCK = 128
D_NARROW = 3 * S.SPAN_BITS + 37  # more than 261 * 1024: a shape list (261 documents) gets no term plane under the default plane_div (planner: df >= docs / 1024)
D_WIDE = (1 << 26) + 37
GROUPS = 2  # whole blocks of a shape list
TAIL_DELTAS = [1, 130, 2, 17000, 3]  # the varbyte tail: one-, two- and three-byte deltas
TAIL_FREQS = [1, 0, 200, 2, 3]
MAX_POS = (1 << 14) - 3  # positions of the hits lists (their partners sit up to two further)
FREQ_BITS = 16
DENSE_STEP = {"narrow": 16, "wide": 120}  # p_dense's grid: a head term (it gets a plane: df >= docs / 1024) long enough to carry a k_psets scatter union (4 df >= docs / 32)
# the literals of csrc/k_fused.hpp PfRegs (tests/test_pfor_cases.py::test_kernel_literals_mirror parses the header)
NW_DELTAS, NW_FREQS = 8, 4
FAST_MAX_CNT, FAST_MAX_BITS = 16, 64


def falls_back(cnt, eb):
    """PfRegs::init refuses the quarter (k_fused.hpp: `if (cnt > 16 || cnt * eb > 64) return false;`): the row goes through the general streams."""
    return cnt > FAST_MAX_CNT or cnt * eb > FAST_MAX_BITS


def refills(b, nw):
    """Half-queue fetches a quarter of width b costs PfRegs<nw> (k_fused.hpp: `used == NW / 2 && b > NW`; a quarter is b words, nw are loaded at init)."""
    return 0 if b <= nw else -(-(b - nw) // (nw // 2))


# ---- the cost rule, restated to construct groups ------------------------------------------------------------------------------------------------
def bitlen(x):
    return int(x).bit_length()


def cost(b, n, eb):
    return 4 * b + (n + 3) // 4 + (n * eb + 31) // 32


def plan(v):
    """(b, nexc, eb) the encoders pick for 128 values (include/pfor128.md: the smallest cost, ties to the smaller b; 32 only when nothing smaller wins), or
    ("eq", value) for the all-equal form."""
    v = np.asarray(v, dtype=np.uint64)
    assert v.size == BLOCK
    if np.all(v == v[0]):
        return ("eq", int(v[0]))
    best = (32, 0, 0, 4 * 32)
    for b in range(32):
        h = v >> np.uint64(b)
        n, eb = int(np.count_nonzero(h)), bitlen(h.max())
        c = cost(b, n, eb)
        if c < best[3]:
            best = (b, n, eb, c)
    return best[:3]


def quarter_positions(c):
    """c in-quarter positions, 0 and 31 among them from two on."""
    return [5] if c == 1 else sorted({(j * 31 + (c - 1) // 2) // (c - 1) for j in range(c)}) if c else []


def make(b, counts=(0, 0, 0, 0), eb=0, floor=1, salt=0, positions=None, top=None):
    """128 values the cost rule encodes at width b with counts[q] exceptions of eb bits in quarter q.  The non-exception values are the FEWEST large ones that
    keep every narrower width dearer (so a list of wide groups stays inside its docID space), the rest `floor`; exception high parts all have their top bit set,
    so no wider b sheds one.  positions: {quarter: in-quarter positions}.  top: the largest value allowed (positions stay below MaxPosition).  Raises when
    the rule would pick another header."""
    nexc = sum(counts)
    where = []
    for q, c in enumerate(counts):
        ps = (positions or {}).get(q) or quarter_positions(c)
        assert len(ps) == c and len(set(ps)) == c and all(0 <= p < 32 for p in ps), (q, c, ps)
        where += [32 * q + p for p in ps]
    free = [i for i in range(BLOCK) if i not in set(where)]
    target = cost(b, nexc, eb)
    big = []  # non-exception values, level by level: level k lies in [2^(b-k), 2^(b-k+1))
    for k in range(1, b + 1):
        m = len(big)
        while m < len(free) and cost(b - k, nexc + m, (eb if nexc else 0) + k) <= target:
            m += 1
        lo = 1 << (b - k)
        for j in range(len(big), m):
            big.append(min(lo + ((j * 5 + salt * 3 + 1) % lo if k > 1 or j else lo - 1), top or (1 << 32)))  # (the first one is 2^b - 1: the width's largest value)
    v = np.full(BLOCK, floor if b else 0, dtype=np.int64)
    order = [free[(j * 37 + 11 * salt) % len(free)] for j in range(len(free))]  # (37 is coprime to every count of free places up to 128)
    assert len(set(order)) == len(free)
    for j, x in enumerate(big):
        v[order[j]] = x
    for j, i in enumerate(where):
        high = (1 << (eb - 1)) | ((j * 7 + salt) % (1 << (eb - 1)))
        v[i] = (high << b) | ((j + salt) % (1 << b) if b else 0)
    got = plan(v)
    assert got == (b, nexc, eb), ("the cost rule does not admit this shape", (b, counts, eb), got)
    return v


def make_eq(value):
    return np.full(BLOCK, value, dtype=np.int64)


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------------
# exception shapes: tag -> (counts per quarter, eb, positions); the width b is chosen per side below
EXC = {
    "1_8_0_9": ((1, 8, 0, 9), 4, {0: [0]}),  # counts 1, 8 and 9; an empty quarter between two that have some; position 0 alone; e0 * eb = 4 and 36 (hs != 0)
    "2_16": ((2, 16, 0, 0), 4, None),  # 16 x 4 = 64 bits: stays fast; e0 = 2, e0 * eb = 8 (hs == 0 with e0 > 0)
    "4x16": ((0, 4, 0, 4), 16, None),  # 4 x 16 = 64 bits: stays fast; e0 = 4 of quarter 3 at bit 64
    "13x5": ((1, 13, 0, 0), 5, None),  # 13 x 5 = 65 bits: quarter 1 falls back (quarter 0 of the same group does not); e0 * eb = 5
    "4x17": ((0, 0, 4, 1), 17, None),  # 4 x 17 = 68 bits: quarter 2 falls back; quarter 3 starts at bit 68
    "17": ((17, 0, 0, 1), 2, None),  # 17 in a quarter: cnt > 16
    "32": ((1, 32, 0, 0), 4, None),  # a whole quarter (33 exceptions of 3 bits would lose to 3 more packed bits)
    "q3": ((0, 0, 0, 2), 1, {3: [0, 31]}),  # exceptions in quarter 3 only (its e0 is 0: the list starts there), at positions 0 and 31; eb = 1
    "e5": ((2, 3, 0, 0), 5, {0: [0, 31], 1: [0, 15, 31]}),  # eb = 5, e0 * eb = 10
    "e8": ((0, 3, 0, 5), 8, None),  # eb = 8, e0 * eb = 24: a multiple of 8 with e0 > 0
    "ebmax": ((0, 0, 1, 0), 25, {2: [31]}),  # deltas only: one delta of 2^25 .. 2^26 - 1
    "w0_e1": ((2, 0, 1, 0), 1, None),  # freqs only, b = 0: most documents at frequency 0, three at 1
    "w0_e9": ((3, 0, 4, 1), 9, {0: [0, 7, 31]}),  # freqs only, b = 0: frequencies 256 .. 511 among zeros
}
# name -> (side, corpus, b, counts, eb, groups) of every shape list; "eq" shapes carry the value as b
SHAPES = {}
for _w in range(2, 21):
    SHAPES[f"d_w{_w}"] = ("d", "narrow" if _w <= 11 else "wide", _w, (0, 0, 0, 0), 0, GROUPS)
SHAPES.update({"d_eq1": ("d", "narrow", ("eq", 5), None, 0, GROUPS), "d_eq2": ("d", "narrow", ("eq", 300), None, 0, GROUPS), "d_eq3": ("d", "wide", ("eq", 20000), None, 0, GROUPS)})
for _t, _b, _c in (("1_8_0_9", 3, "narrow"), ("2_16", 3, "narrow"), ("4x16", 1, "wide"), ("13x5", 3, "narrow"), ("4x17", 1, "wide"), ("17", 3, "narrow"), ("32", 2, "narrow"),
                   ("q3", 4, "narrow"), ("e5", 3, "narrow"), ("e8", 2, "narrow"), ("ebmax", 1, "wide")):  # fmt: skip
    SHAPES[f"d_x_{_t}"] = ("d", _c, _b, EXC[_t][0], EXC[_t][1], 1 if _t == "ebmax" else GROUPS)
for _w in range(1, FREQ_BITS + 1):
    SHAPES[f"f_w{_w}"] = ("f", "narrow", _w, (0, 0, 0, 0), 0, GROUPS)
SHAPES.update({"f_eq0": ("f", "narrow", ("eq", 0), None, 0, GROUPS), "f_eq1": ("f", "narrow", ("eq", 3), None, 0, GROUPS), "f_eq2": ("f", "narrow", ("eq", 200), None, 0, GROUPS)})
for _t, _b in (("1_8_0_9", 2), ("2_16", 2), ("4x16", 0), ("13x5", 2), ("17", 2), ("32", 1), ("q3", 3), ("e5", 2), ("e8", 2), ("w0_e1", 0), ("w0_e9", 0)):
    SHAPES[f"f_x_{_t}"] = ("f", "narrow", _b, EXC[_t][0], EXC[_t][1], GROUPS)
for _w in range(1, 15):
    SHAPES[f"h_w{_w}"] = ("h", "narrow", _w, (0, 0, 0, 0), 0, GROUPS)
SHAPES.update({"h_eq": ("h", "narrow", ("eq", 7), None, 0, GROUPS), "h_x1": ("h", "narrow", 2, (1, 0, 0, 0), 3, GROUPS), "h_x9": ("h", "narrow", 2, (0, 9, 0, 0), 4, GROUPS),
               "h_x17": ("h", "narrow", 3, (0, 0, 17, 1), 5, GROUPS)})  # fmt: skip
# the other side of an exception list is plain: the rows of a d_x list that refuse PfRegs<8> do so with PfRegs<4> willing, and the reverse
JOINT_DELTAS_FALL_BACK = ["d_x_13x5", "d_x_4x17", "d_x_17", "d_x_32"]
JOINT_FREQS_FALL_BACK = ["f_x_13x5", "f_x_17", "f_x_32"]
BOTH = ("x_both", "1_8_0_9", 3, "2_16", 2)  # exceptions on both sides of one block, both fast
STRADDLE = ("h_straddle", 2, 9, 90, 100)  # a group of width 2, a group of width 9, a document of 100 hits from hit ordinal 90 on


def shape_group(name, g=0):
    """Group g of shape list `name`."""
    side, _, b, counts, eb, _ = SHAPES[name]
    if isinstance(b, tuple):
        return make_eq(b[1])
    pos = EXC[name.split("_x_")[1]][2] if "_x_" in name else None
    if side == "h":
        if b == 1:  # values 0 and 1: documents of two hits, the second on the first one's position or right behind it
            v = np.ones(BLOCK, dtype=np.int64)
            v[1::2] = (np.arange(BLOCK // 2) * 3 + g) % 4 == 0
            assert plan(v) == (1, 0, 0)
            return v
        return make(b, counts, eb, floor=1, salt=g, top=MAX_POS if b == 14 else None)
    return make(b, counts, eb, floor=1 if side == "d" or b > 1 else 0, salt=g, positions=pos)  # (freqs of width 0 and 1 rest on frequency 0)


def _plain_deltas(n, salt):
    return 1 + (np.arange(n, dtype=np.int64) * 7 + salt) % 5


def _plain_freqs(n, salt):
    return 1 + (np.arange(n, dtype=np.int64) + salt) % 3


def spread_positions(freqs):
    """Positions of documents whose frequency may exceed MaxPosition: 1 .. f while that fits, else f non-decreasing positions from 1 to MAX_POS."""
    out = []
    for f in np.asarray(freqs, dtype=np.int64).tolist():
        k = np.arange(f, dtype=np.int64)
        out.append(1 + k if f <= MAX_POS else 1 + (k * (MAX_POS - 1)) // (f - 1))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def _corpus_lists(which):
    """-> ({name: (docids, freqs)}, {name: positions}) of corpus `which`, partners included."""
    L, P = {}, {}
    salt = 0

    def add(name, dgroups, fgroups):
        nonlocal salt
        salt += 1
        d = np.concatenate(list(dgroups) + [np.array(TAIL_DELTAS)])
        f = np.concatenate(list(fgroups) + [np.array(TAIL_FREQS)])
        L[name] = (np.cumsum(d), f)
        if int(f.max()) > MAX_POS:
            P[name] = spread_positions(f)

    dshapes = [n for n, s in SHAPES.items() if s[0] == "d" and s[1] == which]
    fshapes = [n for n, s in SHAPES.items() if s[0] == "f" and s[1] == which]
    for n in dshapes:
        G = SHAPES[n][5]
        add(n, [shape_group(n, g) for g in range(G)], [_plain_freqs(BLOCK, g + len(L)) for g in range(G)])
    for n in fshapes:
        G = SHAPES[n][5]
        add(n, [_plain_deltas(BLOCK, g + len(L)) for g in range(G)], [shape_group(n, g) for g in range(G)])
    mixed = [n for n in dshapes if n != "d_x_ebmax"] + ([n for n in dshapes if n == "d_x_ebmax"])  # (the 2^25 delta last: the list ends right behind it)
    add("mixed_d", [shape_group(n, 1 if SHAPES[n][5] > 1 else 0) for n in mixed], [_plain_freqs(BLOCK, i) for i in range(len(mixed))])
    if fshapes:
        add("mixed_f", [_plain_deltas(BLOCK, i) for i in range(len(fshapes))], [shape_group(n, 1) for n in fshapes])
    if which == "narrow":
        name, dt, db, ft, fb = BOTH
        add(name, [make(db, EXC[dt][0], EXC[dt][1], salt=g, positions=EXC[dt][2]) for g in range(GROUPS)], [make(fb, EXC[ft][0], EXC[ft][1], salt=g, positions=EXC[ft][2]) for g in range(GROUPS)])
        # ---- hits.data: a stream of position values cut into documents
        first = 100
        for n in [k for k, s in SHAPES.items() if s[0] == "h"] + [STRADDLE[0]]:
            if n == STRADDLE[0]:
                _, wa, wb, at, hits = STRADDLE
                V = np.concatenate([make(wa, salt=3), make(wb, salt=4), np.array([3, 1, 2, 9, 1])])
                F = np.array([1] * at + [hits] + [1] * (V.size - at - hits), dtype=np.int64)
            else:
                V = np.concatenate([shape_group(n, g) for g in range(SHAPES[n][5])] + [np.array([3, 1, 700, 9, 1])])
                F = np.full(V.size // 2, 2, dtype=np.int64) if n == "h_w1" else np.ones(V.size, dtype=np.int64)
                if n == "h_w1":
                    V = V[: 2 * F.size]
            ends = np.cumsum(F)
            assert int(ends[-1]) == V.size
            pos = np.concatenate([np.cumsum(V[e - k : e]) for e, k in zip(ends.tolist(), F.tolist())])
            assert int(pos.max()) <= MAX_POS and int(pos.min()) >= 1, n
            docs = first + 3 * np.arange(F.size, dtype=np.int64)
            first += 1
            L[n], P[n] = (docs, F), pos
            # the phrase partner: one hit a document, right behind the document's first hit on even ranks, two behind on odd ones
            L["n_" + n], P["n_" + n] = (docs, np.ones(F.size, dtype=np.int64)), pos[ends - F] + 1 + (np.arange(F.size) % 2)
    D = D_NARROW if which == "narrow" else D_WIDE
    cat = [n for n in L if not n.startswith("n_")]
    assert all(int(L[n][0][-1]) <= D for n in L), [n for n in L if int(L[n][0][-1]) > D]
    grid = np.arange(2, D + 1, DENSE_STEP[which], dtype=np.int64)
    L["p_dense"] = (np.unique(np.concatenate([grid, [D]] + [L[n][0][::2] for n in cat])), None)
    L["p_sparse"] = (np.unique(np.concatenate([S.spread(500, D).astype(np.int64)] + [L[n][0][1::3] for n in cat])), None)
    for n in ("p_dense", "p_sparse"):
        L[n] = (L[n][0], _plain_freqs(L[n][0].size, 1))
    return L, P


def catalogue(which):
    """The catalogue lists of a corpus (shape lists, mixed lists, x_both, the hits lists): everything but the partners."""
    names = [n for n, s in SHAPES.items() if s[1] == which] + ["mixed_d"]
    return names + (["mixed_f", BOTH[0], STRADDLE[0]] if which == "narrow" else [])


def lists_of(c, which):
    """The catalogue lists and the hits lists' phrase partners: everything but p_dense / p_sparse."""
    return catalogue(which) + [n for n in c.names if n.startswith("n_")]


SCATTER_OPTS = {"plane_div": 64}  # term planes from df >= docs / 64 on: the mixed lists (3 .. 4 K documents) lose theirs too, the partners keep them


def union_queries(which, dense=True):
    """Unions of five catalogue lists; dense: with the dense partner, whose plane makes them k_psets scatter unions (PSET_UNIT_SCATTER) wherever the five have no plane."""
    cat = catalogue(which)
    us = [" OR ".join(f"{{{n}}}" for n in cat[i : i + 5]) for i in range(0, len(cat), 5)]
    return ["{p_dense} OR " + u for u in us] if dense else us


def docs_queries(c, which):
    """For every list L: L, and L p, L OR p, p NOT L with the dense and the sparse partner; the unions of five catalogue lists, without and with the dense partner."""
    out = []
    for n in lists_of(c, which):
        out.append(f"{{{n}}}")
        for p in ("p_dense", "p_sparse"):
            out += [f"{{{n}}} {{{p}}}", f"{{{n}}} OR {{{p}}}", f"{{{p}}} NOT {{{n}}}"]
    out += union_queries(which, False) + union_queries(which, True)
    return [(c.q(t), 1) for t in out]


_made = {}


def corpus(which):
    """structured.Corpus of `narrow` or `wide`, built once per process."""
    if which not in _made:
        L, P = _corpus_lists(which)
        _made[which] = S.build({k: (S._u32(d), np.asarray(f, dtype=np.int64)) for k, (d, f) in L.items()}, positions={k: np.asarray(p, dtype=np.uint16) for k, p in P.items()})
        assert _made[which].D == (D_NARROW if which == "narrow" else D_WIDE)
    return _made[which]


class EncoderCase:
    """A corpus as the write side's encoder cases want it (tests/write_cases.py: .docs / .freqs / .pos / .tf)."""

    def __init__(self, which):
        c = corpus(which)
        self.name, self.upload, self.reaches = f"pfor_{which}", False, set()
        self.docs, self.freqs, self.pos, self.tf = c.docs, c.freqs, c.pos, c.term_first


# ---- reading the headers back out of the encoded bytes --------------------------------------------------------------------------------------------
def _group(b, p):
    """An ints() group at byte p -> (header, bytes): header = ("eq", value) or (b, nexc, eb, [count per quarter], [e0 per quarter], [exception positions])."""
    L = int(b[p])
    if L == 0:
        v, k = S._vb(b, p + 1)
        return ("eq", v), 1 + k
    w0 = int(b[p + 1]) | int(b[p + 2]) << 8 | int(b[p + 3]) << 16 | int(b[p + 4]) << 24
    wb, nexc, eb = w0 & 0xFF, (w0 >> 8) & 0xFF, (w0 >> 16) & 0xFF
    assert L == 1 + 4 * wb + (nexc + 3) // 4 + (nexc * eb + 31) // 32, (L, wb, nexc, eb)
    epos = [int(x) for x in b[p + 5 + 16 * wb : p + 5 + 16 * wb + nexc]]
    assert epos == sorted(set(epos))
    cnt = [sum(1 for x in epos if x >> 5 == q) for q in range(4)]
    e0 = [next((i for i, x in enumerate(epos) if x >> 5 == q), 0) for q in range(4)]
    return (wb, nexc, eb, cnt, e0, epos), 1 + 4 * L


def index_headers(c, t):
    """[(deltas header, freqs header)] of the whole blocks of term t of corpus c, from the host encoder's index bytes."""
    off = int(c.l_terms[t][1])
    p, out = off + 14, []
    for _ in range(int(c.l_terms[t][0]) // BLOCK):
        hd, k = _group(c.l_index, p)
        p += k
        hf, k = _group(c.l_index, p)
        p += k
        out.append((hd, hf))
    return out


def hits_headers(c, t):
    """[positions header] of the whole 128-hit groups of term t, from the host encoder's hits.data bytes (every group is followed by an all-equal group of
    payload lengths 0 and a zero byte count)."""
    off = int(c.l_terms[t][1])
    u32 = lambda a, q: int(a[q]) | int(a[q + 1]) << 8 | int(a[q + 2]) << 16 | int(a[q + 3]) << 24  # noqa: E731
    p, out = u32(c.l_index, off), []
    for _ in range(u32(c.l_index, off + 4) // BLOCK):
        h, k = _group(c.l_hits, p)
        p += k
        hl, k = _group(c.l_hits, p)
        assert hl == ("eq", 0) and int(c.l_hits[p + k]) == 0
        p += k + 1
        out.append(h)
    return out
