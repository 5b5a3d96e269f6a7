"""Structured segments for the read path (a helper module, imported by tests/test_structured.py and tests/test_gpu_structured.py).

The synthetic corpus of csrc/host/synth.cpp is i.i.d.: every list has one density from its first document to its last, so every docID
window looks like every other.  The corpora here are written posting by posting instead, so that documents sit exactly on the kernels'
window boundaries, lists are empty for whole windows, dense lists carry runs of multi-byte deltas, frequencies hit the planes' levels and
the fused fields' caps, and scores rise or fall with the docID.  Everything is generated in-process from the catalogue below.

build() encodes explicit postings with the product's two host encoders (Google: engine.host_encode_google; Lucene:
hostplan.lucene_encode).  evaluate() answers the postfix programs of oracle_lib.parse_query from the postings ARRAYS with numpy set
operations: it never reads an encoded byte, so it is independent of both codecs and of the oracle's decoder.

Deviations from a single catalogue corpus, with their reasons:
  * `dense_tail3` (a dense run of 100 000, then 64 documents more than 16 384 apart) ends past 1.1 M, beyond the main corpus' D; it
    lives in the `tall` corpus.
  * the frequency patterns reach 300 hits a document; applied to `all` of the main corpus they would make half a billion hits.  They
    live in a corpus of their own (`freq`, D = 2 PL_W + 37: three plane windows, five k_fused windows, three 16-bit ones), which keeps
    the CPU file at seconds; the main corpus' lists carry frequencies 1 .. 3.
"""
import re
import os

import numpy as np

import oracle_lib as O

# ---- mirrors of the geometry constants (test_structured.py::test_geometry_mirrors parses the headers and fails when one drifts)
CELL_DOCS = 1024
WIN_MIN_BLOCKS = 128
SPAN_BITS = 131072
PL_W = 32768
FUS_W = 14336
PSET_ROUND_DOCS = 16384
PSET_STAGE_DOCS = 1024
TREE_CHUNK_WORDS = 2048
PL_RANK_DOCS = 256
TILE_BLOCKS = 256
DENSE_SLOW_CAP = 128
PL_STORED = 4
PL_NESTED = 6
PLK_CAP = 512
FUS_CAP = 512
INLINE_MAX = 7
TOPK_MAX = 256
MIRRORS = {"dev_structs.hpp": ["CELL_DOCS", "WIN_MIN_BLOCKS", "SPAN_BITS", "PL_W", "FUS_W", "PSET_ROUND_DOCS", "PSET_STAGE_DOCS", "TREE_CHUNK_WORDS", "PL_RANK_DOCS", "TILE_BLOCKS",
                               "PL_STORED", "PL_NESTED", "TOPK_MAX"],
           "k_match.hpp": ["DENSE_SLOW_CAP"], "k_planes.hpp": ["PLK_CAP"], "k_fused.hpp": ["FUS_CAP"], "k_phrase.hpp": ["INLINE_MAX"]}  # fmt: skip
WINDOWS = [CELL_DOCS, SPAN_BITS, PL_W, FUS_W, 2 * FUS_W, PSET_ROUND_DOCS, PSET_STAGE_DOCS, TREE_CHUNK_WORDS * 32, PL_RANK_DOCS]
TILE_DOCS = TILE_BLOCKS * 32
CSRC = os.path.join(O.ROOT, "trinity_amd", "csrc")


def header_constants(*files):
    """{name: value} of the integer `constexpr` constants and `#define`s of csrc/<files>, in file order (a later file sees the earlier ones' names)."""
    raw = {}
    for f in files:
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        for m in re.finditer(r"#define\s+(\w+)\s+([^\n]+)", text):
            raw.setdefault(m.group(1), m.group(2).strip())
        for m in re.finditer(r"constexpr\s+(?:unsigned\s+)?\w+\s+([^;(){}]+);", text):
            for part in m.group(1).split(","):
                if "=" in part:
                    k, v = part.split("=", 1)
                    raw[k.strip()] = v.strip()
    out = {}

    def value(name, depth=0):
        if name not in out:
            expr = re.sub(r"\b(0x[0-9a-fA-F]+|\d+)(?:[uU][lL]{0,2}|[lL]{1,2}[uU]?)\b", r"\1", raw[name])
            expr = re.sub(r"\(\s*(?:uint\d+_t|int|unsigned)\s*\)", "", expr)
            names = set(re.findall(r"\b[A-Za-z_]\w*\b", expr))
            if depth > 8 or not names <= set(raw) or not re.fullmatch(r"[\w\s+\-*/<>()]+", expr):
                raise KeyError(name)
            out[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, {n: value(n, depth + 1) for n in names}))  # (integer constant expressions of the project's own headers)
        return out[name]

    for k in list(raw):
        try:
            value(k)
        except (KeyError, SyntaxError, TypeError, ValueError, ZeroDivisionError):
            pass
    return out


# ---- encoding explicit postings ----------------------------------------------------------------------------------------------------------
class Corpus:
    """Explicit postings and their two encodings.  lists: {name: (docids, freqs)}; tid: name -> term id (the order of `lists`)."""

    def __init__(self, lists, positions=None, docs_cnt=None):
        from trinity_amd import engine as E
        from trinity_amd import hostplan as HP

        self.names = list(lists)
        self.tid = {n: i for i, n in enumerate(self.names)}
        self.lists = {n: (np.asarray(d, dtype=np.uint32), np.asarray(f, dtype=np.uint32)) for n, (d, f) in lists.items()}
        self.positions = {}
        docs, freqs, pos, tf = [], [], [], [0]
        for n in self.names:
            d, f = self.lists[n]
            assert d.size == f.size and (d.size == 0 or (d[0] >= 1 and np.all(np.diff(d.astype(np.int64)) > 0))), n
            if positions is not None and n in positions:
                p = np.asarray(positions[n], dtype=np.uint16)
            else:  # 1 .. f for every document
                ends = np.cumsum(f.astype(np.int64))
                p = (np.arange(int(ends[-1]) if f.size else 0, dtype=np.int64) - np.repeat(ends - f, f) + 1).astype(np.uint16)
            assert p.size == int(f.sum()), n
            self.positions[n] = p
            docs.append(d)
            freqs.append(f)
            pos.append(p)
            tf.append(tf[-1] + d.size)
        self.docs, self.freqs, self.pos = np.concatenate(docs), np.concatenate(freqs), np.concatenate(pos)
        self.term_first = np.array(tf, dtype=np.uint64)
        self.D = int(self.docs.max())
        self.docs_cnt = int(docs_cnt or self.D)
        self.postings, self.hits = int(self.docs.size), int(self.freqs.sum())
        self.g_index, self.g_terms = E.host_encode_google(self.docs, self.freqs, self.pos, self.term_first)
        self.l_index, self.l_hits, self.l_terms = HP.lucene_encode(self.docs, self.freqs, self.pos, self.term_first)
        self._hitpos = {}

    def q(self, text):
        """A query text over list names — "{all} {odd} NOT {edges}" — as oracle_lib.parse_query reads it."""
        return text.format(**{n: f"t{i}" for n, i in self.tid.items()})

    def oracle(self):
        """The CPU oracle over the GOOGLE bytes (the checker of scores, of the default mode's records and — in the CPU file — of evaluate())."""
        return O.Index.wrap(self.g_index, self.g_terms, self.docs_cnt, self.postings, self.hits)

    def host_index(self, codec):
        from trinity_amd import hostplan as HP

        return HP.HostIndex(self.g_index, self.g_terms, self.docs_cnt) if codec == 1 else HP.HostIndex(self.l_index, self.l_terms, self.docs_cnt, codec=2, hits=self.l_hits)

    def upload(self, T, dev, codec):
        return T.Index(dev, self.g_index, self.g_terms, self.docs_cnt) if codec == 1 else T.Index(dev, self.l_index, self.l_terms, self.docs_cnt, codec=2, hits=self.l_hits)

    def df(self):
        return np.diff(self.term_first.astype(np.int64))

    def doc_positions(self, t):
        """{docid: positions} of term id t."""
        if t not in self._hitpos:
            d, f = self.lists[self.names[t]]
            ends = np.cumsum(f.astype(np.int64))
            p = self.positions[self.names[t]]
            self._hitpos[t] = {int(x): p[int(e - k) : int(e)] for x, e, k in zip(d, ends, f)}
        return self._hitpos[t]

    # ---- the codec-independent reference --------------------------------------------------------------------------------------------------
    def evaluate(self, prog, masked=None):
        """The ascending docIDs a postfix program (oracle_lib.parse_query) matches, from the postings arrays alone."""
        st = []
        none = np.zeros(0, dtype=np.uint32)
        for w in np.asarray(prog, dtype=np.uint32).tolist():
            op, arg = w >> 28, w & 0x0FFFFFFF
            if op == O.OP_TERM:
                st.append(("T", arg, self.lists[self.names[arg]][0] if arg < len(self.names) else none))
                continue
            n = arg & 0xFFFF if op == O.OP_SOME else arg
            kids = st[-n:]
            del st[-n:]
            sets = [k[2] for k in kids]
            if op == O.OP_AND:
                r = sets[0]
                for s in sets[1:]:
                    r = np.intersect1d(r, s, assume_unique=True)
            elif op == O.OP_OR:
                r = sets[0]
                for s in sets[1:]:
                    r = np.union1d(r, s)
            elif op == O.OP_NOT:
                r = np.setdiff1d(sets[0], sets[1], assume_unique=True)
            elif op == O.OP_OPT:
                r = sets[0]
            elif op == O.OP_SOME:
                allv, cnt = np.unique(np.concatenate(sets), return_counts=True)
                r = allv[cnt >= (arg >> 16)]
            elif op == O.OP_PHRASE:
                assert all(k[0] == "T" for k in kids)
                r = self._phrase([k[1] for k in kids], sets)
            else:
                raise ValueError(op)
            st.append(("N", None, r.astype(np.uint32)))
        assert len(st) == 1
        r = st[0][2]
        if masked is not None and len(masked):
            r = r[~np.isin(r, masked)]
        return r

    def _phrase(self, terms, sets):
        """Consecutive positions, as the reference's DocWordsSpace holds a document: ONE term per position — the phrase's distinct terms are written in phrase
        order, a later one replaces an earlier one at the same position (docwordspace.h) —, a start at every hit p > 0 of the first term with term k at p + k."""
        cand = sets[0]
        for s in sets[1:]:
            cand = np.intersect1d(cand, s, assume_unique=True)
        out = []
        for d in cand.tolist():
            space = {}
            for i, t in enumerate(terms):
                if t in terms[:i]:
                    continue
                for p in self.doc_positions(t)[d].tolist():
                    if p:
                        space[p] = t
            if any(p and all(space.get(p + k) == terms[k] for k in range(1, len(terms))) for p in self.doc_positions(terms[0])[d].tolist()):
                out.append(d)
        return np.array(out, dtype=np.uint32)


def build(lists, positions=None, docs_cnt=None):
    return Corpus(lists, positions, docs_cnt)


# ---- the GOOGLE chunk as the upload walks it (index_host.hpp) ---------------------------------------------------------------------------------
def _vb(b, p):
    x = int(b[p])
    if x < 0x80:
        return x, 1
    if x < 0xC0:
        return ((x & 0x3F) << 8) | int(b[p + 1]), 2
    if x < 0xE0:
        return ((x & 0x1F) << 16) | int(b[p + 1]) | (int(b[p + 2]) << 8), 3
    if x < 0xF0:
        return ((x & 0x0F) << 24) | (int(b[p + 1]) << 16) | (int(b[p + 2]) << 8) | int(b[p + 3]), 4
    return int(b[p + 1]) | (int(b[p + 2]) << 8) | (int(b[p + 3]) << 16) | (int(b[p + 4]) << 24), 5


def google_blocks(index, terms, t):
    """[(last docID, documents, bytes of the interior deltas, longest interior delta in bytes)] of term t's blocks, read from the encoded chunk."""
    off, size = int(terms[t][1]), int(terms[t][2])
    b = index
    sk = int(b[off]) | (int(b[off + 1]) << 8)
    p, end = off + 2, off + size - 8 * sk
    last, out = 0, []
    while p != end:
        delta, k = _vb(b, p)
        p += k
        blen, k = _vb(b, p)
        p += k
        n = int(b[p])
        p += 1
        s, nbytes, longest = p, 0, 0
        for _ in range(n - 1):
            _, k = _vb(b, s)
            s += k
            nbytes += k
            longest = max(longest, k)
        last += delta
        out.append((last, n, nbytes, longest))
        p += blen
    return out


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
D_MAIN = 4 * SPAN_BITS + 37
DF_EDGES = [31, 32, 33, 127, 128, 129, 32 * (WIN_MIN_BLOCKS - 1), 32 * (WIN_MIN_BLOCKS - 1) + 1, 32 * WIN_MIN_BLOCKS, 32 * WIN_MIN_BLOCKS + 1, TILE_DOCS - 1, TILE_DOCS, TILE_DOCS + 1, 3 * TILE_DOCS + 1]
assert DF_EDGES[6:10] == [4064, 4065, 4096, 4097]


def _u32(x):
    return np.unique(np.asarray(x, dtype=np.int64)).astype(np.uint32)


def spread(df, D):
    """df documents from 1 to D, evenly."""
    return _u32([D // 2]) if df == 1 else _u32(1 + (np.arange(df, dtype=np.int64) * (D - 1)) // (df - 1))


def main_docids(D=D_MAIN):
    rng = np.random.default_rng(20240607)
    ar = np.arange(1, D + 1, dtype=np.int64)
    B = np.unique(np.concatenate([np.arange(w, D + 2, w, dtype=np.int64) for w in WINDOWS]))
    edges = np.concatenate([B - 1, B, B + 1, [1, 2, 31, 32, 33, 63, 64, 65, D - 1, D]])
    L = {}
    L["all"] = ar
    L["odd"] = ar[ar % 2 == 1]
    L["every32"] = ar[ar % 32 == 0]
    L["every33"] = ar[ar % 33 == 0]
    L["edges"] = edges[(edges >= 1) & (edges <= D)]
    L["runs"] = np.concatenate([np.arange(s, min(s + 200, D + 1)) for s in range(5, D, 7001)])
    L["lastwin"] = ar[(ar > 3 * SPAN_BITS) & (ar % 3 == 0)]  # the last whole SPAN_BITS window and the 37 documents after it
    L["stub"] = ar[ar >= 4 * SPAN_BITS]  # ... only those
    L["firstwin"] = ar[(ar < SPAN_BITS) & (ar % 3 == 1)]
    L["midwin"] = ar[(ar >= 2 * SPAN_BITS) & (ar < 3 * SPAN_BITS) & (ar % 2 == 0)]
    L["holes"] = ar[((ar < SPAN_BITS) & (ar % 2 == 0)) | (ar >= 4 * SPAN_BITS)]  # windows 1, 2 and 3 hold nothing
    L["first1"] = [1]
    L["last1"] = [D]
    # dense on average (1250 full blocks of one-byte deltas), then 300 blocks inside window 1 that each hold one two-byte delta
    slow = SPAN_BITS + 10 + np.cumsum(np.where(np.arange(300 * 32) % 32 == 5, 200, 1))
    assert slow[-1] < 2 * SPAN_BITS
    L["dense_many_slow"] = np.concatenate([np.arange(1, 40001), slow])
    L["sparse_runs"] = np.concatenate([np.arange(s, min(s + 40, D + 1)) for s in range(900, D, 2000)])
    for df in DF_EDGES:
        L[f"df{df}"] = spread(df, D)
    # either side of the TERM_SPARSE rule  documents * 28 < last document  (index_host.hpp), both ending on D
    lo = D // 28 if (D // 28) * 28 < D else D // 28 - 1
    L["sp_lo"], L["sp_hi"] = spread(lo, D), spread(lo + 1, D)
    assert lo * 28 < D <= (lo + 1) * 28
    L["rnd3"] = np.sort(rng.choice(ar, D // 3, replace=False))
    L["rnd10"] = np.sort(rng.choice(ar, D // 10, replace=False))
    return {k: _u32(v) for k, v in L.items()}


def main_corpus(docs_cnt=None):
    """D = 4 SPAN_BITS + 37; frequencies 1 .. 3 by rank in the list."""
    return build({k: (d, 1 + (np.arange(d.size) % 3)) for k, d in main_docids().items()}, docs_cnt=docs_cnt)


MAIN_PAIR_LISTS = ["all", "odd", "edges", "runs", "lastwin", "firstwin", "holes", "last1", "dense_many_slow", "sparse_runs", "sp_lo", "df4065"]
TEMPLATES = ["{a} OR {b}", "{a} OR {b} OR {c} OR {d} OR {e}", "{a} {b} ({c} OR {d} OR {e})", "({a} OR {b}) ({c} OR {d}) {e}", "{a} ({b} OR {c})", "({a} OR {b}) ({c} OR {d})"]  # (test_gpu_parity.TEMPLATES over names)
OPT_TEMPLATES = ["{a} <{b}>", "{a} {b} <{c} OR {d}>", "{a} <{c}> {b}", "({a} OR {b}) <{c}>", "{a} <{a}>", "({a} {b} NOT {e}) <{c}>"]
MAIN_ROWS = [("all", "odd", "edges", "runs", "lastwin"), ("edges", "all", "firstwin", "holes", "stub"), ("rnd3", "rnd10", "every32", "every33", "sparse_runs"),
             ("dense_many_slow", "odd", "sp_lo", "sp_hi", "midwin"), ("df8192", "df8193", "df24577", "all", "first1"), ("lastwin", "stub", "last1", "holes", "df4064"),
             ("odd", "rnd3", "all", "dense_many_slow", "edges")]  # fmt: skip
SOME_ROWS = [("all", "odd", "edges"), ("lastwin", "firstwin", "holes"), ("rnd3", "rnd10", "runs"), ("dense_many_slow", "sparse_runs", "every32"), ("first1", "last1", "stub")]
NINE = "{all} OR ({odd} {edges}) OR ({runs} {lastwin}) OR ({firstwin} {holes}) OR ({rnd3} {rnd10})"  # a tree over nine terms: TASK_TREE


def main_queries(c):
    """[(text over term ids, some_min)] — every ordered pair of MAIN_PAIR_LISTS as AND / OR / NOT, triples and CNFs, optional forms, matchsome at 1 .. 3."""
    out = []
    for a in MAIN_PAIR_LISTS:
        for b in MAIN_PAIR_LISTS:
            if a != b:
                out += [(c.q(f"{{{a}}} {{{b}}}"), 1), (c.q(f"{{{a}}} OR {{{b}}}"), 1), (c.q(f"{{{a}}} NOT {{{b}}}"), 1)]
    out += [(c.q(f"{{{n}}}"), 1) for n in c.names]
    for df in DF_EDGES:  # the df-boundary lists as leads (31 .. 33 documents, the cell index's edge, one / two / four candidate tiles) and as the probed side
        n = f"{{df{df}}}"
        out += [(c.q(t), 1) for t in (f"{n} {{all}}", f"{n} {{odd}}", f"{n} {{edges}}", f"{{all}} NOT {n}", f"{n} OR {{edges}}", f"{n} {{sp_hi}}")]
    for row in MAIN_ROWS:
        names = {k: "{" + v + "}" for k, v in zip("abcde", row)}
        out += [(c.q(tpl.format(**names)), 1) for tpl in TEMPLATES + OPT_TEMPLATES]
    for row in SOME_ROWS:
        out += [(c.q("[{%s}, {%s}, {%s}]" % row), mn) for mn in (1, 2, 3)]
    out += [(c.q(NINE), 1), (c.q("{edges} NOT ({all} {odd})"), 1), (c.q("{lastwin} OR ({all} {edges})"), 1)]
    return out


def programs(queries):
    return [O.parse_query(t, some_min=mn) for t, mn in queries]


# ---- frequencies --------------------------------------------------------------------------------------------------------------------------
D_FREQ = 2 * PL_W + 37
FREQ_CYCLE = [0, 1, 2, 3, 4, 5, 6, 7, 13, 14, 15, 16, 29, 30, 31, 32, 253, 254, 255, 256, 300]
K_VALUES = (1, 10, 255, 256)


def freq_corpus():
    """Bases `all`, `odd`, `third` (1 in 3) of D = 2 PL_W + 37 under five frequency patterns — `cyc`: FREQ_CYCLE by rank (f = 0, the plane levels PL_STORED / PL_NESTED,
    the fused fields' caps 6 / 14 / 30 / 254 and their neighbours, 300); `one`: constant 1 (every document ties); `rise`: one more every CELL_DOCS documents (the score
    rises with the docID: every window's documents beat the running threshold); `fall`: the same falling; `last3`: 1 everywhere, 7 / 30 / 300 on the last three documents
    (the K best sit at the end of the last task) — and lists of K - 1, K, K + 1 documents for the K of the top-K runs."""
    D = D_FREQ
    ar = np.arange(1, D + 1, dtype=np.int64)
    bases = {"all": ar, "odd": ar[ar % 2 == 1], "third": ar[ar % 3 == 0]}
    L = {}
    for bn, d in bases.items():
        rank = np.arange(d.size)
        L[f"{bn}_cyc"] = (d, np.array(FREQ_CYCLE)[rank % len(FREQ_CYCLE)])
        L[f"{bn}_one"] = (d, np.ones(d.size, dtype=np.int64))
        L[f"{bn}_rise"] = (d, np.minimum(1 + d // CELL_DOCS, 300))
        L[f"{bn}_fall"] = (d, np.minimum(1 + (D - d) // CELL_DOCS, 300))
        f = np.ones(d.size, dtype=np.int64)
        f[-3:] = [7, 30, 300]
        L[f"{bn}_last3"] = (d, f)
    for n in sorted({k + s for k in K_VALUES for s in (-1, 0, 1)} - {0}):
        d = spread(n, D)
        L[f"n{n}"] = (d, 1 + (np.arange(n) * 7) % 5)
    return build({k: (_u32(d), f) for k, (d, f) in L.items()})


FREQ_PATTERNS = ["cyc", "one", "rise", "fall", "last3"]


def freq_queries(c):
    out = []
    for p in FREQ_PATTERNS:
        a, o, t = f"{{all_{p}}}", f"{{odd_{p}}}", f"{{third_{p}}}"
        out += [a, o, t, f"{a} {o}", f"{o} {t}", f"{a} OR {t}", f"{o} OR {t}", f"{a} {o} {t}", f"{a} NOT {t}", f"{o} <{t}>", f"{a} ({o} OR {t})", f"({a} OR {o}) NOT {t}", f"{t} {t}"]
    out += ["{all_cyc} {odd_rise}", "{all_cyc} OR {third_fall}", "{odd_cyc} {third_last3}", "{all_rise} OR {odd_fall} OR {third_cyc}", "{all_one} {odd_cyc} ({third_rise} OR {third_fall})",
            "{all_cyc} {odd_cyc} {third_cyc} {all_one} {odd_one}", "{all_cyc} OR {odd_cyc} OR {third_cyc} OR {all_rise} OR {odd_fall} OR {third_last3}",
            "({all_cyc} OR {n255}) ({odd_rise} OR {n256})", "{third_cyc} <{all_rise} OR {n10}>", "{all_last3} {n257}", "{all_rise} {n11}"]  # fmt: skip
    out += [f"{{n{n}}}" for n in sorted({k + s for k in K_VALUES for s in (-1, 0, 1)} - {0})]
    return [(c.q(t), 1) for t in out]


def tie_queries(c):
    """Queries over the constant-1 lists only: every match of a query scores the same under every similarity."""
    return [(c.q(t), 1) for t in ["{all_one}", "{odd_one}", "{all_one} {odd_one}", "{odd_one} {third_one}", "{all_one} {odd_one} {third_one}", "{all_one} NOT {third_one}"]]


# ---- tall ---------------------------------------------------------------------------------------------------------------------------------
D_TALL = (1 << 21) + (1 << 17) + 5


def tall_corpus():
    """D = 2^21 + 2^17 + 5: gaps that need a three- and a four-byte delta (prefix varint: >= 2^14, >= 2^21), a list that lives beyond 2^21 only, and `dense_tail3`:
    not TERM_SPARSE on average, its last two blocks hold 31 three-byte deltas each (93 bytes: past the 64 the cooperative block decoder looks at)."""
    D = D_TALL
    ar = np.arange(1, D + 1, dtype=np.int64)
    L = {}
    L["dense_tail3"] = np.concatenate([np.arange(1, 100001), 100000 + 16400 * np.arange(1, 65)])
    L["gap4_a"] = np.concatenate([np.arange(1, 65), (1 << 21) + 70 + np.arange(0, 64)])  # one four-byte gap in the middle of a list
    L["gap4_b"] = [3, (1 << 21) + 4, D]
    L["gap4_c"] = np.concatenate([np.arange(10, 1000, 3), (1 << 21) + 1330 + np.arange(0, 5000, 2)])
    L["beyond"] = ar[(ar > (1 << 21)) & (ar % 2 == 0)]
    L["tall_odd"] = ar[ar % 2 == 1]
    L["tall_33"] = ar[ar % 33 == 0]
    L["tall_edges"] = np.concatenate([[b - 1, b, b + 1] for b in range(SPAN_BITS, D, SPAN_BITS)] + [[1, D]])
    return build({k: (_u32(v), 1 + (np.arange(len(_u32(v))) % 4)) for k, v in L.items()})


def tall_queries(c):
    out = [f"{{{n}}}" for n in c.names]
    for a in c.names:
        for b in c.names:
            if a != b:
                out += [f"{{{a}}} {{{b}}}", f"{{{a}}} OR {{{b}}}", f"{{{a}}} NOT {{{b}}}"]
    return [(c.q(t), 1) for t in out]


TALL_SCORED = "{dense_tail3} OR {beyond} OR {gap4_c} OR {tall_33}"


# ---- phrases ------------------------------------------------------------------------------------------------------------------------------
PHRASE_STARTS = [1, 62, 63, 64, 65, 127, 128, 65533, 65534]


def phrase_corpus():
    """Terms a, b, c over 400 documents (and `pad`, in all of them).  Document by document the positions are written so that "a b" / "a b c" start exactly at
    PHRASE_STARTS, or just miss — a gap of 2, the same position (the later term of the phrase owns it), reversed order —, with repeated positions, and with
    frequencies 6, 7, 8 and 70 around k_phrase's INLINE_MAX."""
    docs = {n: [] for n in "abc"}
    pos = {n: [] for n in "abc"}

    def doc(d, **hits):
        for n, p in hits.items():
            docs[n].append(d)
            pos[n].append(sorted(p))

    d = 3
    for s in PHRASE_STARTS:  # exact starts: two terms, then three (a three-term phrase starts at most at 65533)
        doc(d, a=[s], b=[s + 1])
        d += 37
        if s + 2 <= 65535:
            doc(d, a=[s], b=[s + 1], c=[s + 2])
            d += 37
    for s in (1, 63, 64, 127, 8000):  # near misses
        doc(d, a=[s], b=[s + 2])  # a gap of 2
        doc(d + 1, a=[s + 1], b=[s + 1])  # the same position
        doc(d + 2, a=[s + 1], b=[s])  # reversed
        doc(d + 3, a=[s], b=[s + 1], c=[s + 3])  # "a b" but not "a b c"
        doc(d + 4, a=[s], b=[s + 1], c=[s + 1, s + 2])  # inside "a b c", c takes b's position: "a b" matches, "a b c" does not ...
        doc(d + 5, a=[s, s + 10], b=[s + 1, s + 11], c=[s + 1, s + 12])  # ... here the second start of "a b c" survives
        d += 1024
    for f in (6, 7, 8, 70):  # frequencies around INLINE_MAX; the match is the LAST hit of a
        base = [5 * k + 200 for k in range(f)]
        doc(d, a=base, b=[base[-1] + 1] + [9000 + 3 * k for k in range(f - 1)], c=[base[-1] + 2])
        doc(d + 1, a=base, b=[x + 2 for x in base])  # no match at any of the f hits
        doc(d + 2, a=base + base[:2], b=[base[0] + 1])  # repeated positions (f + 2 hits)
        doc(d + 3, a=[100], b=[p for p in range(300, 300 + 3 * f, 3)] + [101])
        d += 300
    doc(d, a=[7])
    doc(d + 1, b=[8])
    doc(d + 2, c=[9])
    D = d + 5
    lists = {n: (docs[n], [len(p) for p in pos[n]]) for n in "abc"}
    positions = {n: np.array([x for p in pos[n] for x in p], dtype=np.uint16) for n in "abc"}
    lists["pad"] = (np.arange(1, D + 1), np.ones(D, dtype=np.int64))
    return build({k: (_u32(dd), np.asarray(ff, dtype=np.int64)) for k, (dd, ff) in lists.items()}, positions=positions)


def phrase_queries(c):
    out = ['"{a} {b}"', '"{a} {b} {c}"', '"{b} {a}"', '"{b} {c}"', '"{a} {c}"', '"{a} {b}" {c}', '"{a} {b}" {pad}', '"{a} {a}"', '"{a} {b} {a}"', '"{c} {b} {a}"', '{pad} NOT "{a} {b}"',
           '"{a} {b}" OR "{b} {c}"', '{c} OR "{a} {b}"', '"{a} {b}" "{b} {c}"', '"{a} {b}" <{c}>', '"{pad} {a}"', '"{a} {pad}"']  # fmt: skip
    return [(c.q(t), 1) for t in out]


# ---- a stream of batches over one index (tests/test_gpu_stream.py) ---------------------------------------------------------------------------
D_STREAM = 2 * SPAN_BITS + 37
STREAM_STEPS = [2, 3, 5, 7, 11, 17, 29, 47, 79, 113, 157, 199]  # h_i: every STREAM_STEPS[i]-th document and the boundary documents — D / 2 .. D / 199, pairwise distinct
STREAM_EDGES = [SPAN_BITS - 1, SPAN_BITS, SPAN_BITS + 1, 2 * SPAN_BITS, D_STREAM]
STREAM_HEADS = [f"h{i}" for i in range(len(STREAM_STEPS))]
STREAM_PHRASE_HEADS = STREAM_HEADS[:6]  # the terms with written positions: df ranks 0 .. 5
STREAM_RARE = {"r0": 5, "r1": 37, "r2": 200}  # fewer than D / 1024 documents: no plane under the default plane_div either, df ranks 12 .. 14
STREAM_PHRASE_STRIDE = 7
STREAM_PHRASE_SHIFTS = [0, 0, 0, 0, 0, 1, 2, 6]  # (a document's shift for a term: 0 five times in eight)


def stream_corpus():
    """D = 2 SPAN_BITS + 37 (three windows).  Head terms h0 .. h11 of pairwise distinct document frequencies D / 2 .. D / 199 — a plane row is the term's df rank, so
    h_i's row is i —, each with documents in every window and on SPAN_BITS - 1, SPAN_BITS, SPAN_BITS + 1, 2 SPAN_BITS and D; frequencies FREQ_CYCLE by rank in the list (a row's
    nested planes and level words differ from its plane 0).  h0 .. h5 carry written positions: hit k of h_i in a document sits at 1 + i + shift + 7 k, shift one of 0 (five
    times in eight), 1, 2, 6 by a hash of (document, term) — "h_i h_i+1" starts exactly where both shifts agree, and misses by the same position (shift 1 against 0: the later
    term of the phrase owns it), reversed order (2 against 0) or a gap of 2 (6 against 0); frequencies 0, 5, 6, 7, 13 lie around k_phrase's INLINE_MAX.  Rare terms r0 .. r2 (5,
    37 and 200 documents) never get a plane."""
    D = D_STREAM
    ar = np.arange(1, D + 1, dtype=np.int64)
    lists, positions = {}, {}
    for i, (n, step) in enumerate(zip(STREAM_HEADS, STREAM_STEPS)):
        d = _u32(np.concatenate([ar[ar % step == i % step], STREAM_EDGES]))
        f = np.array(FREQ_CYCLE, dtype=np.int64)[(np.arange(d.size) + 3 * i) % len(FREQ_CYCLE)]
        lists[n] = (d, f)
        if n in STREAM_PHRASE_HEADS:
            h = ((d.astype(np.uint64) * np.uint64(2654435761) + np.uint64(40503 * (i + 1))) >> np.uint64(13)) & np.uint64(7)
            first = 1 + i + np.array(STREAM_PHRASE_SHIFTS, dtype=np.int64)[h.astype(np.int64)]
            ends = np.cumsum(f)
            k = np.arange(int(ends[-1]), dtype=np.int64) - np.repeat(ends - f, f)
            positions[n] = (np.repeat(first, f) + STREAM_PHRASE_STRIDE * k).astype(np.uint16)
    for j, (n, df) in enumerate(STREAM_RARE.items()):
        d = _u32(STREAM_EDGES) if df == len(STREAM_EDGES) else _u32(np.concatenate([spread(df - len(STREAM_EDGES), D - 3) + 1, STREAM_EDGES]))
        lists[n] = (d, 1 + (np.arange(d.size) * 5 + j) % 9)
    c = build(lists, positions=positions)
    df = c.df()
    assert c.D == D and np.all(np.diff(df[: len(STREAM_HEADS)]) < 0) and int(df[len(STREAM_HEADS) - 1]) > 1024 > D // 1024 > int(df[len(STREAM_HEADS) :].max()), df
    return c


def _stream_shapes(names):
    """ANDs, unions and CNFs over the head terms `names` (in df order) and the rare terms: ONE list, from which the docs-only, scored and phrase tables are all derived."""
    n = len(names)
    out = []
    for i in range(n):
        a, b, c = (f"{{{names[(i + k) % n]}}}" for k in range(3))
        out += [f"{a} {b}", f"{a} OR {b}", f"{a} ({b} OR {c})"]
    a, b = f"{{{names[0]}}}", f"{{{names[-1]}}}"
    out += [f"{a} {{r2}}", f"{b} OR {{r1}}", f"({a} OR {{r0}}) {b}", " OR ".join(f"{{{x}}}" for x in names[:5])]
    return out


def stream_docs_queries(c, names=STREAM_HEADS):
    """DocumentsOnly: every head term of `names` in an AND, a union and a CNF with its neighbours in df order; head terms with rare ones."""
    return [(c.q(t), 1) for t in _stream_shapes(list(names))]


def stream_scored_queries(c, names=STREAM_HEADS):
    """The same shapes, scored (run at K = 10 and 256)."""
    return stream_docs_queries(c, names)


def stream_phrase_queries(c, names=STREAM_PHRASE_HEADS):
    """Phrases over the heads with written positions among `names`: "h_i h_j" of neighbours in df order, "h_i h_j h_k", a phrase and a term, a phrase or a phrase."""
    ph = [x for x in names if x in STREAM_PHRASE_HEADS]
    out = []
    for i in range(len(ph) - 1):
        out += [f'"{{{ph[i]}}} {{{ph[i + 1]}}}"'] + ([f'"{{{ph[i + 1]}}} {{{ph[i]}}}"'] if i % 2 else [])  # (the reversed order for every other pair: numpy's phrase check is slow)
    for i in range(len(ph) - 2):
        out += [f'"{{{ph[i]}}} {{{ph[i + 1]}}} {{{ph[i + 2]}}}"']
    out += [f'"{{{ph[-2]}}} {{{ph[-1]}}}" {{r2}}']
    if len(ph) >= 3:
        out += [f'"{{{ph[1]}}} {{{ph[2]}}}" {{{ph[0]}}}']
    if len(ph) >= 4:
        out += [f'"{{{ph[-4]}}} {{{ph[-3]}}}" OR "{{{ph[-2]}}} {{{ph[-1]}}}"']
    return [(c.q(t), 1) for t in out]


def stream_queries(c):
    return stream_docs_queries(c) + stream_phrase_queries(c)


# ---- the scored cases (shared by the CPU file's score-gap condition and the GPU file) --------------------------------------------------------
MAIN_SCORED_LISTS = ["all", "edges", "lastwin", "holes", "dense_many_slow", "sparse_runs", "df4065", "last1"]


def main_scored_queries(c):
    out = []
    for row in MAIN_ROWS:
        names = {k: "{" + v + "}" for k, v in zip("abcde", row)}
        out += [tpl.format(**names) for tpl in TEMPLATES + OPT_TEMPLATES]
    for a in MAIN_SCORED_LISTS:
        for b in MAIN_SCORED_LISTS:
            if a < b:
                out += [f"{{{a}}} {{{b}}}", f"{{{a}}} OR {{{b}}}", f"{{{b}}} NOT {{{a}}}"]
    out += [f"{{{n}}}" for n in ("edges", "lastwin", "stub", "df31", "df129", "df8193")]
    return [(c.q(t), 1) for t in out] + [(c.q("[{%s}, {%s}, {%s}]" % SOME_ROWS[0]), 2), (c.q(NINE), 1)]


def tall_scored_queries(c):
    return [(c.q(t), 1) for t in [TALL_SCORED, "{beyond} {tall_33}", "{dense_tail3} {tall_odd}", "{gap4_a} OR {gap4_b}", "{tall_edges} OR {gap4_c}", "{beyond}"]]


SCORED_CASES = {"freq": (freq_queries, K_VALUES), "main": (main_scored_queries, (10, 256)), "tall": (tall_scored_queries, (10,)), "phrase": (phrase_queries, (10, 256)),
                "stream": (stream_queries, (10, 256))}
CORPORA = {"main": main_corpus, "freq": freq_corpus, "tall": tall_corpus, "phrase": phrase_corpus, "stream": stream_corpus}
QUERIES = {"main": main_queries, "freq": freq_queries, "tall": tall_queries, "phrase": phrase_queries, "stream": stream_queries}

ALL_PLANES = 1 << 30
# DocumentsOnly option sets (planner options, tri_dev_set_option) and the task kinds each is meant to put queries of the main corpus on
DOCS_OPTION_SETS = [({}, ("n_cand", "n_pset", "n_dense")), ({"dense_min_postings": 0}, ("n_pset", "n_dense")), ({"dense_min_postings": 0, "planes": 0}, ("n_dense",)),
                    ({"plane_div": ALL_PLANES}, ("n_pset", "n_cand")), ({"planes": 0}, ("n_dense", "n_cand")), ({"result_bitmaps": 0}, ("n_dense", "n_pset", "n_cand")),
                    ({"cand_xcd": 0}, ("n_cand",))]  # fmt: skip
# AccumulatedScore top-K: one representative per kernel variant (test_gpu_parity.test_fused_scored_windows_match_oracle's sweep, reduced)
SCORED_OPTION_SETS = [({}, ("n_planes", "n_cand")),
                      ({"dense_min_postings": 0}, ("n_planes", "n_planes8")), ({"dense_min_postings": 0, "plane_div": ALL_PLANES}, ("n_planes", "n_planes8")),
                      ({"dense_min_postings": 0, "plane_div": 0}, ("n_planes", "n_planes8")),
                      ({"dense_min_postings": 0, "planes_split": 1}, ("n_planes",)), ({"dense_min_postings": 0, "planes_split": 7}, ("n_planes",)),
                      ({"dense_min_postings": 0, "planes": 0}, ("n_fused16",)), ({"dense_min_postings": 0, "planes": 0, "fused_halfwords": 0}, ("n_fused",)),
                      ({"dense_min_postings": 0, "fused": 0}, ("n_pset", "n_cand"))]  # fmt: skip


# ---- comparing top-K lists ----------------------------------------------------------------------------------------------------------------
RTOL = 1e-5


def score_gaps(scores, k):
    """The oracle's scores of ranks 1 .. K + 1 -> (exact, smallest relative gap): exact when all DISTINCT scores among them differ by more than RTOL."""
    s = np.unique(np.sort(np.asarray(scores, dtype=np.float64))[::-1][: k + 1])
    if s.size < 2:
        return True, np.inf
    gap = float(np.min(np.diff(s) / np.maximum(np.abs(s[1:]), 1e-300)))
    return gap > RTOL, gap


def check_topk(got_docs, got_scores, docs, scores, k, ora, tag):
    """One query's top-K against the oracle's (docs, scores): scores position by position at rtol 1e-5, docIDs exactly — or, where distinct oracle scores within ranks
    1 .. K + 1 lie within the tolerance of each other, as sets per group of scores within tolerance.  Returns True when the set-wise rule was used."""
    td, ts = ora.topk(docs, scores, k)
    assert len(got_docs) == len(td), (tag, len(got_docs), len(td))
    np.testing.assert_allclose(got_scores, ts, rtol=RTOL, atol=0, err_msg=str(tag))
    exact, _ = score_gaps(scores, k)
    if exact:
        assert got_docs.tolist() == td.tolist(), tag
        return False
    # groups of scores within tolerance (chained); the last group may be cut by K: there the got documents must come from the oracle's whole group
    full = np.asarray(scores, dtype=np.float64)
    at = 0
    while at < len(td):
        end = at + 1
        while end < len(td) and abs(float(ts[end - 1]) - float(ts[end])) <= RTOL * abs(float(ts[end])):
            end += 1
        if end < len(td):
            assert sorted(got_docs[at:end].tolist()) == sorted(td[at:end].tolist()), (tag, at, end)
        else:
            lo = float(ts[end - 1]) * (1 - RTOL) if ts[end - 1] >= 0 else float(ts[end - 1]) * (1 + RTOL)
            group = set(np.asarray(docs)[(full >= lo) & (full <= float(ts[at]) * (1 + RTOL) + 0.0)].tolist())
            assert set(got_docs[at:end].tolist()) <= group and len(set(got_docs[at:end].tolist())) == end - at, (tag, at, end)
        at = end
    return True


# ---- the default ("rich match") mode and the mixed delivery -------------------------------------------------------------------------------------
def rich_freq_queries(c):
    """Small result sets over the frequency cycle: matched terms with frequencies 0 and 300 among them."""
    out = [("{n255} {all_cyc}", 1), ("{n256} OR {n10}", 1), ("{n11} {odd_cyc} <{all_rise}>", 1), ("{n257} NOT {third_cyc}", 1), ("{n254} {all_cyc} {all_fall}", 1), ("[{n255}, {n256}, {n257}]", 2),
           ("{n9} ({all_cyc} OR {third_last3})", 1), ("{n2} {all_cyc}", 1)]  # fmt: skip
    return [(c.q(t), mn) for t, mn in out]


def mixed_queries(c):
    """Main corpus: results held as ascending docIDs whose counts are 1, 2, 3 (mod 4), each directly before a result held as a bitmap — the bitmap's words then start
    at a word offset of the one-call delivery that is not a multiple of four."""
    out = ["{df33}", "{all} OR {odd}", "{first1} OR {last1}", "{all} {odd}", "{df31}", "{all} OR {edges}", "{df129}", "{odd} OR {holes}", "{df127}", "{all} NOT {lastwin}"]
    return [(c.q(t), 1) for t in out]


# ---- the walk k_score and k_rich share (a term's blocks against a tile of matches) ---------------------------------------------------------------------------------------------
D_WALK = 8192 + 37
WALK_FEW = [5, 6, 40, D_WALK - 5, D_WALK - 2]  # by rank in `all` (docIDs start at 1): 5 and 6 share block 0; D - 5 is the last document of the last full block, D - 2 lies in the short block after it


def walk_corpus():
    """`all` (every docID of D = 8192 + 37: 258 blocks, the last one short), `third` (every third), `few` (five documents); frequencies cycle 1, 2, 3 by rank and
    the positions are written (1 .. f).  Not in CORPORA: two queries, for tests/test_gpu_match_walk.py alone."""
    ar = np.arange(1, D_WALK + 1, dtype=np.int64)
    L = {"all": ar, "third": ar[ar % 3 == 0], "few": np.array(WALK_FEW, dtype=np.int64)}
    return build({k: (_u32(d), 1 + np.arange(d.size) % 3) for k, d in L.items()})


def walk_queries(c):
    """`few AND all`: 5 matches against 258 blocks in range — match-driven; `all AND third`: 2 743 matches (two tiles of k_rich's 2048) against no more blocks
    than matches — block-driven."""
    return [(c.q("{few} {all}"), 1), (c.q("{all} {third}"), 1)]
