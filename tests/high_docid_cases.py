"""Segments whose docIDs lie between 2^31 and the top of u32 (a helper module, imported by tests/test_high_docid_cases.py and tests/test_gpu_high_docid.py; no
engine code).

docid_t is 32 bits and any ascending docIDs are legal; the upload refuses only deltas that run past 2^32.  Every other corpus of the suite ends at or below
2^26 + 37.  shifted() moves a small base corpus — a few thousand postings, three bitmap windows — up so that its largest docID is exactly `top`; the tops are the
places where 32-bit arithmetic over docIDs changes its answer (the table in DESIGN.md §36).

Nothing here allocates an array indexed by docID: the references are Corpus.evaluate (numpy set algebra over the postings arrays), the C oracle over the
encoded bytes, and positions cut from the input arrays."""
import os
import re

import numpy as np

import structured as S

SPAN = S.SPAN_BITS
_K = S.header_constants("dev_structs.hpp")
PSCAT_MAX_TASKS, PSET_TASK_WINDOWS, PL_PLANES, PSET_UNIT_SCATTER = _K["PSCAT_MAX_TASKS"], _K["PSET_TASK_WINDOWS"], _K["PL_PLANES"], _K["PSET_UNIT_SCATTER"]


def _literal(header, pattern):
    return int(re.search(pattern, open(os.path.join(S.CSRC, header)).read()).group(1), 16)


# ---- the tops, from the code's own constants
PK_FIRST = _literal("planner_tasks.hpp", r"max_doc < (0x[0-9a-fA-F]+)u")  # the first max docID tasks_onepass does not give to k_planes ...
PK_LAST = PK_FIRST - 1  # ... and the largest it does
SIGN = _literal("isect_side.hpp", r"max_doc >= (0x[0-9a-fA-F]+)u")  # tri_isect_run's refusal; the first docID with bit 31 set; one document more than PSCAT_MAX_TASKS scatter tasks hold
EXTENT_EQ = (1 << 32) - 2 * SPAN  # a plane row's extent, (max docID >> 17) + 2 windows, is exactly 2^32: its end is 0 in 32 bits
TOP = (1 << 32) - 2  # the largest docID a segment can hold (0xffffffff is DocIDsEND); the rows' spare window lies wholly past 2^32
FUSED_MAX_DOC = (1 << 32) // (2 * S.FUS_W) * (2 * S.FUS_W)  # planner_lower.hpp: from this largest docID on no query is given to k_fused (its last window would end past 2^32)
TOPS = {"PK_LAST": PK_LAST, "PK_FIRST": PK_FIRST, "SIGN": SIGN, "EXTENT_EQ": EXTENT_EQ, "TOP": TOP}
assert PK_FIRST == 0x7FFF0000 and SIGN == 1 << 31 and SIGN == PSCAT_MAX_TASKS * PSET_TASK_WINDOWS * SPAN

# ---- the base: three bitmap windows, two head lists that get planes, three rare lists that do not
D_BASE = 2 * SPAN + 37
CHUNK_DOCS = S.TREE_CHUNK_WORDS * 32
EDGES = sorted({CHUNK_DOCS - 1, CHUNK_DOCS, CHUNK_DOCS + 1, SPAN - 1, SPAN, SPAN + 1, SPAN + CHUNK_DOCS, 2 * SPAN - 1, 2 * SPAN, 2 * SPAN + 1, D_BASE - 1, D_BASE})
HEADS = {"h0": (61, 0), "h1": (131, 5)}  # every `step`-th document from `first` on, and the edges: 4 310 documents (135 blocks: a cell index) and 2 014 (no cell index)
RARE = {"r0": 0, "r1": 37, "r2": 200}  # documents besides the edges: fewer than docs_cnt / 1024 = 256 each, no plane under the default plane_div
PHRASE_SHIFTS = S.STREAM_PHRASE_SHIFTS


def base_lists():
    """-> (lists, positions).  Head frequencies follow FREQ_CYCLE by rank (0, the planes' levels, 300 among them), 2 / 3 on the edge documents; hit k of head i sits at
    1 + i + shift + 7 k, shift one of 0 (five times in eight), 1, 2, 6 by a hash of (document, term) and 0 on the edge documents: "h0 h1" starts on every edge document
    — the last one among them — and wherever else both shifts agree."""
    ar = np.arange(1, D_BASE + 1, dtype=np.int64)
    edges = np.array(EDGES, dtype=np.int64)
    lists, positions = {}, {}
    for i, (n, (step, first)) in enumerate(HEADS.items()):
        d = S._u32(np.concatenate([ar[ar % step == first], edges])).astype(np.int64)
        on_edge = np.isin(d, edges)
        f = np.where(on_edge, 2 + i, np.array(S.FREQ_CYCLE, dtype=np.int64)[(np.arange(d.size) + 3 * i) % len(S.FREQ_CYCLE)])
        h = ((d.astype(np.uint64) * np.uint64(2654435761) + np.uint64(40503 * (i + 1))) >> np.uint64(13)) & np.uint64(7)
        start = 1 + i + np.where(on_edge, 0, np.array(PHRASE_SHIFTS, dtype=np.int64)[h.astype(np.int64)])
        ends = np.cumsum(f)
        k = np.arange(int(ends[-1]), dtype=np.int64) - np.repeat(ends - f, f)
        lists[n], positions[n] = (d, f), (np.repeat(start, f) + S.STREAM_PHRASE_STRIDE * k).astype(np.uint16)
    for j, (n, extra) in enumerate(RARE.items()):
        d = S._u32(np.concatenate([S.spread(extra, D_BASE - 3) + 1, edges]) if extra else edges).astype(np.int64)
        lists[n] = (d, 1 + (np.arange(d.size) * 5 + j) % 9)
    return lists, positions


def base_corpus():
    lists, positions = base_lists()
    return S.build({k: (S._u32(d), f) for k, (d, f) in lists.items()}, positions=positions)


def shift_of(top, d_base=D_BASE):
    """Whole bitmap windows: the base's window-edge and chunk-edge documents stay on edges."""
    return (top - d_base) // SPAN * SPAN


def shifted(base, top, span=False):
    """`base` with every docID moved up by shift_of(top) and its last document put on `top` (less than one window further: the order holds), docs_cnt the base's — so that
    the planner's document-frequency rules see the base's densities.  span: documents 1 and 2 join the two head lists (frequency 1; "h0 h1" starts in document 1 and
    misses in document 2): a query's range then runs from the bottom of the docID space to the top."""
    assert D_BASE <= top <= TOP and base.D == D_BASE
    sh = shift_of(top)
    lists, positions = {}, {}
    for n in base.names:
        d, f = base.lists[n]
        d = d.astype(np.int64) + sh
        if int(d[-1]) == D_BASE + sh:
            d[-1] = top
        p = base.positions[n]
        if span and n in HEADS:
            i = list(HEADS).index(n)
            d, f = np.concatenate([[1, 2], d]), np.concatenate([[1, 1], f])
            p = np.concatenate([np.array([1 + i, 2], dtype=np.uint16), p])
        assert int(d[-1]) <= top
        lists[n], positions[n] = (d.astype(np.uint32), f), p
    c = S.build(lists, positions=positions, docs_cnt=base.docs_cnt)
    assert c.D == top
    return c


def plw_of(top):
    """Words of a bitmap over the docID space of a segment whose largest docID is `top` (planner.hpp eligible_planes): whole windows and a spare one."""
    return ((top >> 17) + 2) * (SPAN // 32)


def nwin_of(top):
    return top // SPAN + 1


def row_bytes(top):
    """A full plane row (both parts) — what plane_max_bytes is counted in."""
    return PL_PLANES * plw_of(top) * 4


# ---- the catalogue (DocumentsOnly): one query per path the read side has
CASES = {
    "pair_and": "{h0} {h1}",  # two plane terms: k_psets' pair path; candidate tiles with a plane probe; k_probe
    "pair_or": "{h0} OR {h1}",
    "pair_not": "{h0} NOT {h1}",
    "rare_lead": "{r2} {h0}",  # a short lead against a plane: k_probe / k_and's probes
    "rare_pair": "{r1} {r2}",  # no plane anywhere: merges
    "rare_or": "{r0} OR {r1}",
    "scatter": "{h1} OR {r1}",  # a union of a plane term and one without: PSET_UNIT_SCATTER where the planner allows it
    "scatter4": "{h0} OR {h1} OR {r0} OR {r2}",
    "cnf": "({h0} OR {r0}) {h1}",
    "cnf2": "{h0} ({h1} OR {r2})",
    "not_rare": "{r2} NOT {h0}",
    "not_head": "{h1} NOT {r2}",
    "term_head": "{h0}",
    "term_rare": "{r0}",
    "phrase": '"{h0} {h1}"',
    "phrase_and": '"{h0} {h1}" {r2}',
    "tree": '{r2} OR "{h0} {h1}"',  # a phrase under an OR: TASK_TREE, two distinct leaves
}
SCATTER_SLACK = 1 << 20  # option scatter_bitmap_slack: the base's head lists hold one document in 61 of THREE windows — at 16 384 windows and more only this makes a scatter union


def docs_queries(c, names=None):
    return [(c.q(CASES[n]), 1) for n in (names or CASES)]


SCORED = ["{h0} {h1}", "{h0} OR {h1}", "{h0} OR {h1} OR {r2}", "{h0} ({h1} OR {r2})", "{h0} NOT {h1}", "{h1} <{r2}>", "{r2} {h0}", "{r2}", "{r1} OR {r2}"]
SCORED_K256 = "{h0} OR {h1} OR {r2}"


def scored_queries(c):
    return [(c.q(t), 1) for t in SCORED]


SCORED_SETS = [{}, {"dense_min_postings": 0}, {"dense_min_postings": 0, "planes": 0}, {"dense_min_postings": 0, "planes": 0, "fused_halfwords": 0}, {"dense_min_postings": 0, "fused": 0}]
RICH = ["{h0} {h1}", "{r2} {h0}", "{r1} OR {r2}", "{h1} OR {r1}", '"{h0} {h1}"', '"{h0} {h1}" {r2}']  # conjunctions, unions and phrases whose matches include `top`
TRUTH = ("[{h0}, {h1}, {r2}]", 2)  # a matchsome: the truth-table path (k_fused) in every mode


# ---- wrong readers: what a kernel with one of the 32-bit slips would read of a list (test_high_docid_cases.py shows that each changes a named query's result)
def _top_window(c):
    return c.D // SPAN * SPAN


def reader_loses_high(d, c):
    """documents at or past 2^31 lost (a docID << 1, a 2^31-bit bitmap index)"""
    return d[d < (1 << 31)]


def reader_last_window_end_zero(d, c):
    """the last window's end, w0 + SPAN_BITS, taken as 0 where it is 2^32: the window [w0, 0) holds nothing"""
    w0 = _top_window(c)
    return d if w0 + SPAN < (1 << 32) else d[d < w0]


def reader_drops_top(d, c):
    """document `top` dropped (an exclusive bound one too small)"""
    return d[d != c.D]


def reader_aliases_bottom(d, c):
    """the bottom of the docID space read into the top window: a window start that wrapped to 0"""
    w0 = _top_window(c)
    low = d[d < SPAN].astype(np.int64) + w0
    return np.union1d(d, low[low <= c.D].astype(np.uint32)).astype(np.uint32)


def reader_signed(d, c):
    """a signed compare: the walk ends where the next docID is not above the last one as int32"""
    s = d.view(np.int32).astype(np.int64)
    stop = np.flatnonzero(np.diff(s) <= 0)
    return d[: int(stop[0]) + 1] if stop.size else d


WRONG_READERS = {"loses_high": reader_loses_high, "last_window_end_zero": reader_last_window_end_zero, "drops_top": reader_drops_top, "aliases_bottom": reader_aliases_bottom,
                 "signed": reader_signed}  # fmt: skip
# reader -> (top, span, case) at which it must change the expected result
WRONG_AT = {"loses_high": ("SIGN", False, "pair_and"), "last_window_end_zero": ("TOP", False, "pair_or"), "drops_top": ("EXTENT_EQ", False, "phrase"),
            "aliases_bottom": ("TOP", True, "pair_or"), "signed": ("SIGN", True, "scatter")}  # fmt: skip


class _Misread:
    """evaluate() over lists as a wrong reader returns them."""

    def __init__(self, c, reader):
        self.names, self._hitpos, self.c = c.names, {}, c
        self.lists = {n: (reader(d, c), f) for n, (d, f) in c.lists.items()}

    evaluate = S.Corpus.evaluate
    _phrase = S.Corpus._phrase

    def doc_positions(self, t):
        return self.c.doc_positions(t)


def misread(c, reader, prog):
    return _Misread(c, reader).evaluate(prog)


# ---- tri_isect_run at its limit's accepting side: one gadget request (isect_cases.gadget) whose run ends on the last document, restated from the postings arrays
def isect_gadget(top):
    """Three groups a, b, c: c alone in document 5, a strict superset {a, b} at top - 10, then a run of {a} from top - 8 to `top`.  -> (Corpus, groups as term ids)"""
    run = np.arange(top - 8, top + 1, dtype=np.int64)
    lists = {"a": np.concatenate([[top - 10], run]), "b": np.array([top - 10]), "c": np.array([5])}
    c = S.build({k: (S._u32(d), np.ones(d.size, dtype=np.int64)) for k, d in lists.items()}, docs_cnt=64)
    return c, [[c.tid["a"]], [c.tid["b"]], [c.tid["c"]]]


def isect_restate(c, groups, stop=0):
    """isect_cases.restate without its array over the docID space: the union walk over the sorted distinct documents of the request's lists."""
    import isect_cases as IC

    pg = [[c.lists[c.names[t]][0].astype(np.int64) for t in g] for g in groups]
    orig, any_known = IC.orig_mask(pg)
    docs = np.unique(np.concatenate([t for g in pg for t in g]))
    masks = [0] * docs.size
    for i, g in enumerate(pg):
        for t in g:
            for k in np.searchsorted(docs, t).tolist():
                masks[k] |= 1 << i
    ctx, hist = IC.Ctx(), {}
    for d, m in zip(docs.tolist(), masks):
        if any_known and IC.considered(m, orig, stop):
            ctx.consider(m)
            n, f = hist.get(m, (0, d))
            hist[m] = (n + 1, f)
    return ctx.finalize(), hist
