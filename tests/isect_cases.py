"""The cases of Trinity::intersect on the device (tri_isect_run; a helper module, imported by tests/test_isect_cases.py, tests/test_gpu_isect.py and
tests/test_host_mirror_isect.py) and its yardstick: intersect.cpp restated in plain Python.

restate() is intersect_impl (intersect.cpp:5-170) over explicit postings: the known / unknown terms and origMask (:25-51), the walk of the union of the lists in
docID order with a document's mask (:107-158 — merge_literal() is that loop iterator by iterator; restate() takes the same documents from a numpy OR over the docID
space, and the CPU file checks the two against each other), ctx::consider (:64-91, Ctx.consider: the same scan, swap-removal and push, the `map == mapPrev`
shortcut with indexPrev) and finalize (:93-99).  Nothing in it comes from the engine.  Two things differ from the reference's code on purpose, as in
include/trinity_hip.h: the stop-word rule is the documented one (intersect.h:15-18: the lowest or the highest set bit of the mask is a stop word), and indexPrev
does not wrap at 256 — every case keeps the antichain at or below 255 entries (restate() reports the largest it saw; the CPU file asserts it per case).

derive() is the order-free route the engine takes (csrc/host/isect_rows.hpp): table H (per distinct considered mask its documents and first docID) and table C
(per (mask, epoch) the considered documents whose preceding considered document has the same mask, counted from the mask's threshold on), then the replay.

Three WRONG answers every case must be told from (wrong_answers()): the maximal masks with their true counts; consider() without the shortcut (no run credit); the
predecessor taken as the previous DOCUMENT of the walk rather than the previous considered one.  Every case but `unknown_all` (whose answer is empty by
construction) therefore holds a gadget: a strict superset, then a run of a smaller mask with a document inside that is not considered.

A case's documents are written as a script of (docID, terms) events; terms are named per case, all cases share one corpus of about three plane windows
(structured.build encodes it with both host encoders).  The masked documents of all cases form ONE set, installed on the index once (they are docIDs; a case's
restatement takes the whole set).
"""
import numpy as np

SPAN = 4096  # csrc/k_isect.hpp ISECT_SPAN (test_isect_cases.py checks the mirrors; the GPU file reads them from tri_isect_info)
LDS_SLOTS = 256  # ISECT_LDS_SLOTS
PL_W = 32768
D = 3 * PL_W + 1234  # the last document of the docID space
UNKNOWN = None  # a token the index does not know
M64 = (1 << 64) - 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
class Ctx:
    """intersect.cpp:53-100"""

    def __init__(self, shortcut=True):
        self.map_prev, self.index_prev, self.matches, self.shortcut, self.largest = 0, 0, [], shortcut, 0

    def consider(self, m):  # :64-91
        if self.shortcut and m == self.map_prev:  # :65
            self.matches[self.index_prev][1] += 1  # :66
            return
        self.map_prev = m  # :71
        cnt, i = len(self.matches), 0
        while i < cnt:  # :72
            v = self.matches[i][0]
            if (v & m) == m:  # :73
                if m == v:  # :75
                    self.matches[i][1] += 1
                self.index_prev = i  # :77 (a uint8_t there: every case stays at or below 255 entries)
                return
            elif (m & v) == v:  # :79
                self.matches[i] = self.matches[-1]  # :81
                self.matches.pop()  # :82
                cnt -= 1
            else:
                i += 1
        self.index_prev = cnt  # :88
        self.matches.append([m, 1])  # :89
        self.largest = max(self.largest, len(self.matches))

    def finalize(self):  # :93-99, ties (which std::sort leaves unspecified) by ascending mask
        return sorted(((v, c & 0xFFFFFFFF) for v, c in self.matches), key=lambda e: (-bin(e[0]).count("1"), -e[1], e[0]))


def orig_mask(groups):
    """:25-51 — groups: lists of docID arrays, UNKNOWN (or an empty array: term_ctx().documents == 0) for an unknown token -> (origMask, any known term)"""
    orig, unknown, rem = 0, False, 0
    for i, g in enumerate(groups):
        for t in g:
            if t is not UNKNOWN and len(t):
                orig |= 1 << i  # :33
                rem += 1
            else:
                unknown = True  # :42
    return (0 if unknown else orig), rem > 0  # :50-51, :47


def considered(mask, orig, stop):
    """:138-139 with the documented stop-word rule (intersect.h:15-18)"""
    if mask == orig:
        return False
    return not (stop & ((mask & -mask) | (1 << (mask.bit_length() - 1))))


def doc_masks(groups, top):
    """mask[d] for d in 0 .. top: bit i <=> a term of group i holds d (the OR the merge loop builds per document, :111-131)"""
    m = np.zeros(top + 1, dtype=np.uint64)
    for i, g in enumerate(groups):
        for t in g:
            if t is not UNKNOWN and len(t):
                m[np.asarray(t, dtype=np.int64)] |= np.uint64(1 << i)
    return m


def merge_literal(groups):
    """:107-158 as written: `remaining` iterators, the lowest current document by a linear scan, its mask, next() on the selected ones, swap-removal of an ended one.
    -> [(docID, mask)]"""
    remaining = [[0, np.asarray(t, dtype=np.int64), i] for i, g in enumerate(groups) for t in g if t is not UNKNOWN and len(t)]  # [cursor, docs, tokenIdx] :25-45
    out = []
    rem = len(remaining)
    while rem:
        it = remaining[0]
        lowest, mask, selected = int(it[1][it[0]]), 1 << it[2], [0]  # :110-115
        for i in range(1, rem):  # :116-134
            it = remaining[i]
            d = int(it[1][it[0]])
            if d == lowest:
                mask |= 1 << it[2]
                selected.append(i)
            elif d < lowest:
                mask, selected, lowest = 1 << it[2], [i], d
        out.append((lowest, mask))
        while selected:  # :145-157
            idx = selected.pop()
            remaining[idx][0] += 1
            if remaining[idx][0] == len(remaining[idx][1]):  # :148 DocIDsEND
                rem -= 1
                remaining[idx] = remaining[rem]  # :155 (selected is popped from the back: the moved slot has been advanced already)
    return out


def walk(groups, stop=0, masked=(), top=D):
    """-> (docIDs, masks, considered flags) of the union walk, ascending; origMask applied"""
    orig, any_known = orig_mask(groups)
    if not any_known:
        z = np.zeros(0, dtype=np.int64)
        return z, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool), orig
    m = doc_masks(groups, top)
    docs = np.nonzero(m)[0]
    masks = m[docs]
    is_masked = np.isin(docs, np.asarray(list(masked), dtype=np.int64)) if len(masked) else np.zeros(docs.size, dtype=bool)
    ok = np.array([considered(int(x), orig, stop) for x in masks.tolist()], dtype=bool) & ~is_masked
    return docs, masks, ok, orig


def restate(groups, stop=0, masked=(), top=D):
    """-> (the reference's list [(mask, count)], H {mask: (count, first docID)}, the largest antichain)"""
    docs, masks, ok, _ = walk(groups, stop, masked, top)
    c = Ctx()
    H = {}
    for d, m in zip(docs[ok].tolist(), masks[ok].tolist()):
        c.consider(m)
        n, f = H.get(m, (0, d))
        H[m] = (n + 1, f)
    return c.finalize(), H, c.largest


def run_sequence(seq, shortcut=True):
    c = Ctx(shortcut)
    for m in seq:
        c.consider(m)
    return c.finalize(), c.largest


# ---- the order-free derivation (csrc/host/isect_rows.hpp) ----------------------------------------------------------------------------------------
def tables(seq_docs, seq_masks):
    """H and C of a considered sequence: H {mask: (count, first)}; C {(mask, epoch): count} for documents at or past the mask's threshold"""
    H = {}
    for d, m in zip(seq_docs, seq_masks):
        n, f = H.get(m, (0, d))
        H[m] = (n + 1, f)
    firsts = sorted(f for _, f in H.values())
    thr = {}
    for m, (_, f) in H.items():
        sup = [f2 for m2, (_, f2) in H.items() if m2 != m and (m2 & m) == m]
        thr[m] = max(f, min(sup)) if sup else None
    C = {}
    prev = 0
    for d, m in zip(seq_docs, seq_masks):
        if m == prev and thr[m] is not None and d >= thr[m]:
            e = int(np.searchsorted(firsts, d, side="right"))
            C[(m, e)] = C.get((m, e), 0) + 1
        prev = m
    return H, C


def replay(H, C):
    order = sorted(H, key=lambda m: H[m][1])
    vec = []  # [mask, credit]
    for e, m in enumerate(order, 1):
        i, n, covered = 0, len(vec), False
        while i < n:
            v = vec[i][0]
            if (v & m) == m:
                covered = True
                break
            elif (m & v) == v:
                vec[i] = vec[-1]
                vec.pop()
                n -= 1
            else:
                i += 1
        if not covered:
            vec.append([m, 0])
        for (cm, ce), cnt in C.items():
            if ce == e and all(v[0] != cm for v in vec):
                for v in vec:
                    if (v[0] & cm) == cm:
                        v[1] += cnt
                        break
    return sorted((((v, (H[v][0] + cr) & 0xFFFFFFFF)) for v, cr in vec), key=lambda e: (-bin(e[0]).count("1"), -e[1], e[0]))


def derive(seq_docs, seq_masks):
    return replay(*tables(seq_docs, seq_masks))


def wrong_answers(groups, stop=0, masked=(), top=D):
    """-> {name: list} of the three wrong answers over the same postings"""
    docs, masks, ok, _ = walk(groups, stop, masked, top)
    seq = masks[ok].tolist()
    H = {}
    for m in seq:
        H[m] = H.get(m, 0) + 1
    maximal = [(m, n) for m, n in H.items() if not any(o != m and (o & m) == m for o in H)]
    fin = lambda v: sorted(v, key=lambda e: (-bin(e[0]).count("1"), -e[1], e[0]))
    # the predecessor is the previous document of the walk: a document that is not considered still resets mapPrev
    c = Ctx()
    for m, k in zip(masks.tolist(), ok.tolist()):
        if k:
            c.consider(m)
        else:
            c.map_prev = 0
    return {"maximal_true_counts": fin(maximal), "no_run_credit": run_sequence(seq, shortcut=False)[0], "previous_document": c.finalize()}


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, groups, events, stop=0, masked=(), why="", top=D):
        """groups: lists of term names (UNKNOWN for an unknown token); events: (docID, [term names])"""
        self.name, self.groups, self.stop, self.masked, self.why, self.top = name, groups, stop, sorted(masked), why, top
        self.lists = {}
        for g in groups:
            for t in g:
                if t is not UNKNOWN:
                    self.lists.setdefault(f"{name}.{t}", [])
        for d, ts in events:
            assert 1 <= d <= top, (name, d)
            for t in ts:
                self.lists[f"{name}.{t}"].append(d)
        self.lists = {k: np.unique(np.asarray(v, dtype=np.int64)) for k, v in self.lists.items()}

    def posting_groups(self):
        return [[UNKNOWN if t is UNKNOWN else self.lists[f"{self.name}.{t}"] for t in g] for g in self.groups]

    def term_ids(self, tid):
        """(terms u32, per-group counts) for tri_isect_run; tid: list name -> term id"""
        terms, counts = [], []
        for g in self.groups:
            counts.append(len(g))
            terms += [0xFFFFFFFF if t is UNKNOWN else tid[f"{self.name}.{t}"] for t in g]
        return terms, counts


def gadget(at, run, inside=(), small=("a",), big=("a", "b")):
    """a strict superset at `at`, then the run documents of the smaller mask; `inside`: (docID, terms) of documents in between that are not considered"""
    return [(at, list(big))] + [(d, list(small)) for d in run] + list(inside)


def cases(span=SPAN, lds_slots=LDS_SLOTS):
    S, out = span, []
    abc = [["a"], ["b"], ["c"]]
    ORIG = ["a", "b", "c"]
    # 1. a run of equal non-maximal masks straddles a 64-document step
    at = 2 * S + 64 * 7 + 59
    out.append(Case("step", abc, gadget(at, [at + i for i in range(1, 12) if i != 6], [(at + 6, ORIG)]), why="a run straddles a 64-document step"))
    # 2. ... a span boundary
    at = 3 * S - 5
    out.append(Case("span", abc, gadget(at, [at + i for i in range(1, 11) if i != 7], [(at + 7, ORIG)]), why="a run straddles a span boundary"))
    # 3. ... with wholly empty spans in between (the look-back passes them; tall_cases(): more than 64 of them, a second look)
    at = 5 * S - 3
    run = [at + 1, at + 2, 8 * S + 1, 8 * S + 3, 8 * S + 4]
    out.append(Case("empty_spans", abc, gadget(at, run, [(8 * S + 2, ORIG)]), why="a run straddles spans that hold nothing"))
    # 4. a run starts in the first document, another ends in the last document of the docID space
    ev = [(1, ["a"]), (2, ["a"]), (3, ["a", "b"])] + [(d, ["a"]) for d in list(range(4, D - 1, 997)) + [D - 1, D]] + [(S + 7, ORIG)]
    out.append(Case("ends", abc, ev, why="runs from the first document and to the last document of the docID space"))
    # 5. a masked document and an origMask document inside a run: the run continues across both
    at = 9 * S + 100
    out.append(Case("masked", abc, gadget(at, [at + 1, at + 2, at + 4, at + 6, at + 7], [(at + 3, ["b"]), (at + 5, ORIG)]), masked=[at + 3], why="a masked and an origMask document inside a run"))
    # 6. a stop-word document inside a run (group 2 is a stop word: {b, c} ends on it)
    at = 10 * S + 200
    out.append(Case("stop", abc, gadget(at, [at + 1, at + 2, at + 4, at + 5], [(at + 3, ["b", "c"])]), stop=1 << 2, why="a stop-word document inside a run"))
    # 7. the covering superset changes between epochs: the run credits of {a} go to {a,b}, then (it is deleted by {a,b,d}; {a,c} moves to slot 0) to {a,c}, then
    #    ({a,c} is deleted by {a,c,d}) to {a,b,d}
    at = 11 * S + 300
    ev = [(at, ["a", "b"]), (at + 1, ["a", "c"])] + [(at + 2 + i, ["a"]) for i in range(3)] + [(at + 5, ["a", "b", "d"])] + [(at + 6 + i, ["a"]) for i in range(3)]
    ev += [(at + 11, ["a", "c", "d"])] + [(at + 12 + i, ["a"]) for i in (0, 1, 3, 4)] + [(at + 14, ["a", "b", "c", "d"])]  # (an origMask document inside the last run)
    out.append(Case("epochs", [["a"], ["b"], ["c"], ["d"]], ev, why="the covering entry changes between epochs and one is deleted"))
    # 8. a mask's strict superset first appears in the middle of a span: before it the run is H's, after it C's
    at = 12 * S + 2000
    ev = [(at - 9 + i, ["a"]) for i in range(9)] + gadget(at, [at + i for i in range(1, 9) if i != 4], [(at + 4, ORIG)])
    out.append(Case("mid_span", abc, ev, why="the superset first appears in the middle of a span"))
    # 9. more distinct masks than LDS slots in ONE span; the antichain stays at 1 ({g0..g8} covers everything, origMask has bit 9 too)
    n = lds_slots + 44
    assert n < 511
    base = 13 * S + 5
    g10 = [[f"g{i}"] for i in range(10)]
    bits = lambda m: [f"g{i}" for i in range(10) if m >> i & 1]
    ev = [(base, bits(0x1FF))] + [(base + m, bits(m)) for m in range(1, n + 1)] + [(base + n + 1, bits(n)), (base + n + 2, bits(0x3FF)), (base + n + 3, bits(n))]
    assert base + n + 3 < 14 * S
    out.append(Case("spill", g10, ev, why="more distinct masks than LDS slots in one span"))
    # 10. 64 groups, bit 63 in use
    at = 14 * S + 17
    g64 = [[f"t{i}"] for i in range(64)]
    all64 = [f"t{i}" for i in range(64)]
    ev = gadget(at, [at + 1, at + 2, at + 4, at + 5], [(at + 3, all64)], small=("t63",), big=("t63", "t0")) + [(at + 9, ["t62", "t63"]), (at + 10, ["t62", "t63"])]
    out.append(Case("wide", g64, ev, why="64 groups, bit 63 in use"))
    # 11. a group of three synonyms, one unknown: origMask = 0 and documents that hold every group are counted; a document with two synonyms of a group
    at = 15 * S + 400
    ev = [(at, ["a1", "b"]), (at + 1, ["a2"]), (at + 2, ["a1"]), (at + 3, ["a1", "a2"]), (at + 4, ["b"]), (at + 5, ["a2"]), (at + 6, ["a2", "b"]), (at + 7, ["a1", "b"])]
    out.append(Case("synonyms", [["a1", "a2", UNKNOWN], ["b"]], ev, masked=[at + 4], why="three synonyms, one unknown: origMask = 0"))
    # 12. a group that lies wholly in one plane window (window 1); the run leaves the window
    at = PL_W + 5000
    ev = [(7, ["a"]), (9, ["a"])] + gadget(at, [at + 1, at + 2, at + 4, 2 * PL_W - 1, 2 * PL_W, 2 * PL_W + 1, 2 * PL_W + 3], [(at + 3, ORIG), (PL_W + 1, ["c"]), (2 * PL_W - 2, ["c"])])
    out.append(Case("one_window", abc, ev, why="groups b and c lie wholly in one window"))
    # 13. no known term at all (one token unknown to the dictionary, one whose list is empty)
    out.append(Case("unknown_all", [[UNKNOWN], ["nodocs"]], [], why="no known term: empty lists"))
    return out


D_TALL = 75 * SPAN + 77


def tall_cases(span=SPAN):
    """A docID space of 75 spans, nearly empty: a run across more than 64 spans that hold nothing (the look-back's second look of 64 span words), with an origMask
    document inside; and a run whose predecessor lies exactly 64 and 65 spans back."""
    S = span
    at = 2 * S - 2
    ev = gadget(at, [at + 1, 68 * S + 5, 68 * S + 7, 68 * S + 8], [(68 * S + 6, ["a", "b", "c"])])
    a = Case("lookback", [["a"], ["b"], ["c"]], ev, why="more than 64 empty spans inside a run", top=D_TALL)
    ev = gadget(5, [S - 1, 64 * S + 1, 65 * S + 3, 65 * S + 4, 66 * S + 2], [(65 * S + 2, ["a", "b", "c"]), (D_TALL, ["c"])])
    b = Case("lookback64", [["a"], ["b"], ["c"]], ev, why="the predecessor lies exactly 64 spans back", top=D_TALL)
    return [a, b]


def dense_cases():
    """Random postings over the cases' docID space: 5 tokens with 4 common ones (a document in two holds each) and 6 with 5, the rest rare (one document in 500).
    Every fifth document is masked.  The rare tokens' masks keep arriving late, so epochs keep opening while the common masks' runs go on: table C — keyed by (mask, epoch) — holds more than
    4 x 2^groups entries (test_isect_cases.py asserts it): it cannot be sized from the group count."""
    out = []
    for g, ncommon, seed in ((5, 4, 5), (6, 5, 5)):
        rng = np.random.default_rng(seed)
        c = Case(f"dense{g}", [[f"t{i}"] for i in range(g)], [], why="table C beyond 4 x 2^groups entries")
        for i in range(g):
            d = np.nonzero(rng.random(D + 1) < (0.5 if i < ncommon else 0.002))[0]
            c.lists[f"dense{g}.t{i}"] = d[d > 0].astype(np.int64)
        c.masked = list(range(5, D + 1, 5))  # (every fifth document is masked: documents that are not considered sit inside the runs)
        out.append(c)
    return out


def masked_of(cs):
    return sorted({d for c in cs for d in c.masked})


def corpus(cs):
    """structured.build over every case's lists (an empty list is a term without documents)"""
    import structured as St

    lists = {}
    for c in cs:
        for k, d in c.lists.items():
            lists[k] = (d.astype(np.uint32), np.ones(d.size, dtype=np.uint32))
    return St.build(lists, docs_cnt=max(c.top for c in cs))


def random_sequences(n, seed):
    """seeded run-structured mask sequences over 2 .. 6 bits: [(docIDs, masks)]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        bits = int(rng.integers(2, 7))
        seq = []
        for _ in range(int(rng.integers(1, 40))):
            seq += [int(rng.integers(1, 1 << bits))] * int(rng.integers(1, 5))
        docs = np.cumsum(rng.integers(1, 50, size=len(seq))).tolist()
        out.append((docs, seq))
    return out


def dump_vectors(path, items):
    """H and C of (docs, masks) sequences with the restatement's list, for tests/cpp/isect_rows_cpu_test.cpp: per case `case nH nC nR`, then `h mask count first`,
    `c mask epoch count`, `r mask count` lines"""
    with open(path, "w") as f:
        for docs, seq in items:
            H, C = tables(docs, seq)
            want, _ = run_sequence(seq)
            f.write(f"case {len(H)} {len(C)} {len(want)}\n")
            for m, (n, first) in H.items():
                f.write(f"h {m} {n} {first}\n")
            for (m, e), n in C.items():
                f.write(f"c {m} {e} {n}\n")
            for m, n in want:
                f.write(f"r {m} {n}\n")
