"""The contract of column predicates as document filters (include/trinity_hip.h: tri_filters_from_columns / tri_filter_bitmap) in plain numpy, and the cases that
tests/test_colfilter_cases.py (CPU: the cases tell the right answer from nine wrong implementations; csrc/host/column_pred.hpp equals the contract), tests/test_gpu_colfilter.py
(the engine) and tests/test_host_mirror_colfilter.py (the operator surface) share.

A column is a u32 array of D + 1 values (values[d] = the attribute of docID d; values[0] is never read): order_cases.columns — facet_cases' five and `rev`, `hash` — plus
`mod7@2`, a SECOND column handle over mod7's values (the eighth distinct column a call may name).  A clause is a dict: {"col", "kind": "range" | "set", "lo", "hi",
"set", "negate"}; a Case is a named predicate (clauses, any), the mode it is built in (keep) and, optionally, which `also` filter it names:
  "create"  a filter made by tri_filter_create: also_create_ids(D), dropped;
  "docset"  a filter made by tri_filter_from_docset(keep=True) of the corpus' ALSO_QUERY: everything outside that query's docset is dropped.
The filter of a case drops document d (1 .. D) iff its `also` filter drops d, or the predicate holds for d (mode DROP) / does not hold for d (mode KEEP)."""
import numpy as np

import order_cases as OC
import structured as S

CONSTANTS = S.header_constants("dev_structs.hpp")
CHUNK = CONSTANTS["COLFILTER_CHUNK"]  # docIDs a workgroup of k_filter_columns owns (csrc/k_filter_columns.hpp)
WAVE_DOCS = CONSTANTS["COLFILTER_WAVE_DOCS"]
MAX_CLAUSES, MAX_COLUMNS, MAX_PREDS = CONSTANTS["COLFILTER_MAX_CLAUSES"], CONSTANTS["COLFILTER_MAX_COLUMNS"], CONSTANTS["COLFILTER_MAX_PREDS"]
SET_LIMIT = CONSTANTS["FACET_MAX_BUCKETS"]  # a SET value is below it; a column value at or above it is in no set
HUGE = 0xFFFFFFFF
TINY = {"D": 2000, "V": 200, "slots": 10, "seed": 42}  # the tiny fixture corpus (tests/golden/ref_masked.json: corpora.tiny): smaller than one chunk
ALSO_QUERY = {"stream": "{h0} OR {h1}", "tiny": "t0 OR t1"}  # the query whose docset the "docset" `also` filter keeps
COLUMN_NAMES = ["mod7", "window", "one", "low16", "huge", "rev", "hash", "mod7@2"]
assert TINY["D"] < CHUNK < S.D_STREAM and S.D_STREAM % 64 and S.D_STREAM % 32 and len(COLUMN_NAMES) == MAX_COLUMNS


def columns(D):
    out = dict(OC.columns(D))
    out["mod7@2"] = out["mod7"]
    return {n: out[n] for n in COLUMN_NAMES}


# ---- clauses and cases -------------------------------------------------------------------------------------------------------------------------------
def R(col, lo, hi, negate=False):
    return {"col": col, "kind": "range", "lo": int(lo), "hi": int(hi), "set": [], "negate": negate}


def IN(col, values, negate=False):
    return {"col": col, "kind": "set", "lo": 0, "hi": 0, "set": [int(v) for v in values], "negate": negate}


def docs(D, a, b, negate=False):
    """The documents a .. b (both inclusive), as a RANGE over `rev` (rev[d] = D - d)."""
    return R("rev", D - b, D - a, negate)


class Case:
    def __init__(self, name, clauses, any=False, keep=True, also=None, trivial=None):
        self.name, self.clauses, self.any, self.keep, self.also, self.trivial = name, list(clauses), any, keep, also, trivial  # trivial: "all" / "none" — holds for every / no document, by name

    def in_mode(self, keep):
        return Case(f"{self.name}/{'keep' if keep else 'drop'}", self.clauses, self.any, keep, self.also, self.trivial)

    def __repr__(self):
        return self.name


def predicates(D):
    """The predicates over a corpus of D documents, mode not yet chosen (keep=True)."""
    out = [
        # ranges whose ends fall on documents 1 and D
        Case("doc_1", [docs(D, 1, 1)]), Case("doc_D", [docs(D, D, D)]), Case("docs_1_to_mid", [docs(D, 1, D // 2)]), Case("docs_mid_to_D", [docs(D, D // 2, D)]),
        Case("docs_2_to_D-1", [docs(D, 2, D - 1)]), Case("last_partial_word", [docs(D, D - (D % 32) + 1, D)]), Case("last_partial_group", [docs(D, D - (D % 64), D)]),
        # lo == hi, lo > hi, the full range
        Case("lo_eq_hi", [R("mod7", 3, 3)]), Case("lo_gt_hi", [R("mod7", 5, 2)], trivial="none"), Case("full_range", [R("hash", 0, HUGE)], trivial="all"),
        Case("lo_gt_hi_negated", [R("mod7", 5, 2, negate=True)], trivial="all"),
        # values at 0x80000000 and 0xffffffff
        Case("across_the_sign_bit", [R("hash", 0x40000000, 0xC0000000)]), Case("from_0x80000000", [R("hash", 0x80000000, HUGE)]), Case("to_0x7fffffff", [R("hash", 0, 0x7FFFFFFF)]),
        Case("only_0xffffffff", [R("huge", HUGE, HUGE)]), Case("huge_from_0x80000000", [R("huge", 0x80000000, HUGE)]), Case("huge_small", [R("huge", 1, 0x80000000)]),
        # SET
        Case("set_empty", [IN("mod7", [])], trivial="none"), Case("set_duplicates", [IN("mod7", [3, 3, 5, 3, 5])]), Case("set_with_65535", [IN("huge", [0, 1, SET_LIMIT - 1])]),
        Case("set_on_wide_column", [IN("rev", [1, 2, 3, 100, SET_LIMIT - 1])]), Case("set_low16_ends", [IN("low16", [SET_LIMIT - 1, 0, 1])]),
        Case("set_chunk_edges", [IN("low16", sorted({(p + x) % SET_LIMIT for p in range(0, SET_LIMIT, CHUNK) for x in (-1, 0, 1)}))]),
        Case("set_wave_edges", [IN("low16", sorted({(p + x) % SET_LIMIT for p in range(0, SET_LIMIT, WAVE_DOCS) for x in (-1, 0)}))]),
        # negate
        Case("negated_range", [R("mod7", 3, 3, negate=True)]), Case("negated_set", [IN("huge", [0, 1, SET_LIMIT - 1], negate=True)]), Case("negated_empty_set_and_range", [IN("mod7", [], negate=True), R("mod7", 1, 2)]),
        # any against all, over 1, 2 and 8 clauses
        Case("one_clause_any", [R("mod7", 0, 2)], any=True), Case("two_all", [R("mod7", 0, 2), R("huge", 0, 1)]), Case("two_any", [R("mod7", 0, 2), R("huge", 0, 1)], any=True),
        Case("two_any_negated", [R("mod7", 0, 2, negate=True), IN("huge", [4])], any=True),
        # one column in 8 clauses
        Case("one_column_8_all", [docs(D, 1 + k, D - k) for k in range(4)] + [docs(D, 7 * k, 7 * k + 3, negate=True) for k in range(1, 5)]),
        Case("one_column_8_any", [docs(D, 1 + (D // 9) * k, 5 + (D // 9) * k) for k in range(8)], any=True),
        # 8 distinct columns
        Case("eight_columns_all", [R("mod7", 1, 6), R("window", 0, 1), R("one", 0, 0), R("low16", 0, 60000), R("huge", HUGE, HUGE, negate=True), R("rev", 10, 1 << 30), R("hash", 0x10000000, 0xF0000000),
                                   IN("mod7@2", [1, 2, 3, 4])]),
        Case("eight_columns_any", [R("mod7", 6, 6), R("window", 1, 1), R("one", 1, 1), IN("low16", [5, 77]), R("huge", HUGE, HUGE), R("rev", 0, 3), R("hash", 0, 0x0FFFFFFF), IN("mod7@2", [0])], any=True),
        # `also`
        Case("also_create", [R("mod7", 0, 4)], also="create"), Case("also_docset", [R("mod7", 2, 6)], also="docset"), Case("also_create_any", [IN("huge", [2, 3]), docs(D, 1, 40)], any=True, also="create"),
        Case("also_docset_doc_D", [docs(D, D - 40, D)], also="docset"),
    ]  # fmt: skip
    # ranges on both sides of every multiple of the kernel's chunk: eight multiples a predicate, the two documents m - 1 | m astride each ...
    mult = list(range(CHUNK, D + 1, CHUNK))
    for i in range(0, len(mult), MAX_CLAUSES):
        out.append(Case(f"astride_chunks_{i // MAX_CLAUSES}", [docs(D, m - 1, m) for m in mult[i : i + MAX_CLAUSES]], any=True))
    # ... and ranges that END below / START at a multiple, for the first, the middle and the last ones
    for m in sorted(set(mult[:2] + mult[len(mult) // 2 : len(mult) // 2 + 1] + mult[-2:])):
        out += [Case(f"below_chunk_{m}", [docs(D, 1, m - 1)]), Case(f"from_chunk_{m}", [docs(D, m, D)])]
    # ... of every multiple of SPAN_BITS (the bitmap kernels' window), and the window column itself
    for m in range(S.SPAN_BITS, D + 1, S.SPAN_BITS):
        out += [Case(f"below_span_{m}", [docs(D, 1, m - 1)]), Case(f"from_span_{m}", [docs(D, m, D)]), Case(f"astride_span_{m}", [docs(D, m - 1, m)]), Case(f"window_{m // S.SPAN_BITS}", [R("window", m // S.SPAN_BITS, m // S.SPAN_BITS)])]
    assert len({c.name for c in out}) == len(out)
    return out


def cases(D):
    """Every predicate in both modes."""
    return [p.in_mode(keep) for p in predicates(D) for keep in (True, False)]


def also_create_ids(D):
    """What the "create" `also` filter drops: documents 1 and D, every 11th document, and the last 64."""
    return np.unique(np.concatenate([[1, D], np.arange(11, D + 1, 11), np.arange(D - 63, D + 1)])).astype(np.uint32)


def also_bits(kind, D, docset=None):
    """bool [D + 1]: the documents the `also` filter of `kind` drops (docset: ALSO_QUERY's docID set on the corpus)."""
    bits = np.zeros(D + 1, dtype=bool)
    if kind == "create":
        bits[also_create_ids(D)] = True
    elif kind == "docset":
        bits[1:] = True
        bits[np.asarray(docset, dtype=np.int64)] = False
    return bits


# ---- the contract, and what a wrong implementation would answer (mutant) ------------------------------------------------------------------------------
MUTANTS = ["shift", "signed", "hi_exclusive", "no_negate", "any_as_all", "set_wrap", "modes_swapped", "no_also", "tail_unwritten"]


def clause_holds(cl, cols, mutant=None):
    v = cols[cl["col"]]
    if mutant == "shift":  # the column read one docID off
        v = np.concatenate([v[1:], v[:1]])
    if cl["kind"] == "range":
        if mutant == "signed":
            sv, lo, hi = v.astype(np.int64), cl["lo"], cl["hi"]
            sv = np.where(sv >= 1 << 31, sv - (1 << 32), sv)
            lo, hi = (lo - (1 << 32) if lo >= 1 << 31 else lo), (hi - (1 << 32) if hi >= 1 << 31 else hi)
            t = (sv >= lo) & (sv <= hi)
        else:
            t = (v >= np.uint32(cl["lo"])) & ((v < np.uint32(cl["hi"])) if mutant == "hi_exclusive" else (v <= np.uint32(cl["hi"])))
    else:
        members = np.asarray(sorted(set(cl["set"])), dtype=np.uint32)
        t = np.isin(v & np.uint32(SET_LIMIT - 1), members) if mutant == "set_wrap" else (v < SET_LIMIT) & np.isin(v, members)
    return ~t if cl["negate"] and mutant != "no_negate" else t


def holds(case, cols, mutant=None):
    """bool [D + 1]: where the predicate holds (entry 0 is meaningless)."""
    ts = [clause_holds(cl, cols, mutant) for cl in case.clauses]
    return np.logical_or.reduce(ts) if case.any and mutant != "any_as_all" else np.logical_and.reduce(ts)


def drop_bits(case, cols, D, also=None, mutant=None):
    """bool [D + 1]: the documents the case's filter drops; also: also_bits of the case's `also` filter (None: it names none)."""
    h = holds(case, cols, mutant)
    keep = case.keep != (mutant == "modes_swapped")
    bits = ~h if keep else h.copy()
    if also is not None and mutant != "no_also":
        bits |= also
    bits[0] = False
    if mutant == "tail_unwritten":
        bits[(D >> 5) << 5 :] = False
    return bits


def words_of(bits, nwords):
    """The drop bitmap as tri_filter_bitmap lays it out: bit d & 31 of word d >> 5."""
    padded = np.zeros(nwords * 32, dtype=np.uint8)
    padded[: bits.size] = bits
    return np.packbits(padded, bitorder="little").view(np.uint32)


def bits_of(words, D):
    """bool [D + 1] of a bitmap's words, entry 0 cleared (bit 0 is unspecified)."""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[: D + 1].astype(bool)
    bits[0] = False
    return bits
