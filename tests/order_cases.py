"""The contract of ordering by a column (include/trinity_hip.h: tri_batch_set_order / tri_batch_ordered / tri_cbatch_ordered) in plain Python, and the cases
tests/test_order_cases.py (CPU: the cases tell a right answer from five wrong ones) and the GPU files (tests/test_gpu_order*.py, tests/test_host_mirror_order.py: the
engine) share.

A column is a u32 array of D + 1 values (values[d] = the attribute of docID d; values[0] is never read).  A query's row holds the first min(|S|, k) documents of its
docID set S by (values[d] ascending, docID ascending) — descending: (values[d] descending, docID ASCENDING); values compare as unsigned 32-bit."""
import numpy as np

import facet_cases as F
import structured as S

CONSTANTS = S.header_constants("dev_structs.hpp")
MAX_TOPK = CONSTANTS["ORDER_MAX_TOPK"]
TILE = CONSTANTS["ORDER_TILE"]  # documents a wave offers per step
WAVE_PASS = CONSTANTS["ORDER_TILE"] * CONSTANTS["ORDER_UNROLL"]  # ... and per pass through its loop: below it only wave 0 of a task holds anything
WG_PASS = CONSTANTS["ORDER_WG"] * CONSTANTS["ORDER_UNROLL"]  # documents a workgroup takes per pass: past it a wave comes round again
BUF = CONSTANTS["ORDER_BUF"]  # keys of a wave's candidate buffer
PRUNE_AT = CONSTANTS["ORDER_PRUNE_AT"]  # ... and how many it may hold before it is pruned to its best K
FANIN = CONSTANTS["ORDER_FANIN"]  # lists a merge group folds: a query of more tasks takes a second round
HUGE = 0xFFFFFFFF


def first_k(docset, values, k, descending=False):
    """(docids, values) of the first min(len(docset), k) documents of the set, by numpy.lexsort over (docID, value as a 64-bit integer — negated when descending)."""
    docs = np.asarray(docset, dtype=np.int64)
    v = np.asarray(values, dtype=np.uint32)[docs].astype(np.int64)
    order = np.lexsort((docs, -v if descending else v))[:k]
    return docs[order].astype(np.uint32), v[order].astype(np.uint32)


def rows(docsets, values, k, descending=False):
    """What tri_batch_ordered delivers: (docids [nq, k], values [nq, k], counts [nq]), zero past a row's count."""
    d, v, c = np.zeros((len(docsets), k), np.uint32), np.zeros((len(docsets), k), np.uint32), np.zeros(len(docsets), np.uint32)
    for i, s in enumerate(docsets):
        dd, vv = first_k(s, values, k, descending)
        d[i, : dd.size], v[i, : dd.size], c[i] = dd, vv, dd.size
    return d, v, c


def blend(parts, k, descending=False):
    """A collection: parts = [(docids, values)] per source, oldest first, each sorted as first_k sorts — merged by (value, docID, source) with a STABLE sort of the
    concatenation, cut at k.  A docID that several sources deliver is listed once per source."""
    docs = np.concatenate([np.asarray(d, dtype=np.int64) for d, _ in parts]) if parts else np.zeros(0, np.int64)
    vals = np.concatenate([np.asarray(v, dtype=np.int64) for _, v in parts]) if parts else np.zeros(0, np.int64)
    key = (((HUGE - vals) if descending else vals).astype(np.uint64) << np.uint64(32)) | docs.astype(np.uint64)  # (64 unsigned bits: a value may fill its 32)
    order = np.argsort(key, kind="stable")[:k]
    return docs[order].astype(np.uint32), vals[order].astype(np.uint32)


def blend_rows(part_rows, k, descending=False):
    """[(docids, values, counts)] per source -> the collection's rows."""
    nq = len(part_rows[0][2])
    d, v, c = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)
    for q in range(nq):
        dd, vv = blend([(pd[q, : pc[q]], pv[q, : pc[q]]) for pd, pv, pc in part_rows], k, descending)
        d[q, : dd.size], v[q, : dd.size], c[q] = dd, vv, dd.size
    return d, v, c


def columns(D):
    """facet_cases' named columns and two more: `rev` — strictly decreasing: ascending, the best documents come LAST in the walk and the threshold moves to the very
    end — and `hash`: a multiplicative hash of the docID, no locality."""
    d = np.arange(D + 1, dtype=np.uint64)
    out = dict(F.columns(D))
    out["rev"] = (np.uint64(D) - d).astype(np.uint32)
    out["hash"] = ((d * np.uint64(2654435761)) & np.uint64(HUGE)).astype(np.uint32)
    return out


# ---- the groups the GPU tests run
STREAM_COLUMNS = ["mod7", "hash", "rev"]
STREAM_K = 10
WORST_COLUMNS = ["one", "rev", "huge"]  # every key ties; the threshold moves with every step; 0xffffffff on every third document
# main corpus (D = 4 SPAN_BITS + 37): an empty result; docID 1; docID D; lists of K - 1, K, K + 1 documents for K = 32 and 128; unions held as bitmaps, whose last
# window is the 37 documents past 4 SPAN_BITS
EDGE_QUERIES = ["{first1} {last1}", "{first1}", "{last1}", "{df31}", "{df32}", "{df33}", "{df127}", "{df128}", "{df129}", "{all} OR {odd}", "{odd} OR {holes}", "{all} {odd}", "{stub}",
                "{first1} OR {last1}"]  # fmt: skip
EDGE_KS = [1, 32, 128, 256]
# a corpus of its own for the kernel's sizes: single lists (one candidate tile, one task: the segment IS the list) of one below, at and one above every size k_order names
D_SIZES = 40000
SIZE_EDGES = sorted({n + x for n in (TILE, WAVE_PASS, PRUNE_AT, BUF, MAX_TOPK, WG_PASS, 2 * WG_PASS) for x in (-1, 0, 1)})
assert max(SIZE_EDGES) <= S.TILE_DOCS
TALL_QUERIES = ["{tall_odd}", "{tall_odd} OR {tall_33}", "{dense_tail3} {tall_odd}", "{beyond}", "{tall_odd} NOT {tall_33}"]
TALL_COLUMNS = ["hash", "rev", "one"]


def sizes_corpus():
    """Lists `n<size>` of SIZE_EDGES documents each, spread over 1 .. D_SIZES."""
    return S.build({"n%d" % n: (S.spread(n, D_SIZES), np.ones(n, dtype=np.int64)) for n in SIZE_EDGES}, docs_cnt=D_SIZES)


# ---- what a wrong implementation would answer -------------------------------------------------------------------------------------------------
def shifted(values):
    """The column read one docID off (values[d + 1] for d)."""
    return np.concatenate([values[1:], values[:1]])


def ties_to_the_higher_docid(docset, values, k):
    """Descending taken as the ascending sort reversed: ties in the value go to the HIGHER docID."""
    docs = np.asarray(docset, dtype=np.int64)
    v = np.asarray(values, dtype=np.uint32)[docs].astype(np.int64)
    order = np.lexsort((docs, v))[::-1][:k]
    return docs[order].astype(np.uint32), v[order].astype(np.uint32)


def signed_first_k(docset, values, k, descending=False):
    """Values compared as SIGNED 32-bit (0xffffffff as -1)."""
    docs = np.asarray(docset, dtype=np.int64)
    u = np.asarray(values, dtype=np.uint32)[docs]
    v = u.view(np.int32).astype(np.int64)
    order = np.lexsort((docs, -v if descending else v))[:k]
    return docs[order].astype(np.uint32), u[order]


def first_task_only(docset, values, k, descending=False, task_docs=S.TILE_DOCS):
    """No merge: the list of the query's FIRST task (its first task_docs documents at the most) taken as the query's."""
    return first_k(np.asarray(docset)[:task_docs], values, k, descending)
