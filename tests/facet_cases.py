"""The contract of the facet counts (include/trinity_hip.h: tri_batch_set_facets / tri_batch_facets) in plain Python, and the cases tests/test_facet_cases.py (CPU: the
cases tell a right answer from three wrong ones) and the GPU files (tests/test_gpu_facets*.py, tests/test_host_mirror_facets.py: the engine) share.

A column is a u32 array of D + 1 values (values[d] = the attribute of docID d; values[0] is never read); a facet is (column name, nbuckets); a row has nbuckets + 1
counters: row[min(values[d], nbuckets)] += 1 for every document d of the query's docID set — the last counter is the overflow bucket."""
import numpy as np

import structured as S

CONSTANTS = S.header_constants("dev_structs.hpp")
LDS_COUNTERS = CONSTANTS["FACET_LDS_COUNTERS"]  # the kernel's two thresholds (csrc/k_facet.hpp): counters per query an LDS row holds ...
SHORT_SEGMENT = CONSTANTS["FACET_SHORT_SEGMENT"]  # ... and the task segment below which it is not used
FACETS_MAX = CONSTANTS["FACETS_MAX"]
MAX_BUCKETS = CONSTANTS["FACET_MAX_BUCKETS"]
HUGE = 0xFFFFFFFF


def facet_rows(docsets, values, nbuckets):
    """[nq, nbuckets + 1] u32: per docID set the histogram of min(values[d], nbuckets)."""
    values = np.asarray(values, dtype=np.uint32)
    out = np.zeros((len(docsets), nbuckets + 1), dtype=np.uint32)
    for i, docs in enumerate(docsets):
        v = np.minimum(values[np.asarray(docs, dtype=np.int64)].astype(np.int64), nbuckets)
        out[i] = np.bincount(v, minlength=nbuckets + 1)
    return out


def columns(D):
    """The named columns over a corpus of D documents."""
    d = np.arange(D + 1, dtype=np.int64)
    huge = d % 5
    huge[d % 3 == 0] = HUGE
    return {
        "mod7": (d % 7).astype(np.uint32),
        "window": (d // S.SPAN_BITS).astype(np.uint32),
        "one": np.zeros(D + 1, dtype=np.uint32),  # every document the same value: every match of a query meets on ONE counter
        "low16": (d & 0xFFFF).astype(np.uint32),
        "huge": huge.astype(np.uint32),  # 0xffffffff on every third document: the overflow bucket
    }


def fits(name, D):
    """A bucket count that holds every value of the column (`huge`: every value but 0xffffffff)."""
    return {"mod7": 7, "window": D // S.SPAN_BITS + 1, "one": 1, "low16": min(D + 1, 65536), "huge": 5}[name]


# ---- the facets the GPU tests count, by group: (column, nbuckets) — nbuckets None: fits(column, D)
STREAM_FACETS = [("mod7", 7), ("mod7", 5), ("window", None), ("one", None), ("low16", None), ("huge", None)]
# one below / at / one above the LDS budget (a single facet of nbuckets has nbuckets + 1 counters), and the largest row there is
THRESHOLD_FACETS = [("low16", LDS_COUNTERS - 2), ("low16", LDS_COUNTERS - 1), ("low16", LDS_COUNTERS), ("low16", MAX_BUCKETS)]
FOUR_ON_CHIP = [("mod7", 7), ("low16", 4000), ("window", 2), ("huge", 5)]  # 8 + 4001 + 3 + 6 counters: inside the budget together
FOUR_DIRECT = [("mod7", 5), ("low16", LDS_COUNTERS - 1), ("one", 1), ("huge", 5)]  # the second alone fills the budget: together they take global atomics
assert sum(nb + 1 for _, nb in FOUR_ON_CHIP) <= LDS_COUNTERS < sum(nb + 1 for _, nb in FOUR_DIRECT) and len(FOUR_ON_CHIP) == len(FOUR_DIRECT) == FACETS_MAX
TALL_FACETS = [("one", None), ("window", None)]
TALL_QUERIES = ["{tall_odd}", "{tall_odd} OR {tall_33}", "{dense_tail3} {tall_odd}", "{beyond}", "{tall_odd} NOT {tall_33}"]
# main corpus (D = 4 SPAN_BITS + 37: the last window is partial).  An empty result; one match at docID 1 and one at D; single lists of SHORT_SEGMENT - 1, SHORT_SEGMENT and
# SHORT_SEGMENT + 1 documents (one candidate tile, one task: the segment IS the list); unions held as bitmaps, whose last window is the 37 documents past 4 SPAN_BITS
EDGE_QUERIES = ["{first1} {last1}", "{first1}", "{last1}", "{df%d}" % (SHORT_SEGMENT - 1), "{df%d}" % SHORT_SEGMENT, "{df%d}" % (SHORT_SEGMENT + 1), "{all} OR {odd}", "{odd} OR {holes}", "{all} {odd}",
                "{stub}"]  # fmt: skip
EDGE_FACETS = [("mod7", 1), ("window", 4), ("huge", None), ("low16", None)]  # (mod7 at ONE bucket: documents 1 and D overflow; window at 4: the partial last window does)
# ... the same with low16 at 4000 buckets: the four rows fit the LDS budget together, so a segment's length alone decides the regime — SHORT_SEGMENT - 1 goes direct,
# SHORT_SEGMENT and SHORT_SEGMENT + 1 on chip.  EDGE_FACETS (65 536 buckets of low16) is the direct variant of every edge
EDGE_FACETS_ON_CHIP = [("mod7", 1), ("window", 4), ("huge", 5), ("low16", 4000)]
assert all(n in S.DF_EDGES for n in (SHORT_SEGMENT - 1, SHORT_SEGMENT, SHORT_SEGMENT + 1))


def resolve(facets, D):
    return [(name, fits(name, D) if nb is None else nb) for name, nb in facets]


def stream_masked(D=S.D_STREAM):
    """The masked set of the stream corpus' mask test: the window edges and every 11th document."""
    edges = [1, D] + [k * S.SPAN_BITS + x for k in range(1, D // S.SPAN_BITS + 1) for x in (-1, 0, 1)]
    return np.unique(np.concatenate([np.array([e for e in edges if 1 <= e <= D], dtype=np.int64), np.arange(11, D + 1, 11)])).astype(np.uint32)


def _scatter(D, mul, shift, mod):
    """A docID's class under a multiplicative hash: spread evenly over every list of the corpora, whose documents are arithmetic progressions."""
    d = np.arange(1, D + 1, dtype=np.uint64)
    return d.astype(np.uint32), (((d * np.uint64(mul)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)) % np.uint64(mod)


def stream_filter_drops(D=S.D_STREAM):
    """The documents each of the three filters of the filter test drops: a quarter, a third, a fifth of 1 .. D, scattered."""
    return [d[h == 0] for d, h in (_scatter(D, 2654435761, 7, 4), _scatter(D, 40503, 3, 3), _scatter(D, 2246822519, 11, 5))]


def stream_filters(D=S.D_STREAM):
    """Three filters for one batch, of both polarities, as (docids, keep); query q names filter q % 3.  The third is handed over as its allow-list."""
    a, b, c = stream_filter_drops(D)
    return [(a, False), (b, False), (np.setdiff1d(np.arange(1, D + 1, dtype=np.uint32), c).astype(np.uint32), True)]


# ---- what a wrong implementation would answer -------------------------------------------------------------------------------------------------
def shifted(values):
    """The column read one docID off (values[d + 1] for d)."""
    return np.concatenate([values[1:], values[:1]])


def clamped_rows(docsets, values, nbuckets):
    """Values clamped into the LAST REAL bucket (nbuckets - 1) instead of counted as overflow."""
    rows = facet_rows(docsets, values, nbuckets)
    rows[:, nbuckets - 1] += rows[:, nbuckets]
    rows[:, nbuckets] = 0
    return rows
