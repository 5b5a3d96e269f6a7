"""The contract of the stats of a column (include/trinity_hip.h: tri_batch_set_stats / tri_batch_stats / tri_cbatch_stats) in plain numpy, and the cases
tests/test_stats_cases.py (CPU: the cases tell a right answer from seven wrong ones) and the GPU files (tests/test_gpu_stats*.py, tests/test_host_mirror_stats.py: the
engine) share.

A column is a u32 array of D + 1 values (values[d] = the attribute of docID d; values[0] is never read); a stat is (group column name or None, nbuckets, value column
name); a grouped row has nbuckets + 1 records, an ungrouped one (nbuckets 0) a single record.  For every document d of the query's docID set the record of bucket
min(group[d], nbuckets) takes the document: count += 1, sum += value[d] (u64), min and max folded, unsigned — the last record is the overflow bucket; an empty
record reads count 0, sum 0, min 0xffffffff, max 0."""
import collections

import numpy as np

import facet_cases as F
import order_cases as OC
import structured as S

CONSTANTS = S.header_constants("dev_structs.hpp")
LDS_BUCKETS = CONSTANTS["STATS_LDS_BUCKETS"]  # the kernel's two thresholds (csrc/k_stats.hpp): records per query (all grouped stats) the LDS planes hold ...
SHORT_SEGMENT = CONSTANTS["STATS_SHORT_SEGMENT"]  # ... and the task segment below which they are not used
STATS_MAX = CONSTANTS["STATS_MAX"]
MAX_BUCKETS = CONSTANTS["FACET_MAX_BUCKETS"]
WG = CONSTANTS["STATS_WG"]
HUGE = 0xFFFFFFFF

Stats = collections.namedtuple("Stats", "sums counts mins maxs")
columns = OC.columns  # facet_cases' named columns and order_cases' `rev` and `hash`


def stats_rows(docsets, group, nbuckets, value):
    """Stats(sums u64, counts u32, mins u32, maxs u32), each [nq, nbuckets + 1]; group None: nbuckets must be 0."""
    assert group is not None or nbuckets == 0
    value = np.asarray(value, dtype=np.uint32)
    w = nbuckets + 1
    out = Stats(np.zeros((len(docsets), w), np.uint64), np.zeros((len(docsets), w), np.uint32), np.full((len(docsets), w), HUGE, np.uint32), np.zeros((len(docsets), w), np.uint32))
    for i, docs in enumerate(docsets):
        docs = np.asarray(docs, dtype=np.int64)
        g = np.zeros(docs.size, np.int64) if group is None else np.minimum(np.asarray(group, dtype=np.uint32)[docs].astype(np.int64), nbuckets)
        v = value[docs]
        out.counts[i] = np.bincount(g, minlength=w)
        np.add.at(out.sums[i], g, v.astype(np.uint64))  # (exact 64-bit integer adds)
        np.minimum.at(out.mins[i], g, v)
        np.maximum.at(out.maxs[i], g, v)
    return out


def combine(parts):
    """A collection: the parts' Stats combined — counts (widened) and sums added, mins and maxs folded.  Raises OverflowError, naming (query, bucket), when a sum
    would wrap 64 bits."""
    sums = np.zeros(parts[0].sums.shape, dtype=object)
    for p in parts:
        sums = sums + p.sums.astype(object)
    bad = np.argwhere(sums >= (1 << 64))
    if bad.size:
        raise OverflowError("query %d, bucket %d" % tuple(bad[0]))
    return Stats(sums.astype(np.uint64), sum(p.counts.astype(np.uint64) for p in parts), np.minimum.reduce([p.mins for p in parts]), np.maximum.reduce([p.maxs for p in parts]))


def fits(name, D):
    """A bucket count that holds every value of the group column (`huge`: every value but 0xffffffff; `rev` and `hash` fit nothing: 64 buckets, the rest overflows)."""
    return {"rev": 64, "hash": 64}.get(name) or F.fits(name, D)


def resolve(stats, D):
    return [(g, 0 if g is None else fits(g, D) if nb is None else nb, v) for g, nb, v in stats]


def lds_records(stats):
    """Records per query of the grouped stats: what the kernel holds against STATS_LDS_BUCKETS."""
    return sum(nb + 1 for g, nb, _ in stats if g is not None)


def regime(stats, segment):
    """Per stat the regime a single-task segment of `segment` matches takes: 'registers', 'on chip' or 'direct'."""
    chip = lds_records(stats) <= LDS_BUCKETS and segment >= SHORT_SEGMENT
    return ["registers" if g is None else "on chip" if chip else "direct" for g, _, _ in stats]


# ---- the stats the GPU tests run, by group: (group column or None, nbuckets — None: fits(group, D) —, value column)
STREAM_STATS = [(None, 0, "hash"), ("mod7", 5, "rev")]  # one ungrouped and one grouped together: mod7 at 5 buckets overflows, hash sums pass 2^32
# records one below / at / one above the LDS budget (a single grouped stat of nbuckets has nbuckets + 1 records), and the largest row there is
THRESHOLD_STATS = [("low16", LDS_BUCKETS - 2, "hash"), ("low16", LDS_BUCKETS - 1, "hash"), ("low16", LDS_BUCKETS, "hash"), ("low16", MAX_BUCKETS, "hash")]
FOUR_ON_CHIP = [("mod7", 7, "hash"), ("low16", LDS_BUCKETS - 100, "rev"), ("window", 2, "huge"), ("huge", 5, "low16")]  # 8 + 701 + 3 + 6 records: inside the budget together
FOUR_DIRECT = [("mod7", 5, "hash"), ("low16", LDS_BUCKETS - 1, "rev"), ("one", 1, "huge"), ("huge", 5, "low16")]  # the second alone fills the budget
MIXED_ON_CHIP = [(None, 0, "rev"), ("mod7", 5, "hash"), (None, 0, "huge")]  # registers + on chip in one launch
MIXED_DIRECT = [(None, 0, "hash"), ("low16", LDS_BUCKETS, "rev"), (None, 0, "mod7")]  # registers + direct
assert lds_records(FOUR_ON_CHIP) <= LDS_BUCKETS < lds_records(FOUR_DIRECT) and len(FOUR_ON_CHIP) == len(FOUR_DIRECT) == STATS_MAX
assert lds_records(MIXED_ON_CHIP) <= LDS_BUCKETS < lds_records(MIXED_DIRECT)
# `one`, `huge`, `rev` and `hash` as group and as value — one: every match of a query lands on ONE record; huge: the overflow bucket and sums past 2^32; rev: strictly
# decreasing, so in the walk's order max stands and min moves at every step (and as a group nearly everything overflows); hash: no locality
AS_GROUPS = [("one", 1, "huge"), ("huge", 5, "rev"), ("rev", None, "hash"), ("hash", None, "one")]
AS_VALUES = [(None, 0, "one"), (None, 0, "huge"), (None, 0, "rev"), (None, 0, "hash")]
TALL_STATS = [(None, 0, "hash"), ("one", 1, "rev"), ("mod7", 7, "huge")]  # a million matches a query, many tasks: every task's flush meets the others in one row
TALL_QUERIES = F.TALL_QUERIES
# main corpus (D = 4 SPAN_BITS + 37): facet_cases' edges — an empty result; docID 1; docID D; single-task segments of SHORT_SEGMENT - 1, SHORT_SEGMENT, SHORT_SEGMENT + 1
# documents; unions held as bitmaps whose last window is partial.  Once with rows that fit the budget (the segment's length alone decides the regime), once with a row
# that does not (low16 at 65 536 buckets)
EDGE_QUERIES = F.EDGE_QUERIES
EDGE_STATS_ON_CHIP = [(None, 0, "hash"), ("mod7", 1, "rev"), ("window", 4, "huge"), ("low16", LDS_BUCKETS - 100, "hash")]
EDGE_STATS_DIRECT = [(None, 0, "hash"), ("mod7", 1, "rev"), ("window", 4, "huge"), ("low16", None, "hash")]
assert SHORT_SEGMENT == F.SHORT_SEGMENT and all(n in S.DF_EDGES for n in (SHORT_SEGMENT - 1, SHORT_SEGMENT, SHORT_SEGMENT + 1))
# the ungrouped path's sizes on order_cases.sizes_corpus(): single-task segments one below, at and one above a wave (64) and a workgroup (256).  The segment of ONE
# document is the edges' {first1} and {last1} (sizes_corpus has no list of one)
SIZE_QUERIES = [63, 64, 65, WG - 1, WG, WG + 1]
SIZE_STATS = [(None, 0, "hash"), (None, 0, "rev"), ("mod7", 5, "hash")]
assert all(n in OC.SIZE_EDGES for n in SIZE_QUERIES)
MASK_STATS = [(None, 0, "hash"), ("mod7", 5, "rev"), ("window", None, "huge"), ("huge", None, "low16")]
stream_masked, stream_filter_drops, stream_filters = F.stream_masked, F.stream_filter_drops, F.stream_filters


# ---- what a wrong implementation would answer -------------------------------------------------------------------------------------------------
def shifted(values):
    """The column read one docID off (values[d + 1] for d)."""
    return np.concatenate([values[1:], values[:1]])


def swapped(docsets, group, nbuckets, value):
    """Group and value columns swapped."""
    return stats_rows(docsets, value, nbuckets, group)


def sums32(rows):
    """The sum kept in 32 bits."""
    return rows._replace(sums=rows.sums & np.uint64(HUGE))


def mins_zeroed(rows):
    """The mins plane zero-initialised: every min folds to 0."""
    return rows._replace(mins=np.zeros_like(rows.mins))


def clamped(docsets, group, nbuckets, value):
    """Groups clamped into the LAST REAL bucket (nbuckets - 1) instead of the overflow bucket."""
    return stats_rows(docsets, np.minimum(np.asarray(group, dtype=np.uint32), nbuckets - 1), nbuckets, value)


def first_task_only(docsets, group, nbuckets, value, task_docs=S.TILE_DOCS):
    """No merge across tasks: the records of the query's FIRST task (its first task_docs documents at the most) taken as the query's."""
    return stats_rows([np.asarray(s)[:task_docs] for s in docsets], group, nbuckets, value)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))
