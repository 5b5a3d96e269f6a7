"""GPU tests of the stats of a column over a COLLECTION of segments (run with -m gpu on an MI355X): tri_cbatch_stats — the parts' rows combined on the host: counts
and sums added, mins and maxs folded.  Three sources (tests/crank_cases.py's worlds: 2000, 600 and 20 documents); the expected rows are
tests/stats_cases.py::combine, source by source, of stats_rows over the CPU oracle's docID sets.  Every comparison is integer equality."""
import numpy as np
import pytest

import crank_cases as CR
import oracle_lib as O
import stats_cases as X
from test_gpu_crank import collection, masked, sources  # noqa: F401  (sources: fixture)
from test_gpu_facets_collection import unknown_to_the_newest
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
NONE = np.zeros(0, np.uint32)
# every source holds documents 1 .. 20: the same docIDs, taken once per source that delivers them — with EQUAL values (hash, low16, mod7 depend on the docID alone)
# and with DIFFERENT ones (rev = D - d: another D per source)
STATS = [(None, 0, "hash"), ("mod7", 5, "rev"), ("huge", 5, "low16"), (None, 0, "rev")]


def want_rows(progs, stats, use_masks):
    per_source, parts = [], [[] for _ in stats]
    for si, (D, *_) in enumerate(CR.WORLDS):
        ora = CR.oracle_of(si)
        ora.set_masked(CR.masks()[si] if use_masks else NONE)
        try:
            sets = [ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs]
        finally:
            ora.set_masked(NONE)
        per_source.append(sets)
        cols = X.columns(D)
        for k, (g, nb, v) in enumerate(stats):
            parts[k].append(X.stats_rows(sets, None if g is None else cols[g], nb, cols[v]))
    return [X.combine(p) for p in parts], per_source


def make_columns(T, ixs, names):
    return [{n: T.Column(ix, X.columns(D)[n]) for n in names} for ix, (D, *_) in zip(ixs, CR.WORLDS)]


def spec(cs, stats):
    return [(cs[g] if g is not None else None, nb, cs[v]) for g, nb, v in stats]


def close_all(columns):
    for cs in columns:
        for c in cs.values():
            c.close()


@pytest.mark.parametrize("use_masks", [False, True], ids=["overlapping", "masked"])
def test_rows_are_the_parts_combined(T, sources, use_masks):
    """One query names only terms the newest source does not know (its part holds empty records); without masks documents 1 .. 20 are delivered by all three sources and
    1 .. 600 by two, and are taken once per source."""
    ixs = sources(1)
    a, b = unknown_to_the_newest()
    texts = ["t0 t1", "t0 OR t1 OR t2", f"t{a} OR t{b}", f"t{a}", "t5", "t3 NOT t0", "t199 t198 t197"]
    progs = [O.parse_query(t) for t in texts]
    want, per_source = want_rows(progs, STATS, use_masks)
    assert not len(per_source[2][2]) and len(per_source[0][2]) and len(per_source[1][2])
    if not use_masks:
        assert all(1 in s.tolist() for s in (per_source[0][1], per_source[1][1], per_source[2][1]))  # the same docID in three sources
    columns = make_columns(T, ixs, ["hash", "mod7", "rev", "huge", "low16"])
    try:
        with masked(ixs, None if use_masks else [NONE] * 3), collection(T, ixs, progs, flags=T.FLAG_DOCUMENTS_ONLY) as (cb, parts):
            for p, cs in zip(parts, columns):
                p.set_stats(spec(cs, STATS))
            cb.run()
            cb.sync()
            counts = cb.counts()
            for k, s in enumerate(STATS):
                got = cb.stats(k)
                assert [x.dtype for x in got] == [np.uint64, np.uint64, np.uint32, np.uint32]
                assert X.same(got, want[k]), (s, [x.tolist() for x in got], [x.tolist() for x in want[k]])
                assert got.counts.sum(axis=1).tolist() == counts.tolist()
                assert X.same(got, X.combine([p.stats(k) for p in parts]))
            empty = parts[2].stats(0)
            assert (empty.counts[2, 0], empty.sums[2, 0], empty.mins[2, 0], empty.maxs[2, 0]) == (0, 0, X.HUGE, 0)
    finally:
        close_all(columns)


def test_parts_that_disagree_or_carry_no_stats_are_refused(T, sources):
    ixs = sources(1)
    progs = [O.parse_query(t) for t in ("t0 t1", "t5")]
    columns = make_columns(T, ixs, ["mod7", "hash"])
    try:
        with collection(T, ixs, progs, flags=T.FLAG_DOCUMENTS_ONLY) as (cb, parts):
            for i, (p, cs) in enumerate(zip(parts, columns)):
                p.set_stats([(cs["mod7"], 7 if i != 1 else 5, cs["hash"]), (cs["mod7"], 3, cs["hash"]), (None, 0, cs["hash"]) if i != 2 else (cs["mod7"], 1, cs["hash"])])
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_stats: stat 0 has 5 buckets in part 1 and 7 in part 0"):
                cb.stats(0)
            assert X.same(cb.stats(1), X.combine([p.stats(1) for p in parts]))  # (stat 1 agrees)
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_stats: stat 2 is grouped in part 2 and ungrouped in part 0"):
                cb.stats(2)
            parts[2].set_stats([(columns[2]["mod7"], 7, columns[2]["hash"])])
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_stats: part 2 carries 1 stats, part 0 carries 3"):
                cb.stats(1)
            parts[2].set_stats([])  # a part without stats
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_stats: part 2 carries 0 stats, part 0 carries 3"):
                cb.stats(1)
            for p in parts:
                p.set_stats([])
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match="no stats are set"):
                cb.stats(0)
    finally:
        close_all(columns)
