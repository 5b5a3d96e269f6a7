"""GPU tests of the facet counts over a COLLECTION of segments (run with -m gpu on an MI355X): tri_cbatch_facets — the parts' rows widened and summed.  Three sources
(tests/crank_cases.py's worlds: 2000, 600 and 20 documents); the expected rows are the sum, source by source, of tests/facet_cases.py::facet_rows over the CPU oracle's
docID sets.  Every comparison is integer equality."""
import numpy as np
import pytest

import crank_cases as CR
import facet_cases as F
import oracle_lib as O
from test_gpu_crank import collection, masked, sources  # noqa: F401  (sources: fixture)
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
NONE = np.zeros(0, np.uint32)
FACETS = [("mod7", 5), ("huge", 5), ("low16", 16)]  # (every source holds documents 1 .. 20: the same docIDs, counted once per source that delivers them)


def unknown_to_the_newest():
    """Two terms the two older sources hold and the newest (20 documents) does not."""
    df = [CR.oracle_of(si).terms()[:, 0] for si in range(3)]
    out = [t for t in range(len(df[2])) if df[2][t] == 0 and df[0][t] > 20 and df[1][t] > 5]
    assert len(out) >= 2
    return out[:2]


def want_rows(progs, facets, use_masks):
    total = [np.zeros((len(progs), nb + 1), dtype=np.uint64) for _, nb in facets]
    per_source = []
    for si, (D, *_) in enumerate(CR.WORLDS):
        ora = CR.oracle_of(si)
        ora.set_masked(CR.masks()[si] if use_masks else NONE)
        try:
            sets = [ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs]
        finally:
            ora.set_masked(NONE)
        per_source.append(sets)
        cols = F.columns(D)
        for k, (name, nb) in enumerate(facets):
            total[k] += F.facet_rows(sets, cols[name], nb)
    return total, per_source


@pytest.mark.parametrize("use_masks", [False, True], ids=["overlapping", "masked"])
def test_rows_are_the_sum_of_the_parts(T, sources, use_masks):
    """One query names only terms the newest source does not know (its part counts nothing); without masks documents 1 .. 20 are delivered by all three sources and
    1 .. 600 by two, and are counted once per source."""
    ixs = sources(1)
    a, b = unknown_to_the_newest()
    texts = ["t0 t1", "t0 OR t1 OR t2", f"t{a} OR t{b}", f"t{a}", "t5", "t3 NOT t0", "t199 t198 t197"]
    progs = [O.parse_query(t) for t in texts]
    want, per_source = want_rows(progs, FACETS, use_masks)
    assert not len(per_source[2][2]) and len(per_source[0][2]) and len(per_source[1][2])
    if not use_masks:
        assert all(1 in s.tolist() for s in (per_source[0][1], per_source[1][1], per_source[2][1]))  # the same docID in three sources
    columns = [[T.Column(ix, F.columns(D)[name]) for name, _ in FACETS] for ix, (D, *_) in zip(ixs, CR.WORLDS)]
    try:
        with masked(ixs, None if use_masks else [NONE] * 3), collection(T, ixs, progs, flags=T.FLAG_DOCUMENTS_ONLY) as (cb, parts):
            for p, cs in zip(parts, columns):
                p.set_facets([(c, nb) for c, (_, nb) in zip(cs, FACETS)])
            cb.run()
            cb.sync()
            counts = cb.counts()
            for k, (name, nb) in enumerate(FACETS):
                got = cb.facets(k)
                assert got.dtype == np.uint64 and np.array_equal(got, want[k]), (name, nb, got.tolist(), want[k].tolist())
                assert got.sum(axis=1).tolist() == counts.tolist()
                parts_sum = sum(p.facets(k).astype(np.uint64) for p in parts)
                assert np.array_equal(parts_sum, got)
            assert not parts[2].facets(0)[2].any() and not parts[2].facets(0)[3].any()
    finally:
        for cs in columns:
            for c in cs:
                c.close()


def test_parts_that_disagree_are_refused(T, sources):
    ixs = sources(1)
    progs = [O.parse_query(t) for t in ("t0 t1", "t5")]
    columns = [T.Column(ix, F.columns(D)["mod7"]) for ix, (D, *_) in zip(ixs, CR.WORLDS)]
    try:
        with collection(T, ixs, progs, flags=T.FLAG_DOCUMENTS_ONLY) as (cb, parts):
            for i, (p, c) in enumerate(zip(parts, columns)):
                p.set_facets([(c, 7 if i != 1 else 5), (c, 3)])
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_facets: facet 0 has 5 buckets in part 1 and 7 in part 0"):
                cb.facets(0)
            assert np.array_equal(cb.facets(1), sum(p.facets(1).astype(np.uint64) for p in parts))  # (facet 1 agrees)
            parts[2].set_facets([(columns[2], 7)])
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_facets: part 2 carries 1 facets, part 0 carries 2"):
                cb.facets(1)
            for p in parts:
                p.set_facets([])
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match="no facets are set"):
                cb.facets(0)
    finally:
        for c in columns:
            c.close()
