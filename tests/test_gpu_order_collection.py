"""GPU tests of ordering by a column over a COLLECTION of segments (run with -m gpu on an MI355X): tri_cbatch_ordered — the parts' lists merged per query on the device
by (value, docID, source).  Three sources (tests/crank_cases.py's worlds: 2000, 600 and 20 documents); the expected rows are tests/order_cases.py::blend (a stable
sort) over first_k of the CPU oracle's docID sets, source by source.  Every comparison is integer equality."""
import numpy as np
import pytest

import crank_cases as CR
import oracle_lib as O
import order_cases as OC
from test_gpu_crank import collection, masked, sources  # noqa: F401  (sources: fixture)
from test_gpu_facets_collection import unknown_to_the_newest
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
NONE = np.zeros(0, np.uint32)


def source_sets(progs, use_masks):
    out = []
    for si in range(len(CR.WORLDS)):
        ora = CR.oracle_of(si)
        ora.set_masked(CR.masks()[si] if use_masks else NONE)
        try:
            out.append([ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs])
        finally:
            ora.set_masked(NONE)
    return out


def column_of(si, name):
    """`same`: one column for every source (the same docID carries EQUAL values in all of them); `own`: a hash salted by the source (different values)."""
    D = CR.WORLDS[si][0]
    if name == "own":
        d = np.arange(D + 1, dtype=np.uint64)
        return (((d + np.uint64(977 * si)) * np.uint64(2246822519)) & np.uint64(OC.HUGE)).astype(np.uint32)
    return OC.columns(D)[name]


@pytest.mark.parametrize("use_masks", [False, True], ids=["overlapping", "masked"])
@pytest.mark.parametrize("name", ["mod7", "hash", "own"])
def test_rows_are_the_blend_of_the_parts(T, sources, use_masks, name):
    """One query names only terms the newest source does not know (its part lists nothing).  Without masks documents 1 .. 20 are delivered by all three sources and
    1 .. 600 by two: listed once per source, the older source first where value and docID are equal (mod7, hash), apart where the values differ (own)."""
    ixs = sources(1)
    a, b = unknown_to_the_newest()
    texts = ["t0 t1", "t0 OR t1 OR t2", f"t{a} OR t{b}", f"t{a}", "t5", "t3 NOT t0", "t199 t198 t197"]
    progs = [O.parse_query(t) for t in texts]
    sets = source_sets(progs, use_masks)
    assert not len(sets[2][2]) and len(sets[0][2]) and len(sets[1][2])
    if not use_masks:
        assert all(1 in s[1].tolist() for s in sets)  # the same docID in three sources
    values = [column_of(si, name) for si in range(3)]
    columns = [T.Column(ix, v) for ix, v in zip(ixs, values)]
    try:
        with masked(ixs, None if use_masks else [NONE] * 3), collection(T, ixs, progs, flags=T.FLAG_DOCUMENTS_ONLY) as (cb, parts):
            for k in (10, 256):
                for desc in (False, True):
                    for p, c in zip(parts, columns):
                        p.set_order(c, k, desc)
                    cb.run()
                    cb.sync()
                    part_rows = [OC.rows(s, v, k, desc) for s, v in zip(sets, values)]
                    for p, w in zip(parts, part_rows):
                        assert all(np.array_equal(x, y) for x, y in zip(p.ordered(), w))
                    want = OC.blend_rows(part_rows, k, desc)
                    got = cb.ordered()
                    for g, w, what in zip(got, want, ("docids", "values", "counts")):
                        assert g.dtype == np.uint32 and np.array_equal(g, w), (name, k, desc, what, g.tolist()[:2], w.tolist()[:2])
                    assert got[2].tolist() == [min(k, sum(len(s[q]) for s in sets)) for q in range(len(progs))]
    finally:
        for c in columns:
            c.close()


def test_parts_that_disagree_or_lack_an_order_are_refused(T, sources):
    ixs = sources(1)
    progs = [O.parse_query(t) for t in ("t0 t1", "t5")]
    columns = [T.Column(ix, OC.columns(D)["hash"]) for ix, (D, *_) in zip(ixs, CR.WORLDS)]
    try:
        with collection(T, ixs, progs, flags=T.FLAG_DOCUMENTS_ONLY) as (cb, parts):
            launches = [p.info()["launches"] for p in parts]
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_ordered: no order is set on the parts"):
                cb.ordered()
            assert [p.info()["launches"] for p in parts] == launches  # (a collection none of whose parts has an order runs as it always did)
            counts = cb.counts().tolist()
            for i, (p, c) in enumerate(zip(parts, columns)):
                p.set_order(c, 10 if i != 1 else 5, False)
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_ordered: part 1's order has topk 5, part 0's has 10"):
                cb.ordered()
            parts[1].set_order(columns[1], 10, True)
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_ordered: part 1's order is descending, part 0's is not"):
                cb.ordered()
            parts[1].clear_order()
            cb.run()
            cb.sync()
            with pytest.raises(T.TrinityError, match=r"tri_cbatch_ordered: part 1 has no order"):
                cb.ordered()
            assert cb.counts().tolist() == counts
            parts[1].set_order(columns[1], 10, False)
            cb.run()
            cb.sync()
            d, v, n = cb.ordered()
            assert n.tolist() == [min(10, c) for c in counts]
    finally:
        for c in columns:
            c.close()
