"""GPU tests of the read side (run with -m gpu on an MI355X): csrc/read_side.hpp — every result call of a batch goes through one query view, one segment walk
and one read-back rule (copies on the read-back stream, enqueued under the handle's lock, awaited outside it).  What the calls deliver is pinned against the
oracle elsewhere (test_gpu_parity.py, test_gpu_wide_terms.py, test_gpu_rank.py, ...); here: (a) a read does not depend on what is queued behind its batch on
the engine stream, (b) queries cut into many task segments read as the uncut ones do, (c) tri_decode_terms refuses a term out of range and leaves the handle
usable."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import World, options
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)
from wide_terms_cases import NARROW, NARROW_MIN, OPTS, SHAPES, WORLDS, shape_programs

pytestmark = pytest.mark.gpu
CUT = {"cand_task_cost": 4096, "dense_task_cost": 4096}  # (test_gpu_rank.py::test_many_tasks_per_query)
MODES = ["docs", "scores", "topk", "default"]


def docs_programs(V):
    """the ten queries of test_gpu_parity.py::test_docsets_delivered_as_bitmaps: both result forms occur"""
    texts = ["t0 OR t1", "t0 OR t1 OR t2 OR t3 OR t4", "t0 t1", "t0 t1 (t2 OR t3 OR t4)", "(t0 OR t1) (t2 OR t3) t4", "(t0 OR t1 OR t2) NOT t3", f"t0 OR t{V // 2} OR t{V - 1}",
             f"t{V // 2} OR t{V // 2 + 1}", "t5 t6", f"(t0 OR t{V - 2}) (t1 OR t{V - 3})"]  # fmt: skip
    return [O.parse_query(t) for t in texts]


def default_programs():
    """NARROW + or17 + or64: device rows wider than some queries report (R != nscore), and wide-report queries"""
    shapes, names = shape_programs(O), [sh[0] for sh in SHAPES]
    return [O.parse_query(t, some_min=NARROW_MIN) for t in NARROW] + [shapes[names.index("or17")], shapes[names.index("or64")]]


def make(T, w, mode):
    """-> the batch of `mode` on world w, created under the options in force (the default mode's under OPTS as well)"""
    if mode == "default":
        with options(w.dev, **OPTS):
            b = T.Batch(w.ix, default_programs(), T.FLAG_MATCHED_TERMS | T.FLAG_HIT_PAYLOADS)
        b.set_ranker(10, 3, 4.0, None)
        return b
    flags, topk = {"docs": (T.FLAG_DOCUMENTS_ONLY, 0), "scores": (T.FLAG_ACCUMULATED_SCORE, 0), "topk": (T.FLAG_ACCUMULATED_SCORE, 10)}[mode]
    return T.Batch(w.ix, docs_programs(w.V), flags, topk=topk)


def expanded(first, words):
    return np.nonzero(np.unpackbits(words.view(np.uint8), bitorder="little"))[0].astype(np.uint32) + np.uint32(first)


def read_all(b, mode, forms_as_held=True):
    """Every result call of the batch's mode -> {call: [arrays]}.  forms_as_held = False: a bitmap-form result as the docIDs it stands for (test (b): the
    form is the planner's choice per batch)."""
    counts = b.counts()
    out = {"counts": [counts]}
    n = [int(c) for c in counts]
    if mode == "topk":  # (a top-K batch keeps lists and counts, no docID sets)
        out["topk_results"] = list(b.topk_results())
        return out
    out["docset"] = [b.docset(q, n[q]) for q in range(b.nq)]
    if mode == "default":
        out["matched_terms"] = [a for q in range(len(NARROW)) for a in b.matched_terms(q, n[q])]
        assert all(a.dtype == np.uint32 for a in out["matched_terms"][1::4])  # (the narrow call: 32-bit masks)
        out["matched_terms_wide"] = [a for q in range(b.nq) for a in b.matched_terms_wide(q, n[q])]
        out["matched_payloads"] = [a for q in range(b.nq) for a in b.matched_payloads(q)]
        out["ranked"] = list(b.ranked())
        return out
    out["docsets"] = list(b.docsets())
    out["docset_hashes"] = [b.docset_hashes()]
    if mode == "scores":
        out["scores"] = [b.scores(q, n[q]) for q in range(b.nq)]
        return out
    bitmaps = [b.docset_bitmap(q) for q in range(b.nq)]
    flat, offs, forms = b.docsets_mixed()
    parts = [flat[int(offs[q]) : int(offs[q + 1])] for q in range(b.nq)]
    if forms_as_held:
        out["docset_bitmap"] = [np.array([-1 if bm is None else bm[0]], dtype=np.int64) for bm in bitmaps] + [bm[1] for bm in bitmaps if bm is not None]
        out["docsets_mixed"] = [flat[: int(offs[-1])], offs, forms]
    else:
        out["docset_bitmap"] = [expanded(*bm) for bm in bitmaps if bm is not None]
        out["docsets_mixed"] = [expanded(0, p) if f else p for p, f in zip(parts, forms)]
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for call in a:
        assert len(a[call]) == len(b[call]), (what, call)
        for i, (x, y) in enumerate(zip(a[call], b[call])):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, call, i)


@pytest.fixture(scope="module")
def worlds(T, dev):
    made = {}

    def get(key):
        if key not in made:
            made[key] = World(T, dev, *key)
        return made[key]

    yield get
    for w in made.values():
        w.ix.close()


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("mode", MODES)
def test_reads_do_not_depend_on_what_is_queued_behind_the_batch(T, worlds, mode):
    w = worlds(WORLDS[0] if mode == "default" else (20000, 500, 12, 7))
    b = make(T, w, mode)
    other = T.Batch.conjunctions(w.ix, T.gen_queries(w.V, 1337, 256, 2))  # an unrelated batch of the same index
    try:
        b.run()
        b.sync()
        info = b.info()
        if mode == "docs":
            assert 0 < info["bitmap_queries"] < b.nq  # both result forms
        if mode == "default":
            assert info["unsupported_queries"] == 0 and sum(len(t) > 16 for t in read_all(b, mode)["matched_terms_wide"][0::4]) == 2
        alone = read_all(b, mode)
        assert int(alone["counts"][0].sum()) > 0
        other.run()  # in flight behind b, not awaited ...
        behind = read_all(b, mode)
        other.sync()  # ... until every read is done
        assert_same(alone, behind, mode)
        assert int(other.counts().sum()) > 0
    finally:
        other.close()
        b.close()


# ------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("mode", MODES)
def test_queries_cut_into_many_segments_read_as_the_uncut_ones(T, dev, worlds, mode):
    """The cut is asserted on the HOST planner's plan of the same batch under the same options (trinity_amd.hostplan), as test_gpu_rank.py::test_many_tasks_per_query
    does: nothing reports what a device batch was cut into."""
    from trinity_amd import hostplan as HP

    w = worlds(WORLDS[1])
    hi = HP.HostIndex.from_segment(w.seg)
    try:
        if mode == "default":
            plan = HP.HostPlan(hi, default_programs(), T.FLAG_MATCHED_TERMS | T.FLAG_HIT_PAYLOADS, options={**OPTS, **CUT})
        else:
            flags, topk = {"docs": (T.FLAG_DOCUMENTS_ONLY, 0), "scores": (T.FLAG_ACCUMULATED_SCORE, 0), "topk": (T.FLAG_ACCUMULATED_SCORE, 10)}[mode]
            plan = HP.HostPlan(hi, docs_programs(w.V), flags, topk=topk, options=CUT)
        per_query = [int(q["ntasks"]) for q in plan.plan if q["qid"] != 0xFFFFFFFF]
        assert max(per_query) > 2, per_query
    finally:
        hi.close()
    reads = []
    for opts in ({}, CUT):
        with options(dev, **opts):
            b = make(T, w, mode)
        try:
            b.run()
            b.sync()
            reads.append(read_all(b, mode, forms_as_held=False))
        finally:
            b.close()
    assert int(reads[0]["counts"][0].sum()) > 0
    assert_same(reads[0], reads[1], mode)


# ------------------------------------------------------------------------------------------ (c)
def test_decode_terms_refuses_a_term_out_of_range_and_the_handle_stays_usable(T, worlds):
    w = worlds(WORLDS[0])
    df = [w.df(0), w.df(3)]
    with pytest.raises(T.TrinityError, match="rc=-1"):
        w.ix.decode_terms([0, w.V + 5], [df[0], 0])
    docs, freqs, offs = w.ix.decode_terms([0, 3], df)
    assert offs.tolist() == [0, df[0], df[0] + df[1]] and freqs.size == docs.size
    for i, t in enumerate((0, 3)):
        assert np.array_equal(docs[int(offs[i]) : int(offs[i + 1])], w.ora.exec(O.parse_query(f"t{t}"), O.FLAG_DOCUMENTS_ONLY)[0])
