"""The ranked list of a COLLECTION of segments (tri_cbatch_ranked, ProximityRanker::blend) restated over the CPU oracle — a helper module, imported by
tests/test_crank_cases.py, tests/test_gpu_crank.py and tests/test_host_mirror_collection.py.  Nothing here comes from the engine: per source the ranking is
rank_cases.rows over oracle_lib.Index.exec_rich with the source's mask installed; the collection's list is those rankings concatenated source after source, sorted
STABLY by (-score, docID) and cut to K — so two sources that hold the same docID at the same score both stay, the older source's entry first.

The collection: three oracle worlds over one vocabulary, oldest first.  Each newer source re-indexes documents 1 .. its own size, so source 0 is masked by
documents 1 .. 600 and source 1 by 1 .. 20.  (The newest source is this small so that one of the test queries matches nothing in it: at 200 documents of ten
tokens every narrow query matches in every source, whatever the seed.)"""
import numpy as np

import oracle_lib as O
import rank_cases as R

WORLDS = [(2000, 200, 10, 42), (600, 200, 10, 7), (20, 200, 10, 23)]
UPDATES = [0, 600, 20]  # source i re-indexes documents 1 .. UPDATES[i] of the older sources
K, CAP, ADJ = 10, 3, 4.0
# (tests/test_gpu_rank.py's PAIR_QUERIES, restated here so that the CPU tests do not import a GPU module; tests/test_gpu_crank.py asserts they are the same)
PAIR_QUERIES = ["t0 t1", "t0 OR t1 OR t2", '"t0 t1" OR "t1 t2" OR "t2 t3"', 't0 <"t1 t2">', "[t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11]"]

_ORA, _RECS = {}, {}


def w3(k):
    return 1 + k % 3


def masks(n=len(WORLDS)):
    """Per source: the documents the newer sources update (ascending u32)."""
    return [np.arange(1, max(UPDATES[i + 1 : n], default=0) + 1, dtype=np.uint32) for i in range(n)]


def oracle_of(si):
    if si not in _ORA:
        _ORA[si] = O.Index.generate(*WORLDS[si])
    return _ORA[si]


def recs_of(si, prog, masked=True, n=len(WORLDS)):
    """Source si's default-mode records of the query, under its mask of an n-source collection (masked = False: none installed)"""
    key = (si, masked, n, np.asarray(prog, dtype=np.uint32).tobytes())
    if key not in _RECS:
        ora = oracle_of(si)
        ora.set_masked(masks(n)[si] if masked else np.zeros(0, np.uint32))
        try:
            _RECS[key] = R.records(ora.exec_rich(prog)[1])
        finally:
            ora.set_masked(np.zeros(0, np.uint32))
    return _RECS[key]


def present_slots(si, prog):
    """Source si's slots of the query, [(term, token that carries its weight)]: the program's slots (rank_cases.slots) without the terms that have no documents in
    the source's term table — a source reports, and ranks by, the terms it knows (tri_batch_query_terms on its part), so two terms next to each other there may be
    apart in the program."""
    df = oracle_of(si).terms()[:, 0]
    return [(t, tok) for t, tok in zip(*R.slots(prog)) if t < len(df) and df[t]]


def source_rows(prog, cap, adj, fn, masked=True, n=len(WORLDS)):
    """Per source its whole ranking [(doc, score, pairs)], score descending, docID ascending, under weights fn(slot of the program) (None: 1.0): rank_cases' score
    over the source's own slots (rank_cases.rows where the source knows every term of the query)"""
    tokw = None if fn is None else R.token_weights([prog], fn)
    out = []
    for si in range(n):
        ps = present_slots(si, prog)
        st = [t for t, _ in ps]
        w = [1.0 if tokw is None else tokw[tok] for _, tok in ps]
        rows = [(doc, R.score(terms, st, w, cap, adj), R.pairs_of(terms, st)) for doc, terms in recs_of(si, prog, masked, n)]
        out.append(sorted(rows, key=lambda r: (-r[1], r[0])))
    return out


def blend(lists, K):
    """[(doc, score, ..., source)] — the sources' lists one after the other, sorted stably by (-score, docID), cut to K"""
    allrows = [tuple(r) + (si,) for si, rows in enumerate(lists) for r in rows]
    return sorted(allrows, key=lambda r: (-r[1], r[0]))[:K]


def want(prog, K, cap, adj, fn, masked=True, n=len(WORLDS)):
    """The collection's expected list of one query: [(doc, score, pairs, source)], at most K.  (Each source's list cut to K first changes nothing: an entry past a
    source's K-th has K entries of its own source before it.)"""
    return blend(source_rows(prog, cap, adj, fn, masked, n), K)


def bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])
