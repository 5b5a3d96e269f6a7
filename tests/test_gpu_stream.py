"""GPU tests of the index's PLANE CACHE across a stream of batches (run with -m gpu on an MI355X): growth, reuse, overlap.

Every other GPU test handles a batch as create, run, sync, read, close, on an index whose plane cache is in whatever state earlier tests left it.  The engine's callers
keep several batches in flight on one index, and the cache (tri_index::planes: plane 0, the high region and the phrase rank records) is mutable state shared by all of them:
PlaneCache::fit grows it without draining the engine stream, run_plane_rows builds only the rows whose parts are missing, run_phrases adds rank records row by row,
tri_index_set_masked swaps the mask between runs.  A wrong copy length, a stale `built` bit or a mis-ordered event there gives wrong docID sets or scores, not a crash.

Each test here drives a SEQUENCE of batches over ONE FRESHLY UPLOADED index of the `stream` corpus (tests/structured.py: twelve head terms of pairwise distinct
document frequencies, so a term's plane row — its df rank — is known; frequencies through FREQ_CYCLE, so a row's high part differs from its plane 0; written positions
for phrases), so the cache's state is known at every step, and checks EVERY batch of the sequence:
  * docID sets, counts and FNV hashes against structured.Corpus.evaluate (numpy over the postings, no codec);
  * top-K against the oracle over the GOOGLE bytes, through structured.check_topk at structured.RTOL;
  * Batch.info()["term_planes_decoded_bytes"] — the list bytes of the rows a run had to build — against a model of the cache kept beside the sequence (`Cache`): it
    equals the sum of Index.term_docbytes over exactly the rows whose needed parts no earlier run built.  (Asserted only without TRINITY_TEST_OPTIONS, as in
    test_gpu_structured.py; the results are always asserted.)

The capacity of the cache is set per batch: options(plane_div=ALL_PLANES, plane_max_bytes=N * PL_PLANES * plw * 4) plans a batch with exactly N eligible rows, df ranks
0 .. N - 1 (planner.hpp: eligible_planes).

Before its sequence every test builds the cache of a DECOY (every other document of every list: the same docID space and df ranks) at each of its capacities and closes
it: the device handle's buffer pool hands a growth the idle buffer of the best-fitting size, and without the decoy that is the cache of the previous test — the right rows
of the same corpus, which would hide a lost copy.

Top-K comparison as in test_gpu_structured.py.  Measured on the oracle by tests/test_structured.py::test_score_gap_condition with the `stream` corpus included: 5.0 %
of the scored (query, K, similarity) cases fall under the set-wise rule (bound: 10 %; 4.2 % before this corpus); the smallest relative gap between distinct scores is
3.1e-11.

One device handle for the file; every index is uploaded inside its test and closed, with its batches, when the test ends (the `stream` fixture's teardown, a `finally`
in the last test); nothing sleeps, retries or loops over a timing."""
import numpy as np
import pytest

import oracle_lib as O
import structured as S
from test_gpu_structured import OVERRIDDEN, SWorld, T, dev, options  # noqa: F401  (T, dev: fixtures)

pytestmark = pytest.mark.gpu

HEADS = S.STREAM_HEADS
FULL = len(HEADS)  # rows of the cache at full capacity: every head term, no rare one
PLW = ((S.D_STREAM >> 17) + 2) * (S.SPAN_BITS // 32)  # words of a plane (planner.hpp: eligible_planes)
ONEPASS = {"dense_min_postings": 0}  # every eligible scored query through k_planes: each head term a one-pass slot, which always gets a plane; reads the high parts
SCORE = {"fused": 0, "planes": 3}  # match, then score: k_score reads the level words of the rows
SIMS = (O.SIM_BM25, O.SIM_TFIDF, O.SIM_TRIVIAL)


PL_PLANES = S.header_constants("dev_structs.hpp")["PL_PLANES"]  # bitmaps of a whole plane row: plane 0 + the high part


def capacity(n):
    """The options under which a batch is planned with exactly n eligible rows, df ranks 0 .. n - 1."""
    return {"plane_div": S.ALL_PLANES, "plane_max_bytes": n * PL_PLANES * PLW * 4}


def test_capacity_mirrors_the_header():
    assert PL_PLANES == 7 and PLW == 4 * 4096 and capacity(2)["plane_max_bytes"] == 2 * 7 * PLW * 4


# ------------------------------------------------------------------------------------------ the references, once per module
@pytest.fixture(scope="module")
def ref():
    """The corpus, a decoy of the same docID space, and the caches of numpy sets and oracle scores every test's SWorld shares (computed once, never changed)."""

    class Ref:
        pass

    r = Ref()
    r.c = S.stream_corpus()
    # the decoy: every other document of every list, frequency 3 — the same df ranks and docID space, rows that are SUBSETS of the corpus' rows (a stale decoy row
    # names no document that the corpus' list does not hold: the kernels look a plane's candidates up in the lists)
    r.decoy = S.build({n: (r.c.lists[n][0][::2], np.full(r.c.lists[n][0][::2].size, 3)) for n in r.c.names})
    assert r.decoy.D == r.c.D == S.D_STREAM and np.all(np.diff(r.decoy.df()[:FULL]) < 0)
    r.want, r.scores = {}, {}
    r.masked = np.unique(np.concatenate([[1, S.D_STREAM], [b + x for b in (S.SPAN_BITS, 2 * S.SPAN_BITS) for x in (-1, 0, 1)], np.arange(70000, 70300)])).astype(np.uint32)
    return r


def first_difference(got, want):
    n = min(len(got), len(want))
    at = np.nonzero(np.asarray(got[:n]) != np.asarray(want[:n]))[0]
    i = int(at[0]) if at.size else n
    return {"at": i, "got": int(got[i]) if i < len(got) else None, "want": int(want[i]) if i < len(want) else None, "len_got": len(got), "len_want": len(want)}


class Cache:
    """A model of the index's plane cache, kept beside the sequence: per row, the parts (bit 0: plane 0, bit 1: the high part) that the runs enqueued so far have
    CERTAINLY built (`sure`) and have POSSIBLY built (`maybe`: a batch whose planner chose only some of the terms it names — info()["plane_terms"] says how many, not
    which).  expect() answers the bounds of term_planes_decoded_bytes of the next run — equal, whenever every batch so far named exactly the rows it chose."""

    def __init__(self, docbytes):
        self.docbytes, self.sure, self.maybe = docbytes, {}, {}

    def expect(self, rows, needs, exact, rebuild=False):
        lo = sum(self.docbytes[r] for r in rows if rebuild or (self.maybe.get(r, 0) & needs) != needs) if exact else 0
        hi = sum(self.docbytes[r] for r in rows if rebuild or (self.sure.get(r, 0) & needs) != needs)
        for r in rows:
            self.maybe[r] = self.maybe.get(r, 0) | needs
            if exact:
                self.sure[r] = self.sure.get(r, 0) | needs
        return lo, hi

    def phrase_rows(self, rows):
        """run_phrases (GOOGLE) builds plane 0 with the rank records of the phrase terms' rows that have none."""
        for r in rows:
            self.sure[r] = self.sure.get(r, 0) | 1
            self.maybe[r] = self.maybe.get(r, 0) | 1


class Job:
    """One batch of a sequence: created under its options, run (perhaps several times), checked after its sync."""

    def __init__(self, st, tag, kind, names, cap, k, sim, opts, masked):
        self.st, self.tag, self.kind, self.k, self.sim, self.masked = st, tag, kind, k, sim, masked
        c, w = st.w.c, st.w
        self.queries = {"docs": S.stream_docs_queries, "scored": S.stream_scored_queries, "phrase": S.stream_phrase_queries, "phrase_scored": S.stream_phrase_queries}[kind](c, names)
        self.scored = kind in ("scored", "phrase_scored")
        self.key = ("phrase" if "phrase" in kind else "docs", tuple(names))  # (the scored tables name the same queries)
        self.progs, self.want, self.hashes = w.want(self.key, self.queries)
        with options(w.dev, **dict(capacity(cap) if cap else {}, **opts)):
            self.b = w.T.Batch(w.ix, self.progs, w.T.FLAG_ACCUMULATED_SCORE if self.scored else w.T.FLAG_DOCUMENTS_ONLY, topk=k, similarity=sim)
        st.jobs.append(self)
        info = self.b.info()
        assert info["unsupported_queries"] == 0, tag
        # the rows the batch may build: the head terms it names that are eligible under its capacity; the planner chose info["plane_terms"] of them
        self.rows = sorted({HEADS.index(n) for n in names if n in HEADS and HEADS.index(n) < (cap or FULL)})
        self.exact = info["plane_terms"] == len(self.rows)
        self.high = info["plane_terms"] > 0 and info["plane_bytes"] == info["plane_terms"] * PL_PLANES * PLW * 4
        self.phrase_rows = sorted({HEADS.index(n) for n in names if n in S.STREAM_PHRASE_HEADS}) if "phrase" in kind else []
        if not OVERRIDDEN:
            assert info["plane_terms"] <= len(self.rows) and info["plane_bytes"] == info["plane_terms"] * (PL_PLANES if self.high else 1) * PLW * 4, (tag, info["plane_terms"], info["plane_bytes"])
            assert self.high == (self.scored and info["plane_terms"] > 0), (tag, info["plane_bytes"], info["plane_terms"])  # (a scored batch reads the high parts of its rows)
            if "phrase" not in kind:
                assert self.exact, (tag, info["plane_terms"], self.rows)  # (tests/test_structured.py::test_routing: these tables' head terms are all chosen)
            if info["plane_terms"]:
                st.cap = max(st.cap, cap or FULL)

    def run(self, rebuild=False):
        """Enqueues a run; returns what it decoded and asserts it against the cache's model."""
        self.b.run()
        decoded = self.b.info()["term_planes_decoded_bytes"]  # (counted on the host when the run is enqueued)
        if not OVERRIDDEN:
            lo, hi = self.st.cache.expect(self.rows, 3 if self.high else 1, self.exact, rebuild)
            assert lo <= decoded <= hi, (self.tag, "decoded", decoded, "expected", lo, hi, self.rows)
            if self.st.w.codec == 1 and self.st.cap:
                self.st.cache.phrase_rows([r for r in self.phrase_rows if r < self.st.cap])
        return decoded

    def check(self):
        """After the sync: every query of the batch against the reference."""
        w, b = self.st.w, self.b
        b.sync()
        counts = b.counts()
        M = self.masked
        if not self.scored:
            hashes = b.docset_hashes()
            total = 0
            for i, (text, mn) in enumerate(self.queries):
                exp = self.want[i] if M is None else self.want[i][~np.isin(self.want[i], M)]
                got = b.docset(i, int(counts[i]))
                assert np.array_equal(got, exp), (self.tag, w.codec, text, first_difference(got, exp))
                assert int(hashes[i]) == (self.hashes[i] if M is None else O.fnv1a_docs(exp)), (self.tag, w.codec, text)
                total += len(exp)
            assert b.info()["matches"] == total, (self.tag, b.info()["matches"], total)
            return
        refs = w.scores((self.key, self.sim, M is not None), self.progs, self.sim, M)
        d, s, c = b.topk_results()
        for i, (text, mn) in enumerate(self.queries):
            docs, scores = refs[i]
            nwant = len(self.want[i]) if M is None else int((~np.isin(self.want[i], M)).sum())
            assert int(counts[i]) == nwant == len(docs), (self.tag, w.codec, text, int(counts[i]), nwant, len(docs))
            assert int(c[i]) == min(self.k, len(docs)), (self.tag, w.codec, text)
            S.check_topk(d[i, : int(c[i])], s[i, : int(c[i])], docs, scores, self.k, w.ora, (self.tag, w.codec, self.k, self.sim, text))


class Stream:
    """One freshly uploaded index and the batches of its sequence."""

    def __init__(self, T, dev, ref, codec, corpus=None):
        self.w = SWorld(T, dev, corpus or ref.c, codec)
        if corpus is None:
            self.w._want, self.w._scores = ref.want, ref.scores  # (the module's shared references)
        self.jobs, self.cap = [], 0
        self.cache = Cache({r: int(x) for r, x in enumerate(self.w.ix.term_docbytes([self.w.c.tid[n] for n in HEADS]))})

    def job(self, tag, kind, names, cap=FULL, k=0, sim=0, opts=None, masked=None):
        if "scored" in kind and not k:
            k = 10
        return Job(self, tag, kind, list(names), cap, k, sim, opts or {}, masked)

    def bytes_of(self, rows):
        return sum(self.cache.docbytes[r] for r in rows)

    def close(self):
        for j in self.jobs:
            j.b.close()
        self.w.ix.close()


def scrub(T, dev, ref, codec, caps):
    """Leaves DECOY rows in the pool's idle buffers of the sizes the test's cache is about to take: plane 0, the high region and the rank records at each of `caps`."""
    for n in caps:  # (an index per capacity: the decoy's own cache never grows, every row it reads it has built itself)
        st = Stream(T, dev, ref, codec, corpus=ref.decoy)
        batches = []
        try:
            progs = S.programs(S.stream_docs_queries(st.w.c, HEADS[:n]))
            with options(dev, **capacity(n)):
                batches.append(T.Batch(st.w.ix, progs, T.FLAG_DOCUMENTS_ONLY))
                batches.append(T.Batch(st.w.ix, S.programs([(st.w.c.q('"{h0} {h1}"'), 1)]), T.FLAG_DOCUMENTS_ONLY))
            with options(dev, **dict(capacity(n), **ONEPASS)):
                batches.append(T.Batch(st.w.ix, progs, T.FLAG_ACCUMULATED_SCORE, topk=10))
            for b in batches:
                b.run()
            for b in batches:
                b.sync()
        finally:
            for b in batches:
                b.close()
            st.close()
    dev.sync()


@pytest.fixture
def stream(T, dev, ref):
    """make(codec, caps) -> a Stream over a fresh upload, behind a decoy sequence at `caps`; everything is closed when the test ends."""
    made = []

    def make(codec, caps):
        scrub(T, dev, ref, codec, caps)
        made.append(Stream(T, dev, ref, codec))
        return made[-1]

    yield make
    for st in made:
        st.close()


# ------------------------------------------------------------------------------------------ 1: growth keeps what was built
def growth_sequence(st):
    """Capacity 2, then 5, then full, each batch read after its own sync; then the first two batches — created at the small capacities, kept open — run again."""
    A = st.job("A cap 2", "docs", HEADS[:2], cap=2)
    dA = A.run()
    A.check()
    B = st.job("B cap 5", "docs", HEADS[:5], cap=5)
    dB = B.run()
    B.check()
    C = st.job("C full", "docs", HEADS)
    dC = C.run()
    C.check()
    again = [A.run(), B.run()]
    A.check()
    B.check()
    return dA, dB, dC, again


@pytest.mark.parametrize("codec", [1, 2])
def test_growth_keeps_what_was_built(stream, codec):
    """Rows built at capacity 2 are read at capacity 5 and 12 WITHOUT a rebuild (PlaneCache::fit's copy of plane 0, its `built` bits kept), only the new rows are decoded
    at each growth, and the oldest batch, run again after both growths, decodes nothing and answers the same."""
    st = stream(codec, (2, 5, FULL))
    dA, dB, dC, again = growth_sequence(st)
    if not OVERRIDDEN:
        assert dA == st.bytes_of([0, 1]) > 0 and dB == st.bytes_of([2, 3, 4]) > 0 and dC == st.bytes_of(range(5, FULL)) > 0 and again == [0, 0], (dA, dB, dC, again)


# ------------------------------------------------------------------------------------------ 2: an older batch run after a newer batch's growth
@pytest.mark.parametrize("codec", [1, 2])
def test_older_batch_runs_after_a_newer_batch_s_growth(stream, codec):
    """A batch created at capacity 2 and not yet run; a second batch's creation grows the cache; both run back to back, nothing synced in between: the older batch
    builds its rows in the GROWN cache, behind the move's event.  Names head terms above its capacity too: rows it may not address."""
    st = stream(codec, (2, FULL))
    A = st.job("A cap 2, created first", "docs", HEADS[:5], cap=2)
    B = st.job("B full, grows before A runs", "docs", HEADS)
    dA, dB = A.run(), B.run()
    A.check()
    B.check()
    if not OVERRIDDEN:
        assert dA == st.bytes_of([0, 1]) and dB == st.bytes_of(range(2, FULL)), (dA, dB)


@pytest.mark.parametrize("codec", [1, 2])
def test_growth_behind_a_running_batch_then_the_first_high_region(stream, codec):
    """The other order: A runs and is NOT synced; B's creation grows the cache behind A's readers (the old buffers retire on events recorded behind the copies); B runs;
    a scored batch's creation then adds the high region alone (no resize) and its run decodes every row again, whole; only then A, B and C are synced and read, in that
    order.  Correct at any timing; this is the order in which a wrong event order can bite."""
    st = stream(codec, (2, FULL))
    A = st.job("A cap 2, running", "docs", HEADS[:5], cap=2)
    dA = A.run()
    B = st.job("B full, grows behind A", "docs", HEADS)
    dB = B.run()
    C = st.job("C scored, first high region", "scored", HEADS, k=10, opts=ONEPASS)
    dC = C.run()
    A.check()
    B.check()
    C.check()
    if not OVERRIDDEN:
        assert dA == st.bytes_of([0, 1]) and dB == st.bytes_of(range(2, FULL)) and dC == st.bytes_of(range(FULL)), (dA, dB, dC)


# ------------------------------------------------------------------------------------------ 3: the high part through growth, in both orders
@pytest.mark.parametrize("how", ["onepass", "score"])
@pytest.mark.parametrize("codec", [1, 2])
def test_high_parts_are_copied_by_a_growth(stream, codec, how):
    """Scored first, at capacity 3: plane 0 and the high region are allocated together.  A DocumentsOnly batch at full capacity then resizes while a high region exists.
    The first scored batches — all three similarities, K = 10 and 256 — run again: nothing is decoded and the top-K is still right, so the high rows were copied intact.
    Scored batches over all rows then decode the NEW rows whole (their plane 0 is there, their high part is not)."""
    opts = ONEPASS if how == "onepass" else SCORE
    st = stream(codec, (3, FULL))
    first = [st.job(f"S{i} cap 3", "scored", HEADS[:3], cap=3, k=k, sim=sim, opts=opts) for i, (k, sim) in enumerate([(10, SIMS[0]), (256, SIMS[0]), (10, SIMS[1]), (256, SIMS[2])])]
    d1 = [j.run() for j in first]
    for j in first:
        j.check()
    D = st.job("D full, docs only", "docs", HEADS)
    dD = D.run()
    D.check()
    d2 = [j.run() for j in first]
    for j in first:
        j.check()
    later = [st.job(f"T{i} full", "scored", HEADS, k=k, sim=sim, opts=opts) for i, (k, sim) in enumerate([(10, SIMS[0]), (256, SIMS[1]), (10, SIMS[2])])]
    d3 = [j.run() for j in later]
    for j in later:
        j.check()
    dD2 = D.run()
    D.check()
    if not OVERRIDDEN:
        assert d1 == [st.bytes_of([0, 1, 2]), 0, 0, 0] and dD == st.bytes_of(range(3, FULL)) and d2 == [0, 0, 0, 0], (d1, dD, d2)
        assert d3 == [st.bytes_of(range(3, FULL)), 0, 0] and dD2 == 0, (d3, dD2)


@pytest.mark.parametrize("how", ["onepass", "score"])
@pytest.mark.parametrize("codec", [1, 2])
def test_high_parts_are_added_to_rows_that_have_plane_0(stream, codec, how):
    """DocumentsOnly first, at full capacity; then scored over the same terms (BM25): the high region is new, every row is decoded again for its high part and its plane 0
    is rewritten; DocumentsOnly afterwards decodes nothing and is unchanged."""
    opts = ONEPASS if how == "onepass" else SCORE
    st = stream(codec, (FULL,))
    D = st.job("D full, docs only", "docs", HEADS)
    dD = D.run()
    D.check()
    scored = [st.job(f"S K={k}", "scored", HEADS, k=k, opts=opts) for k in (10, 256)]
    dS = [j.run() for j in scored]
    for j in scored:
        j.check()
    dD2 = D.run()
    D.check()
    E = st.job("E full, docs only, created last", "docs", HEADS[:5])
    dE = E.run()
    E.check()
    if not OVERRIDDEN:
        assert dD == st.bytes_of(range(FULL)) and dS == [st.bytes_of(range(FULL)), 0] and dD2 == 0 and dE == 0, (dD, dS, dD2, dE)


# ------------------------------------------------------------------------------------------ 4: phrase rank records through growth
@pytest.mark.parametrize("codec", [1, 2])
def test_phrase_rank_records_through_growth(stream, codec):
    """GOOGLE: k_phrase finds a head term's hits by rank in plane 0 once run_phrases has built the row's rank directory and hits entries.  A phrase batch at capacity 2
    builds them for rows 0 and 1; a DocumentsOnly batch at capacity 4 builds plane 0 of rows 2 and 3 without rank records (the records of rows 0 and 1 move); a scored
    batch at capacity 6 builds rows 4 and 5 whole, without rank records (they move again); phrase batches at full capacity — DocumentsOnly and scored, K = 10 — then name
    terms of all three groups: rows 0 and 1 have everything, rows 2 .. 5 have plane 0 rebuilt with their rank records; the first phrase batch runs again last.  LUCENE
    has no rank path: the same sequence, for its results (and what its plane rows decode)."""
    st = stream(codec, (2, 4, 6, FULL))
    P1 = st.job("P1 cap 2, phrases", "phrase", HEADS[:2], cap=2)
    P1.run()
    P1.check()
    D2 = st.job("D2 cap 4, docs only", "docs", HEADS[:4], cap=4)
    d2 = D2.run()
    D2.check()
    S3 = st.job("S3 cap 6, scored", "scored", HEADS[4:6], cap=6, k=10, opts=ONEPASS)
    d3 = S3.run()
    S3.check()
    P4 = st.job("P4 full, phrases", "phrase", HEADS[:6])
    P5 = st.job("P5 full, phrases scored", "phrase_scored", HEADS[:6], k=10)
    P4.run()
    P5.run()
    P4.check()
    P5.check()
    P6 = st.job("P6 full, phrases scored, one pass", "phrase_scored", HEADS[:6], k=10, opts=ONEPASS)
    P6.run()
    P6.check()
    P1.run()
    P1.check()
    d2b = D2.run()
    D2.check()
    assert sum(len(x) > 0 for x in P4.want) >= 12 and len(P4.want[0]) > S.PL_RANK_DOCS
    if not OVERRIDDEN:
        assert P4.b.info()["phrase_queries"] >= len(P4.queries)  # (a phrase under an OR is a hidden query of its own)
        assert d3 == st.bytes_of([4, 5]) and d2b == 0, (d3, d2b)
        if codec == 1:  # (rows 0 and 1 got their plane 0 with their rank records, whichever of them P1's planner chose)
            assert d2 == st.bytes_of([2, 3]), d2


# ------------------------------------------------------------------------------------------ 5: the mask changes mid-stream
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("codec", [1, 2])
def test_mask_changes_between_runs(stream, dev, ref, codec, overlap):
    """A runs unmasked and is not synced; the masked set is installed (window-boundary documents, a run of 300, the first document and the last); B is created and runs;
    the set is cleared; C is created and runs; then all are synced and read: A and C unmasked, B masked.  DocumentsOnly and scored batches side by side, at the default
    options — and with k_and on the second stream (option overlap): tri_index_set_masked synchronises the engine stream, which that stream's kernels rejoin."""
    st = stream(codec, (FULL,))
    M = ref.masked
    with options(dev, overlap=overlap):
        A = [st.job("A docs, unmasked", "docs", HEADS, cap=0), st.job("A scored, unmasked", "scored", HEADS, cap=0, k=10)]
        for j in A:
            j.run()
        st.w.ix.set_masked(M)
        B = [st.job("B docs, masked", "docs", HEADS, cap=0, masked=M), st.job("B scored, masked", "scored", HEADS, cap=0, k=10, masked=M)]
        for j in B:
            j.run()
        st.w.ix.set_masked(np.zeros(0, np.uint32))
        C = [st.job("C docs, unmasked again", "docs", HEADS, cap=0), st.job("C scored, unmasked again", "scored", HEADS, cap=0, k=256)]
        for j in C:
            j.run()
        for j in A + B + C:
            j.check()
        if not OVERRIDDEN:
            assert A[0].b.info()["cand_queries"] > 0 and A[0].b.info()["pset_queries"] > 0, A[0].b.info()
    assert any(len(w) != int((~np.isin(w, M)).sum()) for w in A[0].want)


# ------------------------------------------------------------------------------------------ 6: the cold-cache switch
@pytest.mark.parametrize("codec", [1, 2])
def test_planes_rebuild_decodes_every_run(stream, dev, codec):
    """planes_rebuild = 1 (bench.py's cold rotating leg): three rounds of the same two batches, each run enqueued behind the other batch's with no sync between — every
    run rebuilds the rows it names, reports the same bytes and answers the reference; back at 0 the next runs decode nothing."""
    st = stream(codec, (FULL,))
    X = st.job("X docs", "docs", HEADS[:5])
    Y = st.job("Y scored", "scored", HEADS, k=10, opts=ONEPASS)
    seen = []
    with options(dev, planes_rebuild=1):
        for _ in range(3):
            seen.append((X.run(rebuild=True), Y.run(rebuild=True)))
            X.check()
            Y.check()
    after = (X.run(), Y.run())
    X.check()
    Y.check()
    if not OVERRIDDEN:
        assert seen == [(st.bytes_of(range(5)), st.bytes_of(range(FULL)))] * 3 and after == (0, 0), (seen, after)


# ------------------------------------------------------------------------------------------ 7: nothing leaks
def test_growths_hand_their_buffers_back(T, dev, ref):
    """The pool's bytes in use before the upload == after the growth sequence of test 1, once every batch and the index are closed: the row buffers both growths
    retired and the cache itself went back to the pool."""
    dev.sync()
    before = dev.memory()["pool_in_use_bytes"]
    st = Stream(T, dev, ref, 1)
    try:
        growth_sequence(st)
        assert dev.memory()["pool_in_use_bytes"] > before
    finally:
        st.close()
    dev.sync()
    assert dev.memory()["pool_in_use_bytes"] == before, (dev.memory(), before)
