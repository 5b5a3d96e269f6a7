"""GPU tests of the lifecycle the three consumers of a batch's docID sets share (run with -m gpu on an MI355X): facets (tri_batch_set_facets), an order
(tri_batch_set_order) and stats (tri_batch_set_stats) on ONE batch — csrc/consumers.hpp keeps a slot for each and sets, runs, syncs and clears them the same way.  What
no single-consumer test sees: all three set at once and cleared in every order, a refused setter beside two others, the three replaced behind one queued run, and the
three *_last_us options side by side.

The reference is numpy over structured.Corpus.evaluate's docID sets (facet_cases.facet_rows, order_cases.rows, stats_cases.stats_rows), computed once per spec and
codec — never the engine's own docsets.  Every comparison is integer equality.  The corpus is the stream corpus (the smallest the consumers' own lifecycle tests use),
in both codecs; one device handle for the file and one of its own per *_last_us case; every index, column and batch is closed by the test or fixture that made it; nothing sleeps or loops over a timing."""
import itertools

import numpy as np
import pytest

import facet_cases as F
import order_cases as OC
import stats_cases as X
import structured as S

pytestmark = pytest.mark.gpu

ROUNDS = 1  # rounds of k_order_merge: no query of stream_docs_queries has more than ORDER_FANIN tasks (tests/test_gpu_order.py::test_lifecycle_and_launches)
SHARE = {"facets": 1, "order": 1 + ROUNDS, "stats": 1}  # kernels per run
FACETS = [("mod7", 7), ("low16", F.LDS_COUNTERS)]  # 8 counters: under FACET_LDS_COUNTERS; LDS_COUNTERS + 1: over it
STATS = [(None, 0, "hash"), ("mod7", 5, "rev")]  # one ungrouped, one grouped
NOT_SET = {"facets": "no facets are set", "order": "no order is set", "stats": "no stats are set"}
LAST_US = {"facets": "facet_last_us", "order": "order_last_us", "stats": "stats_last_us"}


def order_spec(topk):
    return ("hash", topk, False)


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


@pytest.fixture(scope="module")
def dev(T):
    from conftest import apply_test_options

    d = apply_test_options(T.Device(0))
    yield d
    d.close()


class World:
    """The stream corpus uploaded in one codec, its named columns (made on first use) and the expected rows of every spec asked for (computed once)."""

    def __init__(self, T, dev, corpus, codec):
        self.T, self.c = T, corpus
        self.ix = corpus.upload(T, dev, codec)
        self.values, self.made, self.wanted = X.columns(corpus.D), {}, {}
        self.progs = S.programs(S.stream_docs_queries(corpus))
        self.sets = [corpus.evaluate(p) for p in self.progs]

    def col(self, name):
        if name is None:
            return None
        if name not in self.made:
            self.made[name] = self.T.Column(self.ix, self.values[name])
        return self.made[name]

    def set(self, b, what, spec):
        if what == "facets":
            b.set_facets([(self.col(n), nb) for n, nb in spec])
        elif what == "order":
            b.set_order(self.col(spec[0]), spec[1], spec[2])
        else:
            b.set_stats([(self.col(g), nb, self.col(v)) for g, nb, v in spec])

    def set_all(self, b, specs, order=("facets", "order", "stats")):
        for what in order:
            self.set(b, what, specs[what])

    def read(self, b, what, spec):
        """The consumer's rows as a flat list of arrays."""
        if what == "facets":
            return [b.facets(k) for k in range(len(spec))]
        if what == "order":
            return list(b.ordered())
        return [plane for k in range(len(spec)) for plane in b.stats(k)]

    def want(self, what, spec):
        key = (what, repr(spec))
        if key not in self.wanted:
            if what == "facets":
                rows = [F.facet_rows(self.sets, self.values[n], nb) for n, nb in spec]
            elif what == "order":
                rows = list(OC.rows(self.sets, self.values[spec[0]], spec[1], spec[2]))
            else:
                rows = [plane for g, nb, v in spec for plane in X.stats_rows(self.sets, None if g is None else self.values[g], nb, self.values[v])]
            self.wanted[key] = rows
        return self.wanted[key]

    def check(self, b, specs, tag, only=None):
        for what in only if only is not None else specs:
            got, want = self.read(b, what, specs[what]), self.want(what, specs[what])
            assert len(got) == len(want), (tag, what)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (tag, what, i)

    def close(self):
        for c in self.made.values():  # (a column is destroyed before its index)
            c.close()
        self.ix.close()


@pytest.fixture(scope="module")
def worlds(T, dev):
    corpus, made = S.CORPORA["stream"](), {}

    def get(codec):
        if codec not in made:
            made[codec] = World(T, dev, corpus, codec)
        return made[codec]

    yield get
    for w in made.values():
        w.close()


def clear(b, what):
    if what == "facets":
        b.set_facets([])
    elif what == "order":
        b.clear_order()
    else:
        b.set_stats([])


def run_sync(b):
    b.run()
    b.sync()


# ------------------------------------------------------------------------------------------ 1. all three at once, cleared in every order
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("topk", [1, 256])
def test_all_three_at_once_cleared_in_every_order(T, dev, worlds, codec, topk):
    """Facets, an order and stats on one batch: info().launches is the plain batch's plus every consumer's share, the rows equal numpy's.  Then, for each of the six
    clearing orders: after each clear the launches drop by that consumer's share, a fresh run leaves the remaining consumers' rows as they were, the cleared one's read
    call refuses; at the end the launches are the plain batch's."""
    w = worlds(codec)
    specs = {"facets": FACETS, "order": order_spec(topk), "stats": STATS}
    b = T.Batch(w.ix, w.progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        plain = b.info()["launches"]
        for perm in itertools.permutations(SHARE):
            w.set_all(b, specs)
            assert b.info()["launches"] == plain + 1 + (1 + ROUNDS) + 1, perm
            run_sync(b)
            w.check(b, specs, ("all three", perm))
            left = list(SHARE)
            for what in perm:
                clear(b, what)
                left.remove(what)
                assert b.info()["launches"] == plain + sum(SHARE[x] for x in left), (perm, what)
                run_sync(b)
                w.check(b, specs, (perm, "after clearing", what), only=left)
                for gone in set(SHARE) - set(left):
                    with pytest.raises(T.TrinityError, match=NOT_SET[gone]):
                        w.read(b, gone, specs[gone])
            assert b.info()["launches"] == plain, perm
        assert b.counts().tolist() == [len(s) for s in w.sets]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ 2. a refused setter changes nothing
@pytest.mark.parametrize("codec", [1, 2])
def test_a_refused_setter_changes_nothing(T, dev, worlds, codec):
    """With all three set and a run synced, each setter is called with a spec whose LAST element is invalid — nbuckets 0, topk 257, a column of another index —: the call
    fails, the launches stand, the read call still returns the synced run's rows, and so does a fresh run."""
    w, other = worlds(codec), worlds(3 - codec)  # (the same corpus in the other codec: another index)
    specs = {"facets": FACETS, "order": order_spec(10), "stats": STATS}
    bad = [
        ("facets", lambda: b.set_facets([(w.col("mod7"), 7), (w.col("low16"), 0)]), "nbuckets 0"),
        ("order", lambda: b.set_order(w.col("rev"), OC.MAX_TOPK + 1, True), "topk 257"),
        ("stats", lambda: b.set_stats([(None, 0, w.col("rev")), (w.col("mod7"), 5, other.col("hash"))]), "value column belongs to another index"),
        ("facets", lambda: b.set_facets([(w.col("mod7"), 7), (other.col("low16"), 5)]), "column belongs to another index"),
        ("stats", lambda: b.set_stats([(None, 0, w.col("rev")), (w.col("mod7"), 0, w.col("hash"))]), "nbuckets 0"),
        ("order", lambda: b.set_order(other.col("rev"), 5, True), "the column belongs to another index"),
    ]
    b = T.Batch(w.ix, w.progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        w.set_all(b, specs)
        launches = b.info()["launches"]
        run_sync(b)
        w.check(b, specs, "before")
        for what, call, words in bad:
            with pytest.raises(T.TrinityError, match=words):
                call()
            assert b.info()["launches"] == launches, (what, words)
            w.check(b, specs, ("the synced run's rows", what, words))
        run_sync(b)
        w.check(b, specs, "a fresh run")
        assert b.info()["launches"] == launches
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ 3. replaced behind a queued run
@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("order", [("facets", "order", "stats"), ("stats", "facets", "order")])
def test_replaced_behind_a_queued_run(T, dev, worlds, codec, order):
    """run() without sync(), then each of the three replaced (other nbuckets / topk / value column): after sync() the three read calls refuse — the run predates the
    specs —, and the next run's rows equal numpy's for the new specs."""
    w = worlds(codec)
    first = {"facets": FACETS, "order": order_spec(10), "stats": STATS}
    second = {"facets": [("mod7", 5), ("window", 2)], "order": ("rev", 256, True), "stats": [(None, 0, "rev"), ("mod7", 7, "hash")]}
    b = T.Batch(w.ix, w.progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        w.set_all(b, first)
        launches = b.info()["launches"]
        b.run()  # a run queued ...
        w.set_all(b, second, order)  # ... and the replacements behind it: every setter waits for the run, which consumed into the blocks it was launched with
        assert b.info()["launches"] == launches
        b.sync()
        for what in SHARE:
            with pytest.raises(T.TrinityError, match="tri_batch_sync first"):
                w.read(b, what, second[what])
        run_sync(b)
        w.check(b, second, ("behind the replacements", order))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------ 4. *_last_us
@pytest.mark.parametrize("gone", list(SHARE))
def test_last_us_of_every_consumer(T, worlds, gone):
    """On a device handle of its own (the options are the handle's, 0 until a run writes them): with one consumer cleared, a synced run writes the other two options and
    leaves the cleared one's at 0; with all three set, a synced run writes all three.  No magnitude is asserted."""
    from conftest import apply_test_options

    own = apply_test_options(T.Device(0))
    w = World(T, own, worlds(1).c, 1)
    specs = {"facets": FACETS, "order": order_spec(256), "stats": STATS}
    b = T.Batch(w.ix, w.progs, T.FLAG_DOCUMENTS_ONLY)
    try:
        assert [own.get_option(LAST_US[x]) for x in SHARE] == [0, 0, 0]
        w.set_all(b, specs)
        clear(b, gone)
        run_sync(b)
        assert all((own.get_option(LAST_US[x]) > 0) == (x != gone) for x in SHARE), [own.get_option(LAST_US[x]) for x in SHARE]
        w.set(b, gone, specs[gone])
        run_sync(b)
        assert all(own.get_option(LAST_US[x]) > 0 for x in SHARE), [own.get_option(LAST_US[x]) for x in SHARE]
        w.check(b, specs, ("all three", gone))
    finally:
        b.close()
        w.close()
        own.close()
