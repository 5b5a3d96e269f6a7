"""GPU tests of who owns the device memory (run with -m gpu on an MI355X): csrc/owners.hpp — every buffer, pinned block, event and handle reference of an index,
a batch, a filter and a collection batch is released by the member that holds it, behind the waits of the object's destructor and ahead of its reference on the
device handle.

(a) Pool balance per object kind: one table of the kinds of object a caller creates; each is created on a freshly uploaded index, run, synced, ONE result read and
    checked against the CPU oracle as the neighbouring files do (docID sets and counts exact, top-K docIDs exact and scores within 1e-5 relative, ranked lists bit for
    bit through rank_cases / crank_cases), and closed with its index: the handle's pool_in_use_bytes is then what it was before the upload.
(b) Closing the handle first: tri_dev_close with objects alive only marks the handle; a synced batch, a batch that ran and was never synced, a filter, a collection
    (after its parts) and the index are destroyed after it, the last of them takes the handle along; a fresh handle then answers as the oracle does.

The corpus is the suite's smallest synthetic world, crank_cases.WORLDS[0] = (2000 documents, 200 terms), with the 600-document source that updates it for the
collection; both codecs.  Nothing here makes an allocation fail: the error paths of the owners are not reachable from a test."""
import numpy as np
import pytest

import crank_cases as CR
import oracle_lib as O
import rank_cases as R
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)
from test_gpu_rank import check_row

pytestmark = pytest.mark.gpu
K, CAP, ADJ, w3 = 10, CR.CAP, CR.ADJ, CR.w3
CONJ, UNION, CNF, PHRASE, TREE = "t0 t1", "t0 OR t1 OR t2", "t0 t1 (t2 OR t3 OR t4)", '"t0 t1" t2', 't5 OR "t0 t1"'


@pytest.fixture(scope="module")
def segs(T):
    """(source, codec) -> the segment: built once, uploaded by every case anew"""
    made = {}

    def get(si, codec):
        if (si, codec) not in made:
            made[si, codec] = T.Segment(*CR.WORLDS[si], codec=codec)
        return made[si, codec]

    return get


class Env:
    """What a kind runs in: the handle, and the indexes it uploads — closed, with everything the kind registered, by close()"""

    def __init__(self, T, dev, segs, codec):
        self.T, self.dev, self.segs, self.codec, self.ixs, self.held = T, dev, segs, codec, {}, []
        self.ora = CR.oracle_of(0)  # (both codecs hold the same corpus and answer alike: tests/test_abi.py)

    def ix(self, si=0):
        if si not in self.ixs:
            self.ixs[si] = self.T.Index.from_segment(self.dev, self.segs(si, self.codec))
        return self.ixs[si]

    def keep(self, obj):
        self.held.append(obj)
        return obj

    def batch(self, texts, flags, topk=0, si=0):
        progs = [O.parse_query(t) for t in texts]
        return progs, self.keep(self.T.Batch(self.ix(si), progs, flags, topk=topk))

    def close(self):
        for obj in reversed(self.held):  # (a collection before its parts, a batch before the filters it names)
            obj.close()
        for ix in self.ixs.values():
            ix.close()
        self.held, self.ixs = [], {}


def ran(b):
    b.run()
    b.sync()
    return b


def check_topk(env, b, progs):
    d, s, c = b.topk_results()
    counts = b.counts()
    for i, prog in enumerate(progs):
        docs, scores = env.ora.exec(prog, O.FLAG_ACCUM_SCORE)
        td, ts = env.ora.topk(docs, scores, K)
        assert int(counts[i]) == len(docs) and int(c[i]) == len(td), i
        assert d[i, : len(td)].tolist() == td.tolist(), i
        np.testing.assert_allclose(s[i, : len(td)], ts, rtol=1e-5, atol=0)


def kind_docs_only(env):
    progs, b = env.batch([CONJ, UNION, CNF], env.T.FLAG_DOCUMENTS_ONLY)
    ran(b)
    for i, prog in enumerate(progs):
        assert np.array_equal(b.docset(i), env.ora.exec(prog, O.FLAG_DOCUMENTS_ONLY)[0]), i
    assert b.docset_hashes().size == len(progs)  # (the batch's hipMalloc'ed hash column)


def kind_scored_topk(env):
    progs, b = env.batch([CONJ, UNION, CNF], env.T.FLAG_ACCUMULATED_SCORE, topk=K)
    check_topk(env, ran(b), progs)


def kind_scored_every_match(env):
    progs, b = env.batch([CONJ, UNION, CNF], env.T.FLAG_ACCUMULATED_SCORE, topk=0)
    ran(b)
    for i, prog in enumerate(progs):
        docs, scores = env.ora.exec(prog, O.FLAG_ACCUM_SCORE)
        assert np.array_equal(b.docset(i), docs), i
        np.testing.assert_allclose(b.scores(i), scores, rtol=1e-5, atol=0)


def kind_scored_phrase(env):
    progs, b = env.batch([PHRASE, CONJ], env.T.FLAG_ACCUMULATED_SCORE, topk=K)
    check_topk(env, ran(b), progs)


def kind_tree(env):
    progs, b = env.batch([TREE, CONJ], env.T.FLAG_DOCUMENTS_ONLY)
    ran(b)
    assert np.array_equal(b.docset(0), env.ora.exec(progs[0], O.FLAG_DOCUMENTS_ONLY)[0])
    progs, b = env.batch([TREE, CONJ], env.T.FLAG_ACCUMULATED_SCORE, topk=K)  # (the trees' score stream)
    check_topk(env, ran(b), progs)


def kind_default_ranked(env):
    """hit payloads; a ranker set, cleared, set again at another K — every block but the last goes back while the batch lives"""
    texts = CR.PAIR_QUERIES[:3]
    progs, b = env.batch(texts, env.T.FLAG_MATCHED_TERMS | env.T.FLAG_HIT_PAYLOADS)
    weights = R.token_weights(progs, w3)
    b.set_ranker(3, CAP, ADJ, weights)
    ran(b)
    b.clear_ranker()
    b.set_ranker(K, CAP, ADJ, weights)
    ran(b)
    d, s, c = b.ranked()
    for i, prog in enumerate(progs):
        check_row(d, s, c, i, CR.source_rows(prog, CAP, ADJ, w3, masked=False, n=1)[0], K, texts[i])
    lens, payloads = b.matched_payloads(0)
    assert lens.size == payloads.size


def kind_two_filters(env):
    """one filter made of a docID list (drop), one of a synced batch's docID set (keep)"""
    T = env.T
    src_progs, src = env.batch(["t1 OR t2"], T.FLAG_DOCUMENTS_ONLY)
    ran(src)
    drop = np.arange(1, 1000, 2, dtype=np.uint32)
    filters = [env.keep(T.Filter(env.ix(), drop)), env.keep(T.Filter.from_docset(src, 0, keep=True))]
    progs, b = env.batch([UNION, CONJ, "t0"], T.FLAG_DOCUMENTS_ONLY)
    b.set_filters(filters, [0, T.NO_FILTER, 1])
    ran(b)
    want = [env.ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0] for p in progs]
    allowed = env.ora.exec(src_progs[0], O.FLAG_DOCUMENTS_ONLY)[0]
    assert np.array_equal(b.docset(0), np.setdiff1d(want[0], drop))
    assert np.array_equal(b.docset(1), want[1])
    assert np.array_equal(b.docset(2), np.intersect1d(want[2], allowed))


def kind_ranked_collection(env):
    texts = CR.PAIR_QUERIES[:3]
    progs = [O.parse_query(t) for t in texts]
    parts = []
    for si, mask in enumerate(CR.masks(2)):
        env.ix(si).set_masked(mask)
        parts.append(env.keep(env.T.Batch(env.ix(si), progs, env.T.FLAG_MATCHED_TERMS)))
        parts[-1].set_ranker(K, CAP, ADJ, R.token_weights(progs, w3))
    cb = env.keep(env.T.CollectionBatch(parts))
    ran(cb)
    d, s, c = cb.ranked()
    for i, prog in enumerate(progs):
        check_row(d, s, c, i, CR.want(prog, K, CAP, ADJ, w3, n=2), K, texts[i])


KINDS = [kind_docs_only, kind_scored_topk, kind_scored_every_match, kind_scored_phrase, kind_tree, kind_default_ranked, kind_two_filters, kind_ranked_collection]


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("kind", KINDS, ids=[k.__name__[5:] for k in KINDS])
def test_every_kind_of_object_hands_its_buffers_back(T, dev, segs, kind, codec):
    before = dev.memory()["pool_in_use_bytes"]
    env = Env(T, dev, segs, codec)
    try:
        kind(env)
        assert dev.memory()["pool_in_use_bytes"] > before  # (the objects do hold pooled buffers while they live)
    finally:
        env.close()
    assert dev.memory()["pool_in_use_bytes"] == before, (kind.__name__, dev.memory(), before)


@pytest.mark.parametrize("codec", [1, 2])
def test_the_handle_may_be_closed_first(T, segs, codec):
    """tri_dev_close with objects alive: they keep the handle's streams and pools, and the last of them to go takes the handle along."""
    own = T.Device(0)
    env = Env(T, own, segs, codec)
    progs, synced = env.batch([CONJ, UNION], T.FLAG_DOCUMENTS_ONLY)
    ran(synced)
    want = env.ora.exec(progs[0], O.FLAG_DOCUMENTS_ONLY)[0]
    assert int(synced.counts()[0]) == len(want)
    _, unsynced = env.batch([CONJ, CNF], T.FLAG_ACCUMULATED_SCORE, topk=K)
    unsynced.run()  # (never synced: its destructor waits for the run)
    flt = T.Filter.from_docset(synced, 0, keep=True)
    parts = [env.batch([CONJ], T.FLAG_ACCUMULATED_SCORE, topk=K)[1] for _ in range(2)]
    cb = ran(T.CollectionBatch(parts))
    assert int(cb.counts()[0]) == 2 * len(want)  # (the same source twice, unmasked: every match counted in both parts)
    own.close()
    for obj in [synced, unsynced, flt] + parts + [cb, env.ix()]:
        obj.close()
    fresh = T.Device(0)
    try:
        ix = T.Index.from_segment(fresh, segs(0, codec))
        b = ran(T.Batch(ix, progs, T.FLAG_DOCUMENTS_ONLY))
        assert int(b.counts()[0]) == len(want)
        b.close()
        ix.close()
    finally:
        fresh.close()
