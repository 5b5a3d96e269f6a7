"""GPU tests of the walk k_score and k_rich share (a term's blocks against a tile of matches held in LDS: block-driven or match-driven), on structured.walk_corpus with the
term planes off, so that the scorers walk the postings: `few AND all` — 5 matches, 258 blocks of `all` in their range: the MATCH-DRIVEN branch, two matches
in one block (only the first of a block run decodes it), one on the last document of the last full block, the last one in the list's last, short block — and `all AND third` — 2 743 matches, two tiles of the
default mode's 2048, no more blocks in range than matches: the BLOCK-DRIVEN branch.  Both codecs; scored (top-K and the full score stream) and the default mode
(matched terms, frequencies and positions: its COUNT and WRITE passes).  Docsets against structured.Corpus.evaluate, scores and records against the oracle.
Every batch must have run as one candidate query (k_and, then k_score or k_rich): asserted on info(), unless TRINITY_TEST_OPTIONS chose the paths."""
import numpy as np
import pytest

import oracle_lib as O
import structured as S
from test_gpu_parity import options, rich_flat
from test_gpu_structured import OVERRIDDEN, SWorld, T, check_scored, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
OPTS = {"planes": 0}


@pytest.fixture(scope="module")
def walk_worlds(T, dev):  # noqa: F811
    c = S.walk_corpus()
    made = {codec: SWorld(T, dev, c, codec) for codec in (1, 2)}
    yield made
    for w in made.values():
        w.ix.close()


def case(w, which):
    queries = S.walk_queries(w.c)[which : which + 1]
    progs, want, _ = w.want(("walk", which), queries)
    assert len(want[0]) == (len(S.WALK_FEW), S.D_WALK // 3)[which] and (which == 0 or len(want[0]) > 2048)
    everyone = w.c.lists["all"][0]
    block = (np.searchsorted(everyone, S.WALK_FEW) // 32).tolist()  # by RANK in `all`: its blocks hold 32 postings each, the last one the rest
    assert -(-everyone.size // 32) == 258 and everyone.size % 32 and block[0] == block[1] and block[-2:] == [256, 257], block
    return queries, progs, want


def ran_as_candidates(b):
    """The batch's one query went through k_and's candidate tiles and the walk — no other kernel family took it."""
    info = b.info()
    others = ("dense_queries", "fused_queries", "planes_queries", "phrase_queries", "pset_queries", "probe_queries", "tree_queries", "unsupported_queries")
    assert OVERRIDDEN or (info["cand_queries"] == 1 and not any(info[k] for k in others)), info


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("which", [0, 1], ids=["match_driven", "block_driven"])
def test_scored_walk(walk_worlds, which, codec):
    w = walk_worlds[codec]
    queries, progs, want = case(w, which)
    check_scored(w, ("walk", which), queries, progs, [len(want[0])], 10, OPTS)
    docs, scores = w.scores((("walk", which), 0, False), progs)[0]
    with options(w.dev, **OPTS):
        b = w.T.Batch(w.ix, progs, w.T.FLAG_ACCUMULATED_SCORE, topk=0)
    try:
        b.run()
        b.sync()
        ran_as_candidates(b)
        assert int(b.counts()[0]) == len(docs)
        assert np.array_equal(b.docset(0, len(docs)), want[0]) and np.array_equal(docs, want[0])
        np.testing.assert_allclose(b.scores(0, len(docs)), scores, rtol=1e-5, atol=0)
    finally:
        b.close()


@pytest.mark.parametrize("codec", [1, 2])
@pytest.mark.parametrize("which", [0, 1], ids=["match_driven", "block_driven"])
def test_default_mode_walk(walk_worlds, which, codec):
    w = walk_worlds[codec]
    queries, progs, want = case(w, which)
    with options(w.dev, **OPTS):
        b = w.T.Batch(w.ix, progs, w.T.FLAG_MATCHED_TERMS)
    try:
        b.run()
        b.sync()
        ran_as_candidates(b)
        docs = b.docset(0, int(b.counts()[0]))
        terms, present, freq, pos = b.matched_terms(0, len(docs))
    finally:
        b.close()
    wdocs, wflat, tt, ht = w.ora.exec_rich(progs[0])
    assert np.array_equal(docs, want[0]) and np.array_equal(docs, wdocs)
    assert int(freq.sum()) == ht and int(sum(bin(int(x)).count("1") for x in present)) == tt == 2 * len(docs)
    assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat)
    assert set(freq.ravel().tolist()) == {1, 2, 3}
