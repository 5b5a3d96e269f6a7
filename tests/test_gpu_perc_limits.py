"""The percolator on the device (tri_perc_match, trinity_amd/csrc/k_perc.hpp, perc_side.hpp) on the cases of tests/perc_limit_cases.py, which
tests/test_perc_limit_cases.py checks on the CPU: documents of more than 64 postings, calls that are windows into larger arrays, phrases of 16 words and at the top of
u16, hit lists around a segment of the document-major fill at more than one tile, batches of 65 535 and 65 536 documents whose segment table takes the scan's top level
into a second round, a call of exactly 2^32 pairs, and the refusal of perc_max_bytes at each of the three scratch blocks.  Every comparison is exact against
perc_cases.match_batch: pairs in both orders, per-document counts, the result's counts."""
import numpy as np
import pytest

import perc_cases as PC
import perc_limit_cases as L
from perc_limit_cases import check

pytestmark = pytest.mark.gpu
UNSUPPORTED = -3


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


def dicts(docs):
    return [L.dict_of(d) for d in docs]


def test_long_documents(T, dev):
    """family_long: the 65th posting's leaf flag and row bit, its positions (the carry between a wave's passes), the length of a long document — with perc_prune 1 and 0"""
    progs, docs, nterms, names = L.family_long()
    arrays = L.arrays_of(docs)
    bits = PC.match_batch(progs, dicts(docs))
    p = T.Percolator(dev, progs, nterms)
    try:
        assert p.status().tolist() == [0] * len(progs)
        for prune in (1, 0):
            dev.set_option("perc_prune", prune)
            try:
                info = check(T, p, progs, arrays, bits=bits)
            finally:
                dev.set_option("perc_prune", 1)
            assert info["phrase_rows"] == L.phrase_rows_of(progs, docs) == 23 and (prune or info["evaluated"] == len(progs))
    finally:
        p.close()


def test_call_windows(T, dev):
    """family_window: doc_first[k:] over whole terms / freqs / positions; a full call between two windows sees no stale state"""
    progs, docs, nterms, ks = L.family_window()
    arrays = L.arrays_of(docs)
    whole = dicts(docs)
    p = T.Percolator(dev, progs, nterms)
    try:
        for k in ks[:2] + (0,) + ks[2:] + (ks[0],):
            info = check(T, p, progs, L.window(arrays, k), whole[k:])
            assert info["ndocs"] == len(docs) - k and info["pairs"] > 0
    finally:
        p.close()


def test_phrase_limits(T, dev):
    """family_phrase_limits: lanes j < 16 and readlane up to 15, positions up to 65535 and a sum past it, equal repeated positions, first words of 64 / 128 / 129 positions"""
    progs, docs, nterms = L.family_phrase_limits()
    p = T.Percolator(dev, progs, nterms)
    try:
        assert p.status().tolist() == [0] * 4 and p.info["phrases"] == 4
        info = check(T, p, progs, PC.arrays_of(docs), docs)
        assert info["phrase_rows"] == L.phrase_rows_of(progs, docs) == 4
        info = check(T, p, progs, PC.arrays_of(docs[6:]), docs[6:])  # words 1 and 2 alone: the 16 distinct words have no row, the alternation has
        assert info["phrase_rows"] == L.phrase_rows_of(progs, docs[6:]) == 3
    finally:
        p.close()


@pytest.mark.parametrize("ndocs,nhit", L.GRID)
def test_compaction_grid(T, dev, ndocs, nhit):
    """grid: nhit around PERC_SEG and two segments with W = 65 (two tiles); at W = 2048 nine segments, 32 tiles a candidate, word 2047, and a segment table of more than
    256 scan blocks.  check() asserts the strictly ascending document-major keys and that no pair names a document >= ndocs."""
    progs, docs, nterms, arrays, bits = L.grid(ndocs, nhit)
    p = T.Percolator(dev, progs, nterms)
    try:
        info = check(T, p, progs, arrays, bits=bits)
        assert info["hit_queries"] == nhit and info["phrase_rows"] == 2
    finally:
        p.close()


def test_pairs_at_two_to_the_32(T, dev):
    """65 536 copies of NOT(1) TERM(0) against 65 536 empty documents are 2^32 pairs: refused from the 64-bit total of 32 scan blocks; against 65 535, 4 294 901 760 pairs
    pass that check and are refused by perc_max_bytes at the third block; the pool is handed back; 3 documents answer exactly"""
    need = 65536 * 2048 * 4 + (64 << 20)  # the candidates' match words, and room for blocks 1 and 2 beside them
    if dev.get_option("perc_max_bytes") < need:
        pytest.skip("perc_max_bytes = %d is set below the %d bytes the candidates of this call take" % (dev.get_option("perc_max_bytes"), need))
    nq = 65536
    progs = [PC.tk(0) + [T.tok(T.OP_NOT, 1)]] * nq
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    before = dev.memory()["pool_in_use_bytes"]
    p = T.Percolator(dev, progs, 1)
    try:
        held = dev.memory()["pool_in_use_bytes"]
        with pytest.raises(T.TrinityError, match=r"rc=-3: tri_perc_match: 4294967296 pairs \(fewer than 2\^32 a call"):
            p.match(np.zeros(65537, np.uint64), *empty)
        assert dev.memory()["pool_in_use_bytes"] == held
        with pytest.raises(T.TrinityError, match=r"rc=-3: tri_perc_match: 4294901760 pairs bring the call's scratch to \d+ bytes: above perc_max_bytes"):
            p.match(np.zeros(65536, np.uint64), *empty)
        assert dev.memory()["pool_in_use_bytes"] == held
        r = p.match(np.zeros(4, np.uint64), *empty)
        try:
            for order, (wq, wd) in ((T.PERC_BY_QUERY, (np.repeat(np.arange(nq), 3), np.tile(np.arange(3), nq))), (T.PERC_BY_DOCUMENT, (np.tile(np.arange(nq), 3), np.repeat(np.arange(3), nq)))):
                gq, gd = r.pairs(order)
                assert np.array_equal(gq, wq) and np.array_equal(gd, wd)
            assert r.doc_counts().tolist() == [nq] * 3 and r.info["pairs"] == 3 * nq and r.info["hit_queries"] == r.info["evaluated"] == nq and r.info["ndocs"] == 3
        finally:
            r.close()
        assert dev.memory()["pool_in_use_bytes"] == held
    finally:
        p.close()
    assert dev.memory()["pool_in_use_bytes"] == before


def test_scratch_refusals_at_every_block(T, dev):
    """perc_max_bytes one byte under what a call takes: a call that answers pairs is refused at the third block, one whose candidates hit nothing at the second"""
    progs, docs, nterms = PC.family_some()
    progs = progs + [PC.tk(7, 0) + [T.tok(T.OP_AND, 2)]]  # (terms no other program of the family names)
    arrays = PC.arrays_of(docs)
    lone = PC.arrays_of([{7: [1]}, {7: [2]}])  # the first of two AND-ed terms: a candidate, no pair
    was = dev.get_option("perc_max_bytes")
    before = dev.memory()["pool_in_use_bytes"]
    p = T.Percolator(dev, progs, nterms)
    try:
        held = dev.memory()["pool_in_use_bytes"]
        all3 = check(T, p, progs, arrays, docs)
        r = p.match(*lone)
        two = r.info
        r.close()
        assert all3["pairs"] > 0 and two["pairs"] == 0 and two["evaluated"] == 1 and two["hit_queries"] == 0 and 0 < two["scratch_bytes"]
        try:
            dev.set_option("perc_max_bytes", all3["scratch_bytes"] - 1)
            with pytest.raises(T.TrinityError, match=r"rc=-3: tri_perc_match: %d pairs bring the call's scratch to %d bytes: above perc_max_bytes = %d" % (all3["pairs"], all3["scratch_bytes"], all3["scratch_bytes"] - 1)):
                p.match(*arrays)
            dev.set_option("perc_max_bytes", all3["scratch_bytes"])
            check(T, p, progs, arrays, docs)  # (the bound itself is allowed)
            dev.set_option("perc_max_bytes", two["scratch_bytes"] - 1)
            with pytest.raises(T.TrinityError, match=r"rc=-3: tri_perc_match: 1 candidate queries of 1 match words bring the call's scratch to %d bytes: above perc_max_bytes = %d" % (two["scratch_bytes"], two["scratch_bytes"] - 1)):
                p.match(*lone)
        finally:
            dev.set_option("perc_max_bytes", was)
        assert dev.memory()["pool_in_use_bytes"] == held
        assert check(T, p, progs, arrays, docs)["scratch_bytes"] == all3["scratch_bytes"]
    finally:
        p.close()
    assert dev.memory()["pool_in_use_bytes"] == before
