"""GPU tests of the WRITE side on structured inputs (run with -m gpu on an MI355X): tri_encode_google[_payloads], tri_encode_lucene, tri_commit_google / _lucene and
tri_merge_google / _lucene over the cases of tests/write_cases.py — inputs that sit on the kernels' boundaries (every varint length class, every skiplist phase, the
65535-entry cap, the scans' round and chunk sizes, termIDs whose high bits wrap in the commit key, sessions commit must refuse, merges on k_merge_select's edges) —
and the genuine reference's own commit and merge fixtures fed through the device.

Everything is byte-exact: the device's bytes, term tables and statistics equal the host encoders' over the plain references of write_cases.py (the commit walk
tests/golden/ref_commit.json pins, merge_restated.merge_term with masks); there are no tolerances.  tests/test_write_cases.py shows on the CPU that every case reaches
what it is there for and that the reference side reads the host encoders' bytes back.

Segments whose documentIDs exceed about 10^6 are never uploaded (the index's per-document bitmaps scale with the highest documentID): those cases are checked by bytes
only.  One device handle for the file; every uploaded index is closed; nothing retries."""
import contextlib
import re

import numpy as np
import pytest

import write_cases as W

pytestmark = pytest.mark.gpu
UPLOAD_MAX_DOC = 1_000_000
SESSIONS = {s.name: s for s in W.commit_sessions()}


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


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = W.encoder_cases()[name]()
        return made[name]

    return get


def same_bytes(got, want, tag):
    """Byte for byte; on a mismatch the case and the first differing offset."""
    n = min(got.size, want.size)
    diff = np.flatnonzero(got[:n] != want[:n])
    assert got.size == want.size and not diff.size, (tag, "sizes", got.size, want.size, "first differing offset", int(diff[0]) if diff.size else n)


def same_terms(got, want, tag):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1)) if len(got) == len(want) else [-1]
    assert not len(bad), (tag, "term table, first differing term", int(bad[0]))


@contextlib.contextmanager
def uploaded(T, dev, *args, **kw):
    ix = T.Index(dev, *args, **kw)
    try:
        yield ix
    finally:
        ix.close()


def decodes_back(ix, docs, freqs, tf, tag):
    """Every term through the read side's decoder, 16384 terms a call (tri_decode_terms launches one grid row per requested term)."""
    df = np.diff(tf.astype(np.int64))
    for t0 in range(0, df.size, 16384):
        t1 = min(t0 + 16384, df.size)
        d2, f2, _ = ix.decode_terms(np.arange(t0, t1, dtype=np.uint32), df[t0:t1])
        a, b = int(tf[t0]), int(tf[t1])
        assert np.array_equal(d2, docs[a:b]) and np.array_equal(f2, freqs[a:b]), (tag, t0)


# ------------------------------------------------------------------------------------------ the encoders
@pytest.mark.parametrize("name", [n for n in W.GOOGLE_ENCODER_CASES if n != "google_skip_cap"])
def test_google_encoder_on_structured_cases(T, dev, cases, name):
    from trinity_amd import engine as E

    c = cases(name)
    want, wterms = E.host_encode_google(*c.arrays)
    got, gterms = dev.encode_google(*c.arrays)
    same_terms(gterms, wterms, name)
    same_bytes(got, want, name)
    if c.upload and c.docs.size:
        assert int(c.docs.max()) <= UPLOAD_MAX_DOC
        with uploaded(T, dev, got, gterms, int(c.docs.max())) as ix:
            decodes_back(ix, c.docs, c.freqs, c.tf, name)


def test_google_encoder_keeps_65535_skiplist_entries(T, dev, cases):
    """One term of (65535 + 2) * 8 blocks: 65537 of its blocks are marked, 65535 entries are kept.  The cap is not pinned by any run of the reference: it rests on
    google_codec.cpp:146-158 as mirrored in csrc/host/google_encoder.hpp, whose bytes are the checker here (decoding the term through the oracle takes half a minute).
    The segment (highest documentID 16 777 472) is uploaded and the long term decodes back to the input."""
    from trinity_amd import engine as E

    c = cases("google_skip_cap")
    want, wterms = E.host_encode_google(*c.arrays)
    got, gterms = dev.encode_google(*c.arrays)
    same_terms(gterms, wterms, c.name)
    same_bytes(got, want, c.name)
    off = int(gterms[1, 1])
    assert int(got[off]) | (int(got[off + 1]) << 8) == W.SKIP_CAP
    a, b = int(c.tf[1]), int(c.tf[2])
    with uploaded(T, dev, got, gterms, int(c.docs.max())) as ix:
        d2, f2, _ = ix.decode_terms(np.array([1], dtype=np.uint32), [b - a])
        assert np.array_equal(d2, c.docs[a:b]) and np.array_equal(f2, c.freqs[a:b])


@pytest.mark.parametrize("name", W.LUCENE_ENCODER_CASES)
def test_lucene_encoder_on_structured_cases(T, dev, cases, name):
    from trinity_amd import hostplan as HP

    c = cases(name)
    wi, wh, wt = HP.lucene_encode(c.docs, c.freqs, c.pos, c.tf)
    gi, gh, gt = dev.encode_lucene(c.docs, c.freqs, c.pos, c.tf)
    same_terms(gt, wt, name)
    same_bytes(gi, wi, (name, "index"))
    same_bytes(gh, wh, (name, "hits.data"))
    if c.upload and name.startswith("google_skip_phases"):
        with uploaded(T, dev, gi, gt, int(c.docs.max()), codec=2, hits=gh) as ix:
            decodes_back(ix, c.docs, c.freqs, c.tf, name)


# ------------------------------------------------------------------------------------------ commit
def commit_params():
    return [(n, p) for n, s in SESSIONS.items() for p in (False, True) if p or not s.needs_payloads]


@pytest.mark.parametrize("name,payloads", commit_params())
def test_commit_on_structured_sessions(T, dev, name, payloads):
    """Accepted sessions: the committed termIDs in order, term table, bytes and stats equal the plain reference's (and, payload-less, the Lucene-shaped commit's too).
    Refused sessions: TrinityError naming the smallest offending SORTED posting and the reason (`sorted posting N: ...`, commit_device), the pool's bytes in use unchanged."""
    from trinity_amd import engine as E
    from trinity_amd import hostplan as HP

    s = SESSIONS[name]
    tids, docs, freqs, pos, plen, pval = s.arrays
    pl, pv = (plen, pval) if payloads else (None, None)
    if s.refusal:
        j, _ = W.first_offence(s, payloads)
        calls = [lambda: dev.commit_google(tids, docs, freqs, pos, pl, pv)] + ([] if payloads else [lambda: dev.commit_lucene(tids, docs, freqs, pos)])
        for call in calls:
            before = dev.memory()["pool_in_use_bytes"]
            with pytest.raises(T.TrinityError, match=rf"sorted posting {j}: .*{re.escape(s.refusal)}"):
                call()
            assert dev.memory()["pool_in_use_bytes"] == before, name
        return
    wtids, arrays, wstats = W.commit_reference(s, payloads)
    want, wterms = E.host_encode_google(*arrays)
    got, gtids, gterms, stats = dev.commit_google(tids, docs, freqs, pos, pl, pv)
    assert gtids.tolist() == wtids.tolist(), name
    same_terms(gterms, wterms, name)
    same_bytes(got, want, name)
    assert stats == wstats, name
    if not payloads:
        wi, wh, wt = HP.lucene_encode(*arrays[:4])
        li, lh, ltids, lterms, lstats = dev.commit_lucene(tids, docs, freqs, pos)
        assert ltids.tolist() == wtids.tolist() and lstats == wstats, name
        same_terms(lterms, wt, name)
        same_bytes(li, wi, (name, "index"))
        same_bytes(lh, wh, (name, "hits.data"))


def test_reference_commit_sessions_on_the_device(T, dev):
    """tests/golden/ref_commit.json: the sessions the genuine SegmentIndexSession::commit was fed, in their insertion order, through tri_commit_google — the reference's
    `index` byte for byte and its dictionary's (documents, chunk offset, chunk size) for every term."""
    for rec, s in W.golden_commit_sessions():
        got, gtids, gterms, stats = dev.commit_google(*s.arrays)
        same_bytes(got, np.frombuffer(bytes.fromhex(rec["index"]), dtype=np.uint8), s.name)
        name_of = {t["id"]: t["w"] for d in rec["docs"] for t in d["terms"]}
        ref_terms = {t["w"]: (t["documents"], t["offset"], t["size"]) for t in rec["terms"]}
        assert len(gtids) == len(ref_terms) and stats["docs_cnt"] == len(rec["docs"])
        assert [ref_terms[name_of[int(i)]] for i in gtids] == [tuple(int(x) for x in row) for row in gterms], s.name


# ------------------------------------------------------------------------------------------ merge
@contextlib.contextmanager
def participants(T, dev, case, docs_cnt=None):
    """The case's participants encoded with the host encoders and uploaded, each with its masked documents installed; closed on the way out."""
    from trinity_amd import engine as E
    from trinity_amd import hostplan as HP

    ixs = []
    try:
        for p in case.parts:
            if case.codec == 1:
                index, terms = E.host_encode_google(p.docs, p.freqs, p.pos, p.tf, p.plen, p.pval)
                ixs.append(T.Index(dev, index, terms, docs_cnt or p.docs_cnt))
            else:
                index, hits, terms = HP.lucene_encode(p.docs, p.freqs, p.pos, p.tf)
                ixs.append(T.Index(dev, index, terms, docs_cnt or p.docs_cnt, codec=2, hits=hits))
            if p.masked is not None:
                ixs[-1].set_masked(p.masked)
        yield ixs
    finally:
        for ix in ixs:
            ix.close()


MERGES = {(codec, m.name): m for codec in (1, 2) for m in W.merge_cases(codec)}


@pytest.mark.parametrize("codec,name", list(MERGES))
def test_merge_on_structured_sets(T, dev, codec, name):
    """Bytes, term table and stats equal the host encoder's over merge_restated.merge_term's kept postings; the merged segment uploads and decodes back to them; for the
    GOOGLE codec the kept hits and payloads read back through the oracle over the MERGED bytes."""
    from trinity_amd import engine as E
    from trinity_amd import hostplan as HP

    m = MERGES[(codec, name)]
    merged, arrays, wstats = W.merge_reference(m)
    docs, freqs, pos, tf, plen, pval = arrays
    docs_cnt = max(p.docs_cnt for p in m.parts)
    with participants(T, dev, m) as ixs:
        if codec == 1:
            want, wterms = E.host_encode_google(*arrays)
            got, gterms, stats = dev.merge_google(ixs, m.part_terms)
        else:
            want, wh, wterms = HP.lucene_encode(docs, freqs, pos, tf)
            got, gh, gterms, stats = dev.merge_lucene(ixs, m.part_terms)
            same_bytes(gh, wh, (name, "hits.data"))
        same_terms(gterms, wterms, name)
        same_bytes(got, want, (name, "index"))
        assert stats == wstats, name
    with uploaded(T, dev, got, gterms, docs_cnt, **({} if codec == 1 else {"codec": 2, "hits": gh})) as ix:
        decodes_back(ix, docs, freqs, tf, name)
    if codec == 1:
        W.oracle_read_back(name, arrays, got, gterms)


def test_reference_merges_on_the_device(T, dev):
    """tests/golden/ref_merge.json: the participants the genuine Codecs::Google::IndexSession::merge read, encoded with the host encoder from the fixture's input postings,
    uploaded and merged by tri_merge_google — every output term's chunk byte for byte, its (documents, offset, size), and the output session's length."""
    for rec, m in W.golden_merge_cases():
        with participants(T, dev, m, docs_cnt=rec["maxdoc"]) as ixs:
            got, gterms, stats = dev.merge_google(ixs, m.part_terms)
        assert got.size == rec["out_len"], m.name
        for t, o in enumerate(rec["out"]):
            assert (int(gterms[t, 0]), int(gterms[t, 1]), int(gterms[t, 2])) == (o["documents"], o["offset"], o["size"]), (m.name, o["g"])
            same_bytes(got[o["offset"] : o["offset"] + o["size"]], np.frombuffer(bytes.fromhex(o["chunk"]), dtype=np.uint8), (m.name, o["g"]))
        assert stats["sum_terms_docs"] == sum(o["documents"] for o in rec["out"])
