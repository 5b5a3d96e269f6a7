"""The write side's structured cases (tests/write_cases.py) on the CPU: every case reaches the boundary it is there for, and its inputs are ones the reference side accepts.

  * every case's `reaches` is RECOMPUTED from its arrays (varint classes from the values, block bodies from the lengths of their parts, skip phases from block counts,
    scan sizes from array lengths) and tied to the host encoder's bytes (every chunk's size and skiplist entry count); the union over all cases is write_cases.CLASSES;
  * the host encoder's bytes of every GOOGLE case decode back through the oracle to the input — documents, frequencies, positions, payload lengths, payload bytes (masked
    to each payload's own length: term_hit::payload keeps the bytes a shorter payload does not overwrite) — and PLI.advance around every skiplist-marked block lands where
    numpy's searchsorted says;
  * the Lucene-shaped encoder's units (what one lane of the device encoder runs) equal the sequential encoder on every Lucene case, byte for byte;
  * the restated commit walk reproduces tests/golden/ref_commit.json, and the commit and merge references over the structured cases are accepted by the host encoders."""
import numpy as np
import pytest

import oracle_lib as O
import structured as S
import trinity_amd as T
import write_cases as W
from trinity_amd import engine as E
from trinity_amd import hostplan as HP


@pytest.fixture(scope="module", autouse=True)
def built():
    T.build.build_host()
    O.lib()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = W.encoder_cases()[name]()
        return made[name]

    return get


def test_constants_mirror_the_headers():
    k = S.header_constants("dev_structs.hpp", "k_encode.hpp", "pfor128_group.hpp", "lucene_enc_units.hpp")
    assert k["ENC_SCAN_CHUNK"] == W.ENC_SCAN_CHUNK and k["LENC_BLOCK"] == 128
    assert sorted(set(W.CLASSES)) == sorted(W.CLASSES)  # (no class listed twice)


def entry_counts(index, terms):
    return [int(index[int(o)]) | (int(index[int(o) + 1]) << 8) for o in terms[:, 1].tolist()]


def test_every_case_reaches_what_it_declares(cases):
    """... and the union is the full list.  The 65535-entry cap is not pinned by any reference run: it rests on google_codec.cpp:146-158 as mirrored in
    csrc/host/google_encoder.hpp (`skiplist.size() / 8 < UINT16_MAX`); the cap case is checked here against that mirror's entry count."""
    declared = set()
    for name in W.GOOGLE_ENCODER_CASES:
        c = cases(name)
        index, terms = E.host_encode_google(*c.arrays)
        if name == "google_skip_cap":
            got, entries = W.skip_classes(c.tf)
            assert entries == [0, W.SKIP_CAP]
        else:
            got = W.google_classes(c)
            entries = W.skip_classes(c.tf)[1]
            assert terms[:, 2].tolist() == c.chunk_sizes, name  # (the recomputed varint lengths and bodies add up to the encoder's chunks)
        assert entry_counts(index, terms) == entries, name
        assert c.reaches and c.reaches <= got, (name, sorted(c.reaches - got))
        declared |= c.reaches
    c = cases("lucene_blocks")
    got = W.lucene_classes(c)
    assert c.reaches <= got, sorted(c.reaches - got)
    declared |= c.reaches
    for s in W.commit_sessions():
        got = W.commit_classes(s)
        assert s.reaches and s.reaches <= got, (s.name, sorted(s.reaches - got))
        assert (W.first_offence(s, True) is not None) == (s.refusal is not None), s.name
        declared |= s.reaches
    for codec in (1, 2):
        for m in W.merge_cases(codec):
            got = W.merge_classes(m, W.merge_reference(m)[0])
            assert m.reaches and m.reaches <= got, (m.name, codec, sorted(m.reaches - got))
            declared |= m.reaches
    assert declared == set(W.CLASSES), (sorted(set(W.CLASSES) - declared), sorted(declared - set(W.CLASSES)))


def check_advance(c, ora, entries):
    """PLI.advance to a target inside, before and after every skiplist-marked block of every term that has entries."""
    nb = (np.diff(c.tf.astype(np.int64)) + 31) // 32
    g0 = np.concatenate([[0], np.cumsum(nb)])
    checked = 0
    for t in np.flatnonzero(np.array(entries) > 0).tolist():
        docs = c.docs[int(c.tf[t]) : int(c.tf[t + 1])].astype(np.int64)
        first_marked = (int(g0[t]) + 8) // 8 * 8 - 1
        for e in range(entries[t]):
            j = first_marked + 8 * e - int(g0[t])  # the marked block's index in its term
            lo, hi = 32 * j, min(32 * j + 32, docs.size)
            targets = {int(docs[lo]), int(docs[lo]) - 1, int(docs[hi - 1]), int(docs[hi - 1]) + 1, int(docs[(lo + hi) // 2]) + 1, int(docs[max(lo - 1, 0)]), int(docs[-1]) + 1}
            for target in sorted(targets):
                k = int(np.searchsorted(docs, target))
                want = int(docs[k]) if k < docs.size else O.DOCIDS_END
                assert O.PLI(ora, t).advance(target) == want, (c.name, t, e, target)
                checked += 1
    return checked


@pytest.mark.parametrize("name", [n for n in W.GOOGLE_ENCODER_CASES if n != "google_skip_cap"])
def test_google_cases_decode_back_through_the_oracle(cases, name):
    c = cases(name)
    index, terms = E.host_encode_google(*c.arrays)
    ora = W.oracle_read_back(c.name, c.arrays, index, terms)
    checked = check_advance(c, ora, W.skip_classes(c.tf)[1])
    assert checked > 0 or not name.startswith("google_skip_phases")


@pytest.mark.parametrize("name", W.LUCENE_ENCODER_CASES)
def test_lucene_units_equal_the_sequential_encoder(cases, name):
    c = cases(name)
    wi, wh, wt = HP.lucene_encode(c.docs, c.freqs, c.pos, c.tf)
    ui, uh, ut = HP.lucene_encode(c.docs, c.freqs, c.pos, c.tf, units=True)
    assert np.array_equal(ut, wt), name
    assert ui.size == wi.size and np.array_equal(ui, wi), (name, "index", int(np.argmax(ui[: wi.size] != wi[: ui.size])))
    assert uh.size == wh.size and np.array_equal(uh, wh), (name, "hits.data", int(np.argmax(uh[: wh.size] != wh[: uh.size])))


def test_commit_reference_reproduces_the_reference_index():
    """write_cases.commit_reference (numpy) over the sessions of ref_commit.json, followed by the host encoder: the genuine commit's `index` and dictionary."""
    for rec, s in W.golden_commit_sessions():
        tids, arrays, stats = W.commit_reference(s, True)
        index, terms = E.host_encode_google(*arrays)
        want = np.frombuffer(bytes.fromhex(rec["index"]), dtype=np.uint8)
        assert index.size == want.size and np.array_equal(index, want), rec["seed"]
        name_of = {t["id"]: t["w"] for d in rec["docs"] for t in d["terms"]}
        ref_terms = {t["w"]: (t["documents"], t["offset"], t["size"]) for t in rec["terms"]}
        assert [ref_terms[name_of[int(i)]] for i in tids] == [tuple(int(x) for x in row) for row in terms]
        assert stats["docs_cnt"] == len(rec["docs"])


def test_references_over_the_structured_cases_are_accepted():
    """The restated commit walk and merge walk give term orders and postings both host encoders take (documents ascending within a term, no refusal)."""
    for s in W.commit_sessions():
        if s.refusal:
            continue
        for payloads in (False, True):
            tids, arrays, stats = W.commit_reference(s, payloads)
            assert tids.tolist() == sorted(set(s.tids.tolist()), key=lambda i: (i & 31, i)), s.name
            index, terms = E.host_encode_google(*arrays)
            assert int(terms[:, 0].sum()) == stats["sum_terms_docs"] == s.tids.size and stats["total_terms"] == len(tids), s.name
        HP.lucene_encode(*arrays[:4])
    for codec in (1, 2):
        for m in W.merge_cases(codec):
            merged, arrays, stats = W.merge_reference(m)
            if codec == 1:
                index, terms = E.host_encode_google(*arrays)
            else:
                assert not arrays[4].any()
                index, hits, terms = HP.lucene_encode(*arrays[:4])
            assert terms[:, 0].tolist() == [len(x) for x in merged], (m.name, codec)


def test_merge_reference_reproduces_the_reference_chunks():
    """write_cases.golden_merge_cases (the fixture's participants as merge cases) through merge_reference and the host encoder: the genuine merge's chunks."""
    for rec, m in W.golden_merge_cases():
        merged, arrays, stats = W.merge_reference(m)
        index, terms = E.host_encode_google(*arrays)
        assert index.size == rec["out_len"]
        for t, o in enumerate(rec["out"]):
            assert (int(terms[t, 0]), int(terms[t, 1]), int(terms[t, 2])) == (o["documents"], o["offset"], o["size"]), (m.name, o["g"])
            assert np.array_equal(index[o["offset"] : o["offset"] + o["size"]], np.frombuffer(bytes.fromhex(o["chunk"]), dtype=np.uint8)), (m.name, o["g"])


def test_participants_and_merged_segments_load_on_the_host():
    """Every participant of every merge case, and every merged segment, builds a host index (the walk the upload runs): segments of empty terms only included."""
    for codec in (1, 2):
        for m in W.merge_cases(codec):
            segs = [(p.docs, p.freqs, p.pos, p.tf, p.plen, p.pval, p.docs_cnt) for p in m.parts]
            segs.append(W.merge_reference(m)[1] + (max(p.docs_cnt for p in m.parts),))
            for docs, freqs, pos, tf, plen, pval, docs_cnt in segs:
                if codec == 1:
                    index, terms = E.host_encode_google(docs, freqs, pos, tf, plen, pval)
                    HP.HostIndex(index, terms, docs_cnt)
                else:
                    index, hits, terms = HP.lucene_encode(docs, freqs, pos, tf)
                    HP.HostIndex(index, terms, docs_cnt, codec=2, hits=hits)
