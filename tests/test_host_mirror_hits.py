"""The codec seam's hits through the C++ operator surface (trinity_amd/csrc/host/trinity_gpu.hpp: PostingsListIterator::materialize_hits, DocWordsSpace,
IndexSource::term_hits_at): the driver tests/cpp/host_mirror_hits_test.cpp walks postings lists with next() and advance(), materialises the hits of every document it
stops on and prints them with what the DocWordsSpace then holds; the output must equal the oracle's walk (GOOGLE, a segment with payloads) and the input positions
(LUCENE, the structured cases)."""
import subprocess

import numpy as np
import pytest

import decode_hits_cases as DC
import oracle_lib as O

pytestmark = pytest.mark.gpu
ABSENT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def _run(tmp_path, index, terms, docs_cnt, ta, tb, hits=None):
    from trinity_amd.build import MIRROR_HITS_BIN

    ipath, tpath, hpath = str(tmp_path / "index"), str(tmp_path / "terms"), str(tmp_path / "hits")
    np.asarray(index).tofile(ipath)
    np.ascontiguousarray(terms, dtype=np.uint32).tofile(tpath)
    args = [MIRROR_HITS_BIN, ipath, tpath, str(docs_cnt), str(ta), str(tb)]
    if hits is not None:
        np.asarray(hits).tofile(hpath)
        args.append(hpath)
    res = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stdout.splitlines()


def _expected(lists, ta, tb):
    """The driver's output from {term: {docid: [(pos, len, word)]}} (every document of the two lists)."""
    fmt = lambda hs: "".join(f" {p}:{l}:{w}" for p, l, w in hs)  # noqa: E731
    out = []
    for d, hs in lists[ta].items():
        f = len(hs) & 0xFFFF
        out.append(f"next {d} {f}{fmt(hs[:f])} |" + "".join(" 10" if p else " 00" for p, _, _ in hs[:f]))
    pairs = []
    for d in sorted(set(lists[ta]) & set(lists[tb])):
        a, b = lists[ta][d], lists[tb][d]
        own = {}
        for who, hs in ((1, a), (2, b)):  # one term per position, the last writer wins, position 0 is never set
            for p, _, _ in hs:
                if p:
                    own[p] = who
        out.append(f"both {d} a{fmt(a)} b{fmt(b)} |" + "".join(f" {own.get(p, 0)}" for p, _, _ in a + b))
        pairs += [(ta, d), (tb, d)]
    for t, d in pairs:
        out.append(f"at {t} {d} {len(lists[t][d])}{fmt(lists[t][d])}")
    out += [f"at {ta} 0 {ABSENT}", f"at {tb} {ABSENT} {ABSENT}"]
    return out


def test_google_payload_segment_equals_the_oracle(T, tmp_path):
    index, terms, docs_cnt, postings, hits = DC.payload_case()
    ora = O.Index.wrap(index, terms, docs_cnt, postings, hits)
    lists = {}
    for t in (0, 1):
        it, lists[t] = O.PLI(ora, t), {}
        while True:
            d = it.next()
            if d == O.DOCIDS_END:
                break
            lists[t][d] = list(zip(*it.hits()))
    want = _expected(lists, 0, 1)
    both = [l for l in want if l.startswith("both")]
    taken = [o == "2" for l in both for o in l.split("|")[1].split()[: len(lists[0][int(l.split()[1])])]]
    assert len(both) >= 5 and any(taken) and not all(taken)  # on some documents term b takes a position of term a (the last writer wins)
    assert _run(tmp_path, index, terms, docs_cnt, 0, 1) == want


def test_lucene_structured_cases_equal_the_inputs(T, tmp_path):
    c = DC.corpus()
    ta, tb = c.tid["at100"], c.tid["n261"]
    lists = {}
    for n, t in (("at100", ta), ("n261", tb)):
        lists[t] = {d: [(int(p), 0, 0) for p in c.positions[n][lo : lo + f]] for d, (lo, f) in DC.doc_slices(c, n).items()}
    want = _expected(lists, ta, tb)
    assert sum(l.startswith("both") for l in want) >= 50
    assert _run(tmp_path, c.l_index, c.l_terms, c.docs_cnt, ta, tb, hits=c.l_hits) == want
