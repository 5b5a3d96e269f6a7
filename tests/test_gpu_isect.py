"""Trinity::intersect on the device (tri_isect_run; csrc/k_isect.hpp, csrc/isect_side.hpp) against the plain-Python restatement of intersect.cpp
(tests/isect_cases.py), in both codecs.  tri_isect_results and tri_isect_histogram must equal the restatement exactly: masks and counts, and for H the first docIDs
too.  The cases are named in isect_cases.cases(): each is a place the kernels can go wrong.  Everything is an integer and compares exactly."""
import ctypes as C

import numpy as np
import pytest

import isect_cases as IC
import oracle_lib as O

pytestmark = pytest.mark.gpu
TRI_ERR_INVALID, TRI_ERR_UNSUPPORTED = -1, -3
UNK = 0xFFFFFFFF


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
def geometry(T, dev):
    """(span, LDS slots) as tri_isect_info states them: the cases are built from these, so that they sit on the kernels' real boundaries"""
    import structured as S

    ix = S.build({"one": (np.array([1], dtype=np.uint32), np.array([1], dtype=np.uint32))}, docs_cnt=1).upload(T, dev, 1)
    try:
        x = ix.intersect([([[0]], 0)])
        info = x.info()
        x.close()
    finally:
        ix.close()
    return info["span_docs"], info["lds_slots"]


@pytest.fixture(scope="module")
def world(T, dev, geometry):
    """The cases' corpus uploaded in both codecs with the cases' masked documents installed, and every case's expected answers (computed once)."""
    cs = IC.cases(*geometry)
    masked = IC.masked_of(cs)
    corp = IC.corpus(cs)
    ixs = {codec: corp.upload(T, dev, codec) for codec in (1, 2)}
    for ix in ixs.values():
        ix.set_masked(masked)
    want = {c.name: IC.restate(c.posting_groups(), c.stop, masked) for c in cs}
    yield cs, corp, ixs, want, masked
    for ix in ixs.values():
        ix.close()


def request(c, corp):
    terms, counts = c.term_ids(corp.tid)
    groups, at = [], 0
    for n in counts:
        groups.append(terms[at : at + n])
        at += n
    return groups, c.stop


def hist_of(H):
    return sorted((m, n, f) for m, (n, f) in H.items())


def check(isect, r, want, tag):
    lst, H, _ = want
    assert isect.results(r) == lst, tag
    assert isect.histogram(r) == hist_of(H), tag


# ---- cases 1 .. 13: one request a call, then all of them in one call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [1, 2])
def test_named_cases(world, codec):
    cs, corp, ixs, want, _ = world
    ix = ixs[codec]
    for c in cs:
        x = ix.intersect([request(c, corp)])
        try:
            assert x.status() == [0], c.name
            check(x, 0, want[c.name], (c.name, codec))
            info = x.info()
            assert info["h_size"] == [len(want[c.name][1])]
            if c.name == "spill":
                assert info["lds_spills"][0] > 0 and info["h_size"][0] > info["lds_slots"]
            else:
                assert info["lds_spills"] == [0]
            if c.name == "unknown_all":
                assert info["rows"] == 0 and info["passes"] == 0 and x.results(0) == [] and x.histogram(0) == []
            else:
                assert info["passes"] == 2 and info["c_size"][0] > 0
        finally:
            x.close()
    x = ix.intersect([request(c, corp) for c in cs])
    try:
        assert x.status() == [0] * len(cs)
        for r, c in enumerate(cs):
            check(x, r, want[c.name], (c.name, codec, "batch"))
    finally:
        x.close()


def test_the_rows_are_built_once_for_shared_terms(world):
    """two requests that share terms in one call (case 14): the second names the first's groups in reverse order, with a stop word, plus one term of another case"""
    cs, corp, ixs, want, masked = world
    by = {c.name: c for c in cs}
    a = by["masked"]
    g, _ = request(a, corp)
    extra = corp.tid["step.a"]
    b_groups = [g[2], g[1], g[0], [extra]]
    pg = a.posting_groups()
    b_want = IC.restate([pg[2], pg[1], pg[0], [by["step"].lists["step.a"]]], 1 << 3, masked)
    x = ixs[1].intersect([(g, a.stop), (b_groups, 1 << 3)])
    try:
        assert x.status() == [0, 0]
        check(x, 0, want["masked"], "first")
        check(x, 1, b_want, "second")
        assert x.info()["rows"] == 4  # a, b, c once + step.a
        assert x.info()["row_bytes"] * 4 <= x.info()["scratch_bytes"]
    finally:
        x.close()


def test_a_table_overflow_is_per_request(world, dev):
    """isect_max_masks of a handful (case 15): the request with hundreds of masks answers TRI_ERR_UNSUPPORTED, the others of the call are right; likewise isect_max_runs"""
    cs, corp, ixs, want, _ = world
    by = {c.name: c for c in cs}
    reqs = [request(by[n], corp) for n in ("step", "spill", "epochs")]
    L = __import__("trinity_amd").engine.hip_lib()
    old = dev.get_option("isect_max_masks"), dev.get_option("isect_max_runs")
    try:
        dev.set_option("isect_max_masks", 8)
        x = ixs[2].intersect(reqs)
        try:
            assert x.status() == [0, TRI_ERR_UNSUPPORTED, 0] and x.info()["max_masks"] == 8
            check(x, 0, want["step"], "step")
            check(x, 2, want["epochs"], "epochs")
            n = C.c_size_t(77)
            assert L.tri_isect_results(x.h, 1, None, None, 0, C.byref(n)) == TRI_ERR_UNSUPPORTED and n.value == 77
            assert L.tri_isect_histogram(x.h, 1, None, None, None, 0, C.byref(n)) == TRI_ERR_UNSUPPORTED and n.value == 77
        finally:
            x.close()
        dev.set_option("isect_max_masks", old[0])
        dev.set_option("isect_max_runs", 1)  # `epochs` credits three (mask, epoch) keys, `step` one
        x = ixs[1].intersect([reqs[0], reqs[2]])
        try:
            assert x.status() == [0, TRI_ERR_UNSUPPORTED]
            check(x, 0, want["step"], "step")
        finally:
            x.close()
    finally:
        dev.set_option("isect_max_masks", old[0])
        dev.set_option("isect_max_runs", old[1])
    # the row budget: the whole call is refused, nothing is returned
    oldb = dev.get_option("isect_max_bytes")
    try:
        dev.set_option("isect_max_bytes", 1000)
        out = C.c_void_p(5)
        rq = (__import__("trinity_amd").engine.TriIsectRequest * 1)()
        rq[0].ngroups = 1
        t = np.array([corp.tid["step.a"]], dtype=np.uint32)
        gf = np.array([0, 1], dtype=np.uint32)
        assert L.tri_isect_run(ixs[1].h, rq, 1, t.ctypes.data, gf.ctypes.data, C.byref(out)) == TRI_ERR_UNSUPPORTED and out.value == 5
        assert b"isect_max_bytes" in L.tri_last_error()
    finally:
        dev.set_option("isect_max_bytes", oldb)


def test_refusals(T, world):
    """every refusal (case 16): TRI_ERR_INVALID, nothing written"""
    cs, corp, ixs, want, _ = world
    ix = ixs[1]
    L = T.engine.hip_lib()
    Req = T.engine.TriIsectRequest
    nterms = len(corp.names)
    out = C.c_void_p(5)

    def run(ngroups, terms, first, reserved=0, nreq=1):
        rq = (Req * nreq)()
        for r in range(nreq):
            rq[r].ngroups, rq[r].reserved = ngroups, reserved
        t = np.array(list(terms) + [0], dtype=np.uint32)
        gf = np.array(first, dtype=np.uint32)
        return L.tri_isect_run(ix.h, rq, nreq, t.ctypes.data, gf.ctypes.data, C.byref(out))

    rq = (Req * 1)()
    rq[0].ngroups = 1
    buf = np.zeros(8, dtype=np.uint32)
    for args in ((None, rq, 1, buf.ctypes.data, buf.ctypes.data, C.byref(out)), (ix.h, None, 1, buf.ctypes.data, buf.ctypes.data, C.byref(out)),
                 (ix.h, rq, 1, None, buf.ctypes.data, C.byref(out)), (ix.h, rq, 1, buf.ctypes.data, None, C.byref(out)), (ix.h, rq, 1, buf.ctypes.data, buf.ctypes.data, None)):  # fmt: skip
        assert L.tri_isect_run(*args) == TRI_ERR_INVALID and b"null argument" in L.tri_last_error()
    assert run(0, [], [0]) == TRI_ERR_INVALID and b"groups" in L.tri_last_error()
    assert run(65, [0] * 65, list(range(66))) == TRI_ERR_INVALID and b"groups" in L.tri_last_error()
    assert run(2, [0, 1], [0, 2, 1]) == TRI_ERR_INVALID and b"ascend" in L.tri_last_error()
    assert run(1, [nterms], [0, 1]) == TRI_ERR_INVALID and b"out of range" in L.tri_last_error()
    assert run(1, [0xFFFFFFFE], [0, 1]) == TRI_ERR_INVALID
    assert run(1, [0], [0, 1], reserved=1) == TRI_ERR_INVALID and b"reserved" in L.tri_last_error()
    assert out.value == 5
    assert run(1, [UNK], [0, 1]) == 0 and out.value != 5  # 0xffffffff is an unknown token, not a refusal
    L.tri_isect_destroy(out)
    # the result calls: a cap that is too small, a request that does not exist, null arguments
    c = next(c for c in cs if c.name == "epochs")
    x = ix.intersect([request(c, corp)])
    try:
        n = C.c_size_t(77)
        m, k, f = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        assert L.tri_isect_results(x.h, 0, m.ctypes.data, k.ctypes.data, 1, C.byref(n)) == TRI_ERR_INVALID and b"room for 1" in L.tri_last_error()
        assert L.tri_isect_histogram(x.h, 0, m.ctypes.data, k.ctypes.data, f.ctypes.data, 2, C.byref(n)) == TRI_ERR_INVALID and b"room for 2" in L.tri_last_error()
        assert L.tri_isect_results(x.h, 1, m.ctypes.data, k.ctypes.data, 8, C.byref(n)) == TRI_ERR_INVALID
        assert L.tri_isect_histogram(x.h, 1, m.ctypes.data, k.ctypes.data, f.ctypes.data, 8, C.byref(n)) == TRI_ERR_INVALID
        assert L.tri_isect_results(x.h, 0, m.ctypes.data, None, 8, C.byref(n)) == TRI_ERR_INVALID
        assert L.tri_isect_results(x.h, 0, m.ctypes.data, k.ctypes.data, 8, None) == TRI_ERR_INVALID
        assert L.tri_isect_histogram(x.h, 0, m.ctypes.data, k.ctypes.data, None, 8, C.byref(n)) == TRI_ERR_INVALID
        assert L.tri_isect_status(x.h, None) == TRI_ERR_INVALID and L.tri_isect_get_info(x.h, None) == TRI_ERR_INVALID
        assert n.value == 77 and not m.any() and not k.any() and not f.any()
    finally:
        x.close()


def test_the_masked_set_of_the_moment_applies(world):
    """the index's masked set as it stands at the call: cleared, the `masked` case's document breaks its run; installed again, the answer is the first one"""
    cs, corp, ixs, want, masked = world
    c = next(c for c in cs if c.name == "masked")
    ix = ixs[2]
    try:
        ix.set_masked([])
        x = ix.intersect([request(c, corp)])
        bare = IC.restate(c.posting_groups(), c.stop, ())
        assert bare[0] != want["masked"][0]
        check(x, 0, bare, "no masked set")
        x.close()
    finally:
        ix.set_masked(masked)
    x = ix.intersect([request(c, corp)])
    check(x, 0, want["masked"], "masked set back")
    x.close()


# ---- the look-back over more than 64 spans ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [1, 2])
def test_tall_lookback(T, dev, codec, geometry):
    cs = IC.tall_cases(geometry[0])
    corp = IC.corpus(cs)
    ix = corp.upload(T, dev, codec)
    try:
        x = ix.intersect([request(c, corp) for c in cs])
        assert x.info()["nspans"] > 64 + 4
        for r, c in enumerate(cs):
            check(x, r, IC.restate(c.posting_groups(), c.stop, (), top=c.top), (c.name, codec))
        x.close()
    finally:
        ix.close()


# ---- table C beyond 4 x 2^groups entries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [1, 2])
def test_dense_requests_whose_runs_outnumber_their_groups(T, dev, codec):
    """5 and 6 tokens, most of them common, rare ones arriving late: hundreds of (mask, epoch) keys — C is sized from pass 1's histogram, so the requests are
    answered, not refused; with isect_max_runs below their need they are refused and the message names the option"""
    cs = IC.dense_cases()
    corp = IC.corpus(cs)
    ix = corp.upload(T, dev, codec)
    try:
        ix.set_masked(IC.masked_of(cs))
        wants = [IC.restate(c.posting_groups(), 0, IC.masked_of(cs)) for c in cs]
        x = ix.intersect([request(c, corp) for c in cs])
        assert x.status() == [0, 0]
        info = x.info()
        for r, (c, w) in enumerate(zip(cs, wants)):
            check(x, r, w, (c.name, codec))
            assert info["c_size"][r] > 4 * 2 ** len(c.groups)
        assert info["max_runs"] >= max(info["c_size"])
        x.close()
        old = dev.get_option("isect_max_runs")
        try:
            dev.set_option("isect_max_runs", 4 * 2 ** 5)
            x = ix.intersect([request(cs[0], corp)])
            assert x.status() == [TRI_ERR_UNSUPPORTED] and x.info()["max_runs"] == 4 * 2 ** 5
            x.close()
        finally:
            dev.set_option("isect_max_runs", old)
    finally:
        ix.close()


# ---- case 17: an i.i.d. corpus -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [1, 2])
def test_zipf_terms_of_a_random_corpus(T, dev, codec):
    D, V = 100000, 10000
    seg = T.Segment(D, V, 10, 42, codec=codec)
    gseg = seg if codec == 1 else T.Segment(D, V, 10, 42)
    ora = O.Index.wrap(gseg.index, gseg.terms, gseg.docs_cnt, gseg.sum_terms_docs, gseg.sum_term_hits)  # (the CPU oracle's decoder: the postings the restatement walks)
    ix = T.Index.from_segment(dev, seg)
    try:
        q = T.gen_queries(V, 7, 3, 5)
        rows = [r.tolist() for r in q if len(set(r.tolist())) == 5][:2]
        assert rows
        masked = O.masked_docs(D, 3, 20).tolist()
        ix.set_masked(masked)
        reqs, wants = [], []
        for row in rows:
            groups = [[t] for t in row]
            reqs.append((groups, 0))
            wants.append(IC.restate([[ora.decode_term(t)[0]] for t in row], 0, masked, top=D + 1))
            reqs.append(([[row[0], row[1]], [row[2]], [row[3], UNK], [row[4]]], 1 << 1))  # synonyms, an unknown token, a stop word
            wants.append(IC.restate([[ora.decode_term(row[0])[0], ora.decode_term(row[1])[0]], [ora.decode_term(row[2])[0]], [ora.decode_term(row[3])[0], IC.UNKNOWN],
                                     [ora.decode_term(row[4])[0]]], 1 << 1, masked, top=D + 1))  # fmt: skip
        x = ix.intersect(reqs)
        assert x.status() == [0] * len(reqs)
        for r, w in enumerate(wants):
            assert w[2] <= 255 and len(w[1]) > 4
            check(x, r, w, (codec, r))
        x.close()
    finally:
        ix.close()
