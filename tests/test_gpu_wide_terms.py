"""GPU tests of the default mode's WIDE-REPORT queries (run with -m gpu on an MI355X): option rich_max_terms = 64 — queries of 17 .. 64 reportable terms through
k_tree_leaves / k_tree_leaves_wide (64-bit report masks) and k_rich_wide (csrc/k_rich.hpp), read back through tri_batch_query_terms_wide /
tri_batch_matched_terms_wide.  Every reported term, frequency and position against the CPU oracle's default mode (never handed more than 64 distinct terms: it
aborts on a 65th), on both worlds of tests/test_gpu_wide_trees.py and in both codecs."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import World, options, rich_flat
from test_gpu_parity import T, dev  # noqa: F401  (fixtures)
from wide_terms_cases import NARROW, OPTS, OR65, SHAPES, WORLDS, mixed_programs, narrow_programs, shape_programs

pytestmark = pytest.mark.gpu
CASES = [(wi, codec) for wi in range(len(WORLDS)) for codec in (1, 2)]
IDS = [f"{WORLDS[wi][0]}-codec{codec}" for wi, codec in CASES]
NAMES = [sh[0] for sh in SHAPES]


class Ctx:
    """One world in one codec: the index on the device, the oracle, the oracle's default-mode answers (computed once per dropped set and query) and the
    device's answers for the eight shapes at plain options (computed once: tests (d) and (f) compare with them)."""

    def __init__(self, T, dev, wi, codec):
        self.T, self.dev, self.wi = T, dev, wi
        self.w = World(T, dev, *WORLDS[wi], codec=codec)
        self.progs = shape_programs(O)
        self.memo, self._plain = {}, None

    def want(self, key, drop, prog):
        k = (key, prog.tobytes())
        if k not in self.memo:
            self.w.ora.set_masked(drop)
            try:
                self.memo[k] = self.w.ora.exec_rich(prog)
            finally:
                self.w.ora.set_masked(np.zeros(0, np.uint32))
        return self.memo[k]

    def run(self, progs, flags=None, filters=None, runs=1):
        """-> per run, per query (docs, terms, present, freq, positions); the batch's info"""
        T = self.T
        b = T.Batch(self.w.ix, progs, T.FLAG_MATCHED_TERMS if flags is None else flags)
        try:
            assert not b.query_status().any()
            if filters is not None:
                b.set_filters(*filters)
            out = []
            for _ in range(runs):
                b.run()
                b.sync()
                counts = b.counts()
                res = []
                for i in range(len(progs)):
                    docs = b.docset(i, int(counts[i]))
                    res.append((docs,) + b.matched_terms(i, len(docs)))
                out.append(res)
            return out, b.info()
        finally:
            b.close()

    def plain(self):
        if self._plain is None:
            with options(self.dev, **OPTS):
                (self._plain,), info = self.run(self.progs)
            assert info["tree_queries"] == len(self.progs) and info["unsupported_queries"] == 0
        return self._plain


@pytest.fixture(scope="module")
def ctxs(T, dev):
    made = {}

    def get(case):
        if case not in made:
            made[case] = Ctx(T, dev, *case)
        return made[case]

    yield get
    for c in made.values():
        c.w.ix.close()


def bits(present):
    return int(sum(bin(int(x)).count("1") for x in present))


def check_against(res, want, name):
    docs, terms, present, freq, pos = res
    wdocs, wflat, tt, ht = want
    assert np.array_equal(docs, wdocs), name
    print(f"[wide terms] {name}: n {len(docs)} terms_total {bits(present)} (oracle {tt}) hits_total {int(freq.sum())} (oracle {ht})")
    assert int(freq.sum()) == ht and bits(present) == tt, name
    assert np.array_equal(rich_flat(docs, terms, present, freq, pos), wflat), name


def same(a, b, name):
    for x, y in zip(a, b):  # docs, terms, present, freq, positions
        assert x.dtype == y.dtype and np.array_equal(x, y), name


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_shape_reports_what_the_oracle_reports(ctxs, case):
    c = ctxs(case)
    got = c.plain()
    none = np.zeros(0, np.uint32)
    for sh, prog, res in zip(SHAPES, c.progs, got):
        want = c.want("plain", none, prog)
        assert (len(want[0]), want[2], want[3]) == sh[4 + c.wi], sh[0]  # the table
        assert len(res[1]) == sh[3] and res[2].dtype == np.uint64, sh[0]
        check_against(res, want, sh[0])


def test_a_phrase_mask_on_both_sides_of_bit_32_reports_both_terms(ctxs):
    """straddle at D = 2000: t0 is bit 31, t1 bit 32, t2 bit 33.  The documents "t0 t1" matches report t0 and t1, those of "t1 t2" t1 and t2 — 245 and 73 of them."""
    c = ctxs((0, 1))
    docs, terms, present, freq, pos = c.plain()[NAMES.index("straddle")]
    assert terms[31:34].tolist() == [0, 1, 2]
    for text, n, need in (('"t0 t1"', 245, (1 << 31) | (1 << 32)), ('"t1 t2"', 73, (1 << 32) | (1 << 33))):
        pd = c.w.ora.exec(O.parse_query(text), O.FLAG_DOCUMENTS_ONLY)[0]
        assert len(pd) == n
        at = np.searchsorted(docs, pd)
        assert np.array_equal(docs[at], pd) and np.all((present[at] & np.uint64(need)) == np.uint64(need)), text


# ------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_masked_documents_and_per_query_filters(ctxs, case):
    c = ctxs(case)
    T, D = c.T, WORLDS[c.wi][0]
    mask = np.array(sorted(set(np.random.default_rng(3).integers(1, D, D // 7).tolist())), dtype=np.uint32)
    drop = np.array(sorted(set(np.random.default_rng(9).integers(1, D + 1, D // 5).tolist())), dtype=np.uint32)
    both = np.union1d(mask, drop).astype(np.uint32)
    flt = None
    try:
        c.w.ix.set_masked(mask)
        flt = T.Filter(c.w.ix, drop)
        with options(c.dev, **OPTS):
            (masked,), _ = c.run(c.progs)
            (filtered,), _ = c.run(c.progs, filters=([flt], [0 if i % 2 == 1 else T.engine.NO_FILTER for i in range(len(c.progs))]))
        for i, (sh, prog) in enumerate(zip(SHAPES, c.progs)):
            check_against(masked[i], c.want("masked", mask, prog), sh[0] + " masked")
            key, gone = ("both", both) if i % 2 == 1 else ("masked", mask)
            check_against(filtered[i], c.want(key, gone, prog), sh[0] + " masked+filter")
    finally:
        if flt is not None:
            flt.close()
        c.w.ix.set_masked(np.zeros(0, np.uint32))


# ------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_narrow_queries_of_a_mixed_batch_answer_as_they_do_alone(ctxs, case):
    c = ctxs(case)
    mixed, narrow_at = mixed_programs(O)
    (alone,), info_alone = c.run(narrow_programs(O))  # default options
    with options(c.dev, **OPTS):
        b = c.T.Batch(c.w.ix, mixed, c.T.FLAG_MATCHED_TERMS)
        try:
            assert not b.query_status().any()
            b.run()
            b.sync()
            counts = b.counts()
            wide_at = [i for i in range(len(mixed)) if i not in narrow_at]
            for j, qi in enumerate(narrow_at):
                docs = b.docset(qi, int(counts[qi]))
                res = (docs,) + b.matched_terms(qi, len(docs))
                assert res[2].dtype == np.uint32
                same(res, alone[j], NARROW[j])
                wterms, wpresent, wfreq, wpos = b.matched_terms_wide(qi, len(docs))  # the same query through the wide call: the mask zero-extended
                assert wpresent.dtype == np.uint64 and np.all(wpresent >> np.uint64(32) == 0) and np.array_equal(wpresent.astype(np.uint32), res[2]), NARROW[j]
                assert np.array_equal(wterms, res[1]) and np.array_equal(wfreq, res[3]) and np.array_equal(wpos, res[4]), NARROW[j]
            plain = c.plain()
            for j, qi in enumerate(wide_at):
                docs = b.docset(qi, int(counts[qi]))
                same((docs,) + b.matched_terms(qi, len(docs)), plain[j], NAMES[j])
        finally:
            b.close()


# ------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_wide_leaf_kernel_gives_the_narrow_ones_answers(ctxs, case):
    """tree_wide_min_nodes = 0: or17 / or33 / some60 / straddle (at most 64 nodes: k_tree_leaves at plain options) through k_tree_leaves_wide."""
    c = ctxs(case)
    idx = [NAMES.index(n) for n in ("or17", "or33", "some60", "straddle")]
    with options(c.dev, tree_wide_min_nodes=0, **OPTS):
        (forced,), info = c.run([c.progs[i] for i in idx])
    assert info["tree_queries"] == len(idx)
    plain = c.plain()
    for res, i in zip(forced, idx):
        same(res, plain[i], NAMES[i])


# ------------------------------------------------------------------------------------------ (e)
def test_the_narrow_calls_refuse_a_wide_report_query_and_write_nothing(ctxs, T):
    c = ctxs((0, 1))
    L = T.engine.hip_lib()
    with options(c.dev, **OPTS):
        b = T.Batch(c.w.ix, [c.progs[NAMES.index("or64")], O.parse_query("t0 t1")], T.FLAG_MATCHED_TERMS)
    try:
        b.run()
        b.sync()
        n = int(b.counts()[0])
        guard = 0xDEADBEEF
        terms = np.full(17, guard, dtype=np.uint32)  # the caller's 16 words and a guard word behind them
        nt = C.c_uint32(77)
        assert L.tri_batch_query_terms(b.h, 0, terms.ctypes.data, C.byref(nt)) == -1  # TRI_ERR_INVALID
        assert b"tri_batch_query_terms_wide" in L.tri_last_error() and np.all(terms == guard)
        present = np.full(n + 1, guard, dtype=np.uint32)
        freq = np.full((n, 16), 0xBEEF, dtype=np.uint16)
        npos = C.c_size_t()
        assert L.tri_batch_matched_terms(b.h, 0, present.ctypes.data, freq.ctypes.data, None, 0, C.byref(npos)) == -1
        assert b"tri_batch_matched_terms_wide" in L.tri_last_error() and np.all(present == guard) and np.all(freq == 0xBEEF)
        assert L.tri_batch_matched_terms(b.h, 0, None, None, None, 0, C.byref(npos)) == -1  # (the sizing call too)
        # the narrow query beside it: both pairs of calls
        m = int(b.counts()[1])
        narrow = b.matched_terms(1, m)
        wide = b.matched_terms_wide(1, m)
        assert narrow[1].dtype == np.uint32 and np.array_equal(narrow[1], wide[1].astype(np.uint32)) and np.array_equal(narrow[2], wide[2])
    finally:
        b.close()


def test_default_options_still_leave_the_shapes_out(ctxs, T, dev):
    c = ctxs((0, 1))
    assert dev.get_option("rich_max_terms") == 16
    progs = c.progs + [O.parse_query("t0 t1")]
    with options(dev, tree_max_nodes=1024):
        b = T.Batch(c.w.ix, progs, T.FLAG_MATCHED_TERMS, allow_unsupported=True)
    try:
        assert b.query_status().tolist() == [-3] * len(c.progs) + [0] and b.info()["unsupported_queries"] == len(c.progs)
        b.run()
        b.sync()
        counts = b.counts()
        assert not counts[: len(c.progs)].any() and int(counts[-1]) == len(c.w.ora.exec(progs[-1], O.FLAG_DOCUMENTS_ONLY)[0])
    finally:
        b.close()
    with options(dev, **OPTS):  # a 65th term: left out at 64 too (its status only: the oracle does not take it)
        b = T.Batch(c.w.ix, [O.parse_query(OR65), c.progs[0]], T.FLAG_MATCHED_TERMS, allow_unsupported=True)
        assert b.query_status().tolist() == [-3, 0]
        b.close()
    for bad in (15, 65):
        with options(dev, rich_max_terms=bad):
            with pytest.raises(T.TrinityError, match="rich_max_terms"):
                T.Batch(c.w.ix, progs[-1:], T.FLAG_MATCHED_TERMS)


# ------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_second_run_answers_as_the_first(ctxs, case):
    """The high mask halves and the wide rows are cleared per run: a stale bit or cell would show in the second run's present / freq."""
    c = ctxs(case)
    with options(c.dev, **OPTS):
        (first, second), _ = c.run(c.progs, runs=2)
    plain = c.plain()
    for a, b, p, name in zip(first, second, plain, NAMES):
        same(a, b, name)
        same(a, p, name)


# ------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_payloads_run_parallel_to_the_wide_calls_positions(ctxs, case):
    c = ctxs(case)
    T = c.T
    i = NAMES.index("or64")
    with options(c.dev, **OPTS):
        b = T.Batch(c.w.ix, [c.progs[i]], T.FLAG_MATCHED_TERMS | T.FLAG_HIT_PAYLOADS)
    try:
        b.run()
        b.sync()
        n = int(b.counts()[0])
        docs = b.docset(0, n)
        res = (docs,) + b.matched_terms(0, n)
        same(res, c.plain()[i], "or64")
        lens, payloads = b.matched_payloads(0)
        assert len(lens) == len(payloads) == len(res[4]) == SHAPES[i][4 + c.wi][2]  # *n == *npos == the oracle's hits_total
    finally:
        b.close()
