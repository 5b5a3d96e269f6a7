"""The yardstick of the stats of a column, checked on the CPU (tests/stats_cases.py): for the queries and stats the GPU tests run, the expected rows (numpy over
structured.Corpus.evaluate's docID sets, which equal the oracle's) can tell a right answer from seven wrong ones, group of stats by group —
  shift     the VALUE column read one docID off: every non-empty query is told by a stat of its group whose value column varies from one docID to the next (hash,
            rev, huge, low16, mod7).  `one` as a value tells nothing; a set that is uniform modulo 7 has the same mod7 sums one docID off, and hash or rev tell it;
  swap      group and value columns swapped: every non-empty query, by a grouped stat of its group.  An ungrouped stat has no group to swap: the group of the four
            columns as values (AS_VALUES) cannot tell this one, the four columns as groups (AS_GROUPS) do;
  sum32     a sum kept in 32 bits: every group holds a record whose sum reaches 2^32 (two documents of hash or huge do).  Single-document queries, and the
            values one, mod7, low16 and rev (small numbers) on short lists, tell nothing;
  min0      a mins plane initialised to zero: every non-empty query, by a stat whose value is not zero on the set — never by `one`, whose min IS zero;
  clamp     the overflow bucket clamped into the last real one: every grouped stat whose nbuckets lies below the group's values on the set.  The tall group
            (`one` at 1 and mod7 at 7 buckets: both fit) cannot tell it, nor can a group of ungrouped stats;
  unmasked  the rows of the unmasked, unfiltered set: every query of the mask test and of the filter test;
  task0     a query's first task taken for the whole query: every tall query of more than one candidate tile.
It asserts which regime of k_stats every group and every edge segment takes, from the header's constants; that the counts of every grouped case equal
facet_cases.facet_rows; and that csrc/host/stats_rows.hpp — the host aggregation behind StatsCounter::consider and tri_cbatch_stats' combine — equals stats_rows on the
same cases and refuses a sum that wraps 64 bits: a stand-alone program built with -fsanitize=address,undefined (nothing sanitised is loaded into Python).  No GPU here."""
import os
import subprocess

import numpy as np
import pytest

import facet_cases as F
import oracle_lib as O
import order_cases as OC
import stats_cases as X
import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stats_cpu_test.cpp")
VARYING = ("hash", "rev", "huge", "low16", "mod7")


@pytest.fixture(scope="module")
def groups():
    """[(tag, corpus, query texts, docID sets, stats)] — the groups of the GPU tests, evaluated once."""
    out = []
    stream = S.stream_corpus()
    queries = S.stream_docs_queries(stream)
    sets = [stream.evaluate(p) for p in S.programs(queries)]
    ora = stream.oracle()
    for (text, mn), p, s in zip(queries, S.programs(queries), sets):
        assert np.array_equal(ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0], s), text
    for tag, stats in (("stream", X.STREAM_STATS), ("thresholds", X.THRESHOLD_STATS), ("four_on_chip", X.FOUR_ON_CHIP), ("four_direct", X.FOUR_DIRECT), ("mixed_on_chip", X.MIXED_ON_CHIP),
                       ("mixed_direct", X.MIXED_DIRECT), ("as_groups", X.AS_GROUPS), ("as_values", X.AS_VALUES), ("mask", X.MASK_STATS)):  # fmt: skip
        out.append((tag, stream, [t for t, _ in queries], sets, X.resolve(stats, stream.D)))
    main = S.main_corpus()
    eq = [main.q(t) for t in X.EDGE_QUERIES]
    esets = [main.evaluate(O.parse_query(t)) for t in eq]
    out.append(("edges_direct", main, eq, esets, X.resolve(X.EDGE_STATS_DIRECT, main.D)))
    out.append(("edges_on_chip", main, eq, esets, X.resolve(X.EDGE_STATS_ON_CHIP, main.D)))
    sizes = OC.sizes_corpus()
    sq = [sizes.q("{n%d}" % n) for n in X.SIZE_QUERIES]
    out.append(("sizes", sizes, sq, [sizes.evaluate(O.parse_query(t)) for t in sq], X.resolve(X.SIZE_STATS, sizes.D)))
    tall = S.tall_corpus()
    tq = [tall.q(t) for t in X.TALL_QUERIES]
    out.append(("tall", tall, tq, [tall.evaluate(O.parse_query(t)) for t in tq], X.resolve(X.TALL_STATS, tall.D)))
    return out


def rows_of(cols, sets, stat):
    g, nb, v = stat
    return X.stats_rows(sets, None if g is None else cols[g], nb, cols[v])


def test_which_regime_each_group_of_stats_and_each_edge_segment_takes(groups):
    """A group's records per query (its GROUPED stats together) against STATS_LDS_BUCKETS: the on-chip groups fit it — there a segment's length decides —, the direct
    ones do not; an ungrouped stat is folded in registers whatever stands beside it."""
    rec = {tag: X.lds_records(stats) for tag, _, _, _, stats in groups}
    assert (X.LDS_BUCKETS + X.STATS_MAX) * 20 <= 16384 and X.SHORT_SEGMENT in (32, 128)
    assert [X.lds_records([s]) - X.LDS_BUCKETS for s in X.THRESHOLD_STATS[:3]] == [-1, 0, 1]
    assert [X.regime([s], 10**6) for s in X.THRESHOLD_STATS] == [["on chip"], ["on chip"], ["direct"], ["direct"]]
    assert rec["four_on_chip"] <= X.LDS_BUCKETS < rec["four_direct"] and rec["edges_on_chip"] <= X.LDS_BUCKETS < rec["edges_direct"]
    assert rec["mixed_on_chip"] <= X.LDS_BUCKETS < rec["mixed_direct"] and rec["as_values"] == 0 and rec["stream"] <= X.LDS_BUCKETS and rec["tall"] <= X.LDS_BUCKETS
    stats = dict((tag, s) for tag, _, _, _, s in groups)
    assert X.regime(stats["mixed_on_chip"], 10**6) == ["registers", "on chip", "registers"] and X.regime(stats["mixed_direct"], 10**6) == ["registers", "direct", "registers"]
    assert X.regime(stats["as_values"], 1) == ["registers"] * 4 and X.regime(stats["four_on_chip"], 10**6) == ["on chip"] * 4 and X.regime(stats["four_direct"], 10**6) == ["direct"] * 4
    assert X.regime(stats["tall"], S.TILE_DOCS) == ["registers", "on chip", "on chip"]
    # the edges: a segment one below the threshold goes direct, at it and one above on chip — when the rows fit; with the wide row every segment goes direct
    for n, want in ((1, "direct"), (X.SHORT_SEGMENT - 1, "direct"), (X.SHORT_SEGMENT, "on chip"), (X.SHORT_SEGMENT + 1, "on chip")):
        assert X.regime(stats["edges_on_chip"], n) == ["registers"] + [want] * 3, n
        assert X.regime(stats["edges_direct"], n) == ["registers"] + ["direct"] * 3, n
    assert all(X.regime(stats["sizes"], n) == ["registers", "registers", "on chip" if n >= X.SHORT_SEGMENT else "direct"] for n in X.SIZE_QUERIES)
    assert min(X.SIZE_QUERIES) < X.SHORT_SEGMENT <= max(X.SIZE_QUERIES)


def test_the_rows_tell_shift_swap_sum32_min0_and_clamp(groups):
    told = dict.fromkeys(("shift", "swap", "sum32", "min0", "clamp"), 0)
    for tag, c, texts, sets, stats in groups:
        cols = X.columns(c.D)
        nq = len(sets)
        by = {k: np.zeros(nq, bool) for k in told}
        for g, nb, v in stats:
            want = rows_of(cols, sets, (g, nb, v))
            assert want.counts.sum(axis=1).tolist() == [len(s) for s in sets], (tag, g, nb, v)
            empty = want.counts == 0
            assert not want.sums[empty].any() and (want.mins[empty] == X.HUGE).all() and not want.maxs[empty].any()
            if g is not None:  # the counts plane is the facet row of the group column
                assert np.array_equal(want.counts, F.facet_rows(sets, cols[g], nb)), (tag, g, nb)
            off = X.stats_rows(sets, None if g is None else cols[g], nb, X.shifted(cols[v]))
            swap = X.swapped(sets, cols[g], nb, cols[v]) if g is not None and g != v else None
            clamp = X.clamped(sets, cols[g], nb, cols[v]) if g is not None else None
            for i, s in enumerate(sets):
                if not len(s):
                    continue
                one = X.Stats(*(p[i : i + 1] for p in want))
                if v in VARYING and not X.same(one, X.Stats(*(p[i : i + 1] for p in off))):
                    by["shift"][i] = True
                if swap is not None:
                    assert not X.same(one, X.Stats(*(p[i : i + 1] for p in swap))), (tag, texts[i], g, v)
                    by["swap"][i] = True
                if int(want.sums[i].max()) >= 1 << 32:
                    assert not X.same(one, X.sums32(one))
                    by["sum32"][i] = True
                if (want.mins[i][want.counts[i] > 0] != 0).any():
                    assert not X.same(one, X.mins_zeroed(one))
                    by["min0"][i] = True
                if g is not None and int(cols[g][s].max()) >= nb:
                    assert want.counts[i, nb] > 0 and not X.same(one, X.Stats(*(p[i : i + 1] for p in clamp))), (tag, texts[i], g, nb)
                    by["clamp"][i] = True
        full = np.array([len(s) > 0 for s in sets])
        many = np.array([len(s) > 1 for s in sets])
        assert (by["shift"] | ~full).all() and (by["min0"] | ~full).all(), (tag, by)
        assert by["sum32"].any() and (by["sum32"] | ~many).all() or tag in ("sizes",) and by["sum32"].all(), (tag, by["sum32"])
        if X.lds_records(stats):
            assert (by["swap"] | ~full).all(), (tag, by["swap"])
        else:
            assert tag == "as_values" and not by["swap"].any()
        if tag == "tall" or not X.lds_records(stats):
            assert not by["clamp"].any(), tag  # (named above: nothing overflows here)
        else:
            assert (by["clamp"] | ~full).all(), (tag, by["clamp"])
        for k in told:
            told[k] += int(by[k].sum())
    assert all(n > 100 for n in told.values()), told


def test_edge_and_size_queries_are_what_they_say(groups):
    tag, c, texts, sets, _ = next(g for g in groups if g[0] == "edges_direct")
    assert [len(s) for s in sets[:6]] == [0, 1, 1, X.SHORT_SEGMENT - 1, X.SHORT_SEGMENT, X.SHORT_SEGMENT + 1] and X.SHORT_SEGMENT + 1 <= S.TILE_DOCS
    assert sets[1].tolist() == [1] and sets[2].tolist() == [c.D] and c.D % S.SPAN_BITS == 37
    for i in (6, 7, 9):
        assert int(sets[i].max()) == c.D and int((sets[i] > 4 * S.SPAN_BITS).sum()) >= 19, texts[i]
    sizes = next(g for g in groups if g[0] == "sizes")
    assert [len(s) for s in sizes[3]] == X.SIZE_QUERIES == [63, 64, 65, 255, 256, 257] and max(X.SIZE_QUERIES) <= S.TILE_DOCS


def test_a_first_task_left_unmerged_is_told(groups):
    tag, c, texts, sets, stats = next(g for g in groups if g[0] == "tall")
    cols = X.columns(c.D)
    assert max(len(s) for s in sets) > (1 << 20)  # (many tasks a query: a million matches)
    for g, nb, v in stats:
        want = rows_of(cols, sets, (g, nb, v))
        first = X.first_task_only(sets, None if g is None else cols[g], nb, cols[v])
        for i, s in enumerate(sets):
            if len(s) > S.TILE_DOCS:
                assert not np.array_equal(want.counts[i], first.counts[i]) and not np.array_equal(want.sums[i], first.sums[i]), (texts[i], g, v)
    assert sum(len(s) > S.TILE_DOCS for s in sets) >= 3


def test_masked_and_filtered_rows_differ_from_the_unmasked_ones():
    c = S.stream_corpus()
    queries = S.stream_docs_queries(c)
    progs = S.programs(queries)
    cols = X.columns(c.D)
    full = [c.evaluate(p) for p in progs]
    masked = X.stream_masked(c.D)
    drops = X.stream_filter_drops(c.D)
    msets = [c.evaluate(p, masked=masked) for p in progs]
    fsets = [s[~np.isin(s, drops[i % 3])] for i, s in enumerate(full)]
    for stat in X.resolve(X.MASK_STATS, c.D):
        plain = rows_of(cols, full, stat)
        for kind, sets in (("mask", msets), ("filters", fsets)):
            rows = rows_of(cols, sets, stat)
            for i, (text, _) in enumerate(queries):
                assert len(sets[i]) and not np.array_equal(rows.counts[i], plain.counts[i]) and not np.array_equal(rows.sums[i], plain.sums[i]), (kind, text, stat)


def test_combine_adds_and_folds_and_refuses_a_wrap():
    a = X.Stats(np.array([[3, 1 << 63]], np.uint64), np.array([[1, 2]], np.uint32), np.array([[3, 1]], np.uint32), np.array([[3, 9]], np.uint32))
    b = X.Stats(np.array([[4, (1 << 63) - 1]], np.uint64), np.array([[0xFFFFFFFF, 2]], np.uint32), np.array([[1, 7]], np.uint32), np.array([[2, 11]], np.uint32))
    got = X.combine([a, b])
    assert got.sums.tolist() == [[7, (1 << 64) - 1]] and got.counts.tolist() == [[1 << 32, 4]] and got.mins.tolist() == [[1, 1]] and got.maxs.tolist() == [[3, 11]]
    assert got.counts.dtype == np.uint64
    with pytest.raises(OverflowError, match="query 0, bucket 1"):
        X.combine([a, b, X.Stats(np.array([[0, 1]], np.uint64), a.counts, a.mins, a.maxs)])


def test_host_aggregation_equals_stats_rows_under_sanitizers(groups, tmp_path):
    """csrc/host/stats_rows.hpp over the groups' (query, stat) cases — consider(id) one by one, consider(ids, cnt) in uneven runs, two halves combined by add() — plus its
    own edges, among them two parts whose sums wrap 64 bits."""
    lines, ncases = [], 0
    cols_out, col_of = [], {}

    def col(D, cols, name):
        if (D, name) not in col_of:
            col_of[D, name] = len(cols_out)
            cols_out.append(cols[name])
        return col_of[D, name]

    for tag, c, texts, sets, stats in groups:
        if tag in ("tall", "four_direct", "mixed_direct", "edges_on_chip", "mask"):
            continue  # (tall: a million documents a query — the same code path as the rest; the others: stats the remaining groups hold)
        cols = X.columns(c.D)
        for g, nb, v in stats:
            if nb > 2000:
                continue  # (the widest rows: the same code, much text)
            want = rows_of(cols, sets, (g, nb, v))
            for i in range(0, len(sets), 1 if tag.startswith("edges") or tag == "sizes" else 7):
                if len(sets[i]) > 10000:
                    continue
                row = [-1 if g is None else col(c.D, cols, g), col(c.D, cols, v), nb, len(sets[i])] + sets[i].tolist()
                lines.append(" ".join(map(str, row + want.sums[i].tolist() + want.counts[i].tolist() + want.mins[i].tolist() + want.maxs[i].tolist())))
                ncases += 1
    vec = tmp_path / "stats_vectors.txt"
    with open(vec, "w") as f:
        f.write("%d\n" % len(cols_out))
        for v in cols_out:
            f.write("%d %s\n" % (v.size, " ".join(map(str, v.tolist()))))
        f.write("%d\n" % ncases)
        f.write("\n".join(lines) + "\n")
    binary = str(tmp_path / "stats_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary, str(vec)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    assert res.stdout.split()[:4] == ["cases", str(ncases), "bad", "0"] and ncases > 100, res.stdout
