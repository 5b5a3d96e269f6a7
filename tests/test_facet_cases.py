"""The yardstick of the facet counts, checked on the CPU (tests/facet_cases.py): for the queries and facets the GPU tests run, the expected rows (numpy.bincount over
structured.Corpus.evaluate's docID sets, which equal the oracle's) sum to the match counts and can tell a right answer from three wrong ones —
  shift     the column read one docID off: every non-empty query is told by at least one facet of its group whose column varies from one docID to the next (mod7,
            low16, huge).  Not by every one: `window` changes at 2 .. 17 docIDs of a corpus, `one` nowhere, and a set that is uniform modulo 7 — {all} {odd} of the
            main corpus — has the same mod7 row one docID off; low16 tells that one;
  clamp     values clamped to nbuckets - 1 instead of counted as overflow: asserted for every (query, facet) whose nbuckets lies below the column's values on that
            set, and every non-empty query has such a facet in its group;
  unmasked  the rows of the unmasked, unfiltered set: asserted for every query and facet of the mask test and of the filter test.
And csrc/host/facet_rows.hpp — the host counting behind FacetCounter::consider — equals facet_rows on the same cases: a stand-alone program built with
-fsanitize=address,undefined (nothing sanitised is loaded into Python).  No GPU here."""
import os
import subprocess

import numpy as np
import pytest

import facet_cases as F
import oracle_lib as O
import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "facet_cpu_test.cpp")
VARYING = ("mod7", "low16", "huge")


@pytest.fixture(scope="module")
def groups():
    """[(tag, corpus, queries, docID sets, facets)] — the groups of the GPU tests, evaluated once."""
    out = []
    stream = S.stream_corpus()
    queries = S.stream_docs_queries(stream)
    sets = [stream.evaluate(p) for p in S.programs(queries)]
    ora = stream.oracle()
    for (text, mn), p, s in zip(queries, S.programs(queries), sets):
        assert np.array_equal(ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0], s), text
    for tag, facets in (("stream", F.STREAM_FACETS), ("thresholds", F.THRESHOLD_FACETS), ("four_on_chip", F.FOUR_ON_CHIP), ("four_direct", F.FOUR_DIRECT)):
        out.append((tag, stream, [t for t, _ in queries], sets, F.resolve(facets, stream.D)))
    main = S.main_corpus()
    eq = [main.q(t) for t in F.EDGE_QUERIES]
    esets = [main.evaluate(O.parse_query(t)) for t in eq]
    out.append(("edges", main, eq, esets, F.resolve(F.EDGE_FACETS, main.D)))
    out.append(("edges_on_chip", main, eq, esets, F.resolve(F.EDGE_FACETS_ON_CHIP, main.D)))
    tall = S.tall_corpus()
    tq = [tall.q(t) for t in F.TALL_QUERIES]
    out.append(("tall", tall, tq, [tall.evaluate(O.parse_query(t)) for t in tq], F.resolve(F.TALL_FACETS, tall.D)))
    for tag, c, texts, sets in ((g[0], g[1], g[2], g[3]) for g in out if g[0] in ("edges", "tall")):  # ... and the oracle agrees with evaluate on these too
        ora = c.oracle()
        for t, s in zip(texts, sets):
            assert np.array_equal(ora.exec(O.parse_query(t), O.FLAG_DOCUMENTS_ONLY)[0], s), (tag, t)
    return out


def test_which_regime_each_group_of_facets_takes(groups):
    """A group's counters per query (all its facets together) against the LDS budget: the on-chip groups fit it — there a segment's length decides —, the direct ones do not."""
    per_query = {tag: sum(nb + 1 for _, nb in facets) for tag, _, _, _, facets in groups}
    assert per_query["edges_on_chip"] <= F.LDS_COUNTERS < per_query["edges"], per_query
    assert per_query["four_on_chip"] <= F.LDS_COUNTERS < per_query["four_direct"], per_query
    assert per_query["tall"] <= F.LDS_COUNTERS
    assert [nb + 1 - F.LDS_COUNTERS for _, nb in F.THRESHOLD_FACETS[:3]] == [-1, 0, 1]


def test_rows_sum_to_the_match_counts_and_tell_shift_and_clamp(groups):
    told = {"shift": 0, "clamp": 0}
    for tag, c, texts, sets, facets in groups:
        cols = F.columns(c.D)
        shift_q, clamp_q = np.zeros(len(sets), bool), np.zeros(len(sets), bool)
        for name, nb in facets:
            want = F.facet_rows(sets, cols[name], nb)
            assert want.sum(axis=1).tolist() == [len(s) for s in sets], (tag, name, nb)
            off = F.facet_rows(sets, F.shifted(cols[name]), nb)
            clamp = F.clamped_rows(sets, cols[name], nb)
            for i, s in enumerate(sets):
                if not len(s):
                    assert not want[i].any(), (tag, texts[i])
                    continue
                if name in VARYING and not np.array_equal(want[i], off[i]):
                    shift_q[i] = True
                    told["shift"] += 1
                if int(cols[name][s].max()) >= nb:
                    assert want[i, nb] > 0 and not np.array_equal(want[i], clamp[i]), (tag, texts[i], name, nb)
                    clamp_q[i] = True
                    told["clamp"] += 1
        if tag != "tall":  # (the tall group counts `one` and `window` at sizes that fit: cross-workgroup accumulation, no overflow)
            for i, s in enumerate(sets):
                assert not len(s) or (shift_q[i] and clamp_q[i]), (tag, texts[i])
    assert told["shift"] > 300 and told["clamp"] > 200, told


def test_edge_queries_are_the_edges(groups):
    """The edge group holds what it says: an empty set, {1}, {D}, lists one below, at and one above the short-segment threshold, unions that reach the partial last window."""
    tag, c, texts, sets, _ = next(g for g in groups if g[0] == "edges")
    assert [c.df()[c.tid["df%d" % n]] for n in (F.SHORT_SEGMENT - 1, F.SHORT_SEGMENT, F.SHORT_SEGMENT + 1)] == [F.SHORT_SEGMENT - 1, F.SHORT_SEGMENT, F.SHORT_SEGMENT + 1]
    assert F.SHORT_SEGMENT + 1 <= S.TILE_DOCS  # (one candidate tile, one task: the segment is the whole list)
    assert [len(s) for s in sets[:6]] == [0, 1, 1, F.SHORT_SEGMENT - 1, F.SHORT_SEGMENT, F.SHORT_SEGMENT + 1]
    assert sets[1].tolist() == [1] and sets[2].tolist() == [c.D] and c.D % S.SPAN_BITS == 37
    for i in (6, 7, 9):
        assert int(sets[i].max()) == c.D and int((sets[i] > 4 * S.SPAN_BITS).sum()) >= 19, texts[i]
    tall = next(g for g in groups if g[0] == "tall")
    assert max(len(s) for s in tall[3]) > (1 << 20)  # (many tasks a query: a million matches)


def test_masked_and_filtered_rows_differ_from_the_unmasked_ones():
    c = S.stream_corpus()
    queries = S.stream_docs_queries(c)
    progs = S.programs(queries)
    cols = F.columns(c.D)
    full = [c.evaluate(p) for p in progs]
    masked = F.stream_masked(c.D)
    drops = F.stream_filter_drops(c.D)
    for ids, keep in F.stream_filters(c.D):
        assert ids.size and ids.dtype == np.uint32
    for (ids, keep), drop in zip(F.stream_filters(c.D), drops):
        assert np.array_equal(np.setdiff1d(np.arange(1, c.D + 1), ids) if keep else ids, drop)
    msets = [c.evaluate(p, masked=masked) for p in progs]
    fsets = [s[~np.isin(s, drops[i % 3])] for i, s in enumerate(full)]
    for name, nb in F.resolve([("mod7", 7), ("mod7", 5), ("window", None), ("huge", None)], c.D):
        plain = F.facet_rows(full, cols[name], nb)
        for kind, sets in (("mask", msets), ("filters", fsets)):
            rows = F.facet_rows(sets, cols[name], nb)
            assert rows.sum(axis=1).tolist() == [len(s) for s in sets]
            for i, (text, _) in enumerate(queries):
                assert len(sets[i]) and not np.array_equal(rows[i], plain[i]), (kind, text, name, nb)


def test_host_counting_equals_facet_rows_under_sanitizers(groups, tmp_path):
    """csrc/host/facet_rows.hpp over the groups' (query, facet) cases — consider(id) one by one and consider(ids, cnt) in uneven runs — plus its own edges."""
    lines, ncases = [], 0
    cols_out, col_of = [], {}
    for tag, c, texts, sets, facets in groups:
        if tag in ("tall", "four_on_chip", "four_direct", "edges_on_chip"):
            continue  # (tall: a million documents a query — the same code path as the rest; the two fours: facets the other groups hold)
        cols = F.columns(c.D)
        for name, nb in facets:
            if (tag, name) not in col_of and (c.D, name) not in col_of:
                col_of[c.D, name] = len(cols_out)
                cols_out.append(cols[name])
            k = col_of[c.D, name]
            want = F.facet_rows(sets, cols[name], nb)
            for i in range(0, len(sets), 1 if tag == "edges" else 5):
                if tag == "edges" and len(sets[i]) > 10000:
                    continue
                lines.append(" ".join(map(str, [k, nb, len(sets[i])] + sets[i].tolist() + want[i].tolist())))
                ncases += 1
    vec = tmp_path / "facet_vectors.txt"
    with open(vec, "w") as f:
        f.write("%d\n" % len(cols_out))
        for v in cols_out:
            f.write("%d %s\n" % (v.size, " ".join(map(str, v.tolist()))))
        f.write("%d\n" % ncases)
        f.write("\n".join(lines) + "\n")
    binary = str(tmp_path / "facet_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary, str(vec)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    assert res.stdout.split()[:4] == ["cases", str(ncases), "bad", "0"] and ncases > 100, res.stdout
