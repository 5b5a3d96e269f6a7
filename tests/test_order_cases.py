"""The yardstick of ordering by a column, checked on the CPU (tests/order_cases.py): for the very queries and columns the GPU tests run, the expected rows
(numpy.lexsort over structured.Corpus.evaluate's docID sets, which equal the oracle's) can tell a right answer from five wrong ones — in every test group at least one
(query, column, direction) differs from
  shift       the column read one docID off.  NOT told by `one` (every document the same value);
  high ties   descending taken as the ascending sort reversed, ties to the HIGHER docID.  NOT told by `rev` or `hash` (no two documents of a set share a value);
  signed      values compared as signed 32-bit (`huge`'s 0xffffffff as -1).  Told only by `huge`; NOT by `one`, `mod7`, `rev` (all below 2^31);
  unmasked    the rows of the unmasked, unfiltered set: asserted for every query of the mask test and of the filter test;
  no merge    the first task's list taken as the query's: asserted on the tall group, whose sets span many tasks.
It asserts which side of each of k_order's sizes (dev_structs.hpp, read through structured.header_constants) every edge case lies on.  And csrc/host/order_rows.hpp —
the host selection behind ColumnOrder::consider — equals first_k / blend on the same cases: a stand-alone program built with -fsanitize=address,undefined (nothing
sanitised is loaded into Python).  No GPU here."""
import os
import subprocess

import numpy as np
import pytest

import facet_cases as F
import oracle_lib as O
import order_cases as OC
import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "order_cpu_test.cpp")
NO_SHIFT = ("one",)
NO_TIES = ("rev", "hash")
NO_SIGN = ("one", "mod7", "rev", "window", "low16")


@pytest.fixture(scope="module")
def groups():
    """[(tag, corpus, query texts, docID sets, columns, ks)] — the groups of the GPU tests, evaluated once."""
    out = []
    stream = S.stream_corpus()
    queries = S.stream_docs_queries(stream)
    sets = [stream.evaluate(p) for p in S.programs(queries)]
    ora = stream.oracle()
    for (text, mn), p, s in zip(queries, S.programs(queries), sets):
        assert np.array_equal(ora.exec(p, O.FLAG_DOCUMENTS_ONLY)[0], s), text
    out.append(("stream", stream, [t for t, _ in queries], sets, OC.STREAM_COLUMNS, [OC.STREAM_K]))
    out.append(("worst", stream, [t for t, _ in queries], sets, OC.WORST_COLUMNS, [256, 10]))
    main = S.main_corpus()
    eq = [main.q(t) for t in OC.EDGE_QUERIES]
    out.append(("edges", main, eq, [main.evaluate(O.parse_query(t)) for t in eq], ["hash", "mod7"], OC.EDGE_KS))
    sizes = OC.sizes_corpus()
    sq = [sizes.q("{n%d}" % n) for n in OC.SIZE_EDGES]
    out.append(("sizes", sizes, sq, [sizes.evaluate(O.parse_query(t)) for t in sq], ["hash", "rev", "one"], [256, 255, 10]))
    tall = S.tall_corpus()
    tq = [tall.q(t) for t in OC.TALL_QUERIES]
    out.append(("tall", tall, tq, [tall.evaluate(O.parse_query(t)) for t in tq], OC.TALL_COLUMNS, [256]))
    for tag, c, texts, sets in ((g[0], g[1], g[2], g[3]) for g in out if g[0] in ("edges", "sizes", "tall")):  # ... and the oracle agrees with evaluate on these too
        ora = c.oracle()
        for t, s in zip(texts, sets):
            assert np.array_equal(ora.exec(O.parse_query(t), O.FLAG_DOCUMENTS_ONLY)[0], s), (tag, t)
    return out


def differ(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_rows_tell_shift_high_ties_and_signed_compares(groups):
    for tag, c, texts, sets, names, ks in groups:
        cols = OC.columns(c.D)
        told = {"shift": 0, "ties": 0, "signed": 0}
        for name in names:
            for k in ks:
                for i, s in enumerate(sets):
                    up, down = OC.first_k(s, cols[name], k), OC.first_k(s, cols[name], k, True)
                    assert len(up[0]) == len(down[0]) == min(k, len(s)) and set(up[0].tolist()) <= set(s.tolist())
                    if not len(s):
                        continue
                    for desc, want in ((False, up), (True, down)):
                        shift = differ(want, OC.first_k(s, OC.shifted(cols[name]), k, desc))
                        signed = differ(want, OC.signed_first_k(s, cols[name], k, desc))
                        assert not (shift and name in NO_SHIFT) and not (signed and name in NO_SIGN), (tag, name, texts[i])
                        told["shift"] += shift
                        told["signed"] += signed
                    ties = differ(down, OC.ties_to_the_higher_docid(s, cols[name], k))
                    assert not (ties and name in NO_TIES), (tag, name, texts[i])
                    told["ties"] += ties
        # every group holds a column that varies from docID to docID, one with ties (mod7, one, huge) and one with values on both sides of 2^31 (hash, huge)
        assert set(names) - set(NO_SHIFT) and set(names) - set(NO_TIES) and set(names) - set(NO_SIGN), tag
        assert told["shift"] > 0 and told["ties"] > 0 and told["signed"] > 0, (tag, told)


def test_edge_queries_lie_on_the_sides_of_the_kernels_sizes_they_claim(groups):
    assert (OC.TILE, OC.WAVE_PASS, OC.PRUNE_AT, OC.BUF, OC.MAX_TOPK, OC.WG_PASS, OC.FANIN) == (64, 256, 448, 512, 256, 1024, 32)
    assert OC.PRUNE_AT + OC.TILE == OC.BUF and OC.PRUNE_AT >= OC.MAX_TOPK  # (a buffer at the mark has room for one step's newcomers; a pruned one is below it)
    for n in (OC.TILE, OC.WAVE_PASS, OC.PRUNE_AT, OC.BUF, OC.MAX_TOPK, OC.WG_PASS, 2 * OC.WG_PASS):
        assert {n - 1, n, n + 1} <= set(OC.SIZE_EDGES)
    tag, c, texts, sets, _, ks = next(g for g in groups if g[0] == "sizes")
    assert [len(s) for s in sets] == OC.SIZE_EDGES and max(OC.SIZE_EDGES) <= S.TILE_DOCS  # (one candidate tile, one task: the segment is the whole list)
    assert 256 in ks and 255 in ks  # (every key of a `rev` ascending segment beats the threshold: wave 0 prunes once it holds more than ORDER_PRUNE_AT of them)
    tag, c, texts, sets, _, ks = next(g for g in groups if g[0] == "edges")
    assert [len(s) for s in sets[:9]] == [0, 1, 1, 31, 32, 33, 127, 128, 129] and {1, 32, 128, 256} == set(ks)  # K - 1, K, K + 1 for K = 32 and 128
    assert sets[1].tolist() == [1] and sets[2].tolist() == [c.D] and c.D % S.SPAN_BITS == 37 and sets[13].tolist() == [1, c.D]
    for i in (9, 10, 12):
        assert int(sets[i].max()) == c.D and int((sets[i] > 4 * S.SPAN_BITS).sum()) >= 19, texts[i]  # (bitmaps with the partial last window)
    tag, c, texts, sets, names, _ = next(g for g in groups if g[0] == "tall")
    assert max(len(s) for s in sets) > (1 << 20) and max(len(s) for s in sets) > OC.FANIN * S.TILE_DOCS  # (more single-tile tasks than one merge group folds)
    cols = OC.columns(c.D)
    told = 0
    for name in names:
        for desc in (False, True):
            for s in sets:
                told += differ(OC.first_k(s, cols[name], 256, desc), OC.first_task_only(s, cols[name], 256, desc))
    assert told > 0  # (`rev` ascending and `hash`: the best documents do not lie in the first task)
    assert not differ(OC.first_k(sets[0], cols["one"], 256), OC.first_task_only(sets[0], cols["one"], 256))  # (`one` cannot tell: the lowest docIDs come first)


def test_masked_and_filtered_rows_differ_from_the_unmasked_ones():
    c = S.stream_corpus()
    queries = S.stream_docs_queries(c)
    progs = S.programs(queries)
    cols = OC.columns(c.D)
    full = [c.evaluate(p) for p in progs]
    masked = F.stream_masked(c.D)
    drops = F.stream_filter_drops(c.D)
    msets = [c.evaluate(p, masked=masked) for p in progs]
    fsets = [s[~np.isin(s, drops[i % 3])] for i, s in enumerate(full)]
    for kind, sets in (("mask", msets), ("filters", fsets)):
        for i, (text, _) in enumerate(queries):
            assert len(sets[i]) < len(full[i])
            # `rev` ascending lists the HIGHEST docIDs, D among them — a masked window edge; both directions of `rev` and `hash` together tell every query
            assert any(differ(OC.first_k(sets[i], cols[n], 10, d), OC.first_k(full[i], cols[n], 10, d)) for n in ("rev", "hash") for d in (False, True)), (kind, text)


def test_blend_is_the_stable_sort_of_the_concatenation():
    vals = [np.array([0, 5, 5, 9, 1], np.uint32), np.array([0, 5, 7, 9], np.uint32)]
    parts = [OC.first_k(np.array([1, 2, 3, 4]), vals[0], 3), OC.first_k(np.array([1, 2, 3]), vals[1], 3)]
    d, v = OC.blend(parts, 4)
    assert d.tolist() == [4, 1, 1, 2] and v.tolist() == [1, 5, 5, 5]  # (docID 1 at value 5 in both sources: listed twice, the older source's first)
    parts = [OC.first_k(np.array([1, 2, 3, 4]), vals[0], 3, True), OC.first_k(np.array([1, 2, 3]), vals[1], 3, True)]
    d, v = OC.blend(parts, 4, True)
    assert d.tolist() == [3, 3, 2, 1] and v.tolist() == [9, 9, 7, 5]


def test_host_selection_equals_first_k_under_sanitizers(groups, tmp_path):
    """csrc/host/order_rows.hpp over the groups' (query, column, K, direction) cases — consider(id) one by one and consider(ids, cnt) in uneven runs — and over blends of
    three parts, plus its own edges."""
    lines, blends = [], []
    cols_out, col_of = [], {}

    def col_index(D, name):
        if (D, name) not in col_of:
            col_of[D, name] = len(cols_out)
            cols_out.append(OC.columns(D)[name])
        return col_of[D, name]

    for tag, c, texts, sets, names, ks in groups:
        if tag == "tall":
            continue  # (a million documents a query — the same code path as the rest)
        for name in names:
            ci = col_index(c.D, name)
            for k in ks:
                for desc in (False, True):
                    for i in range(0, len(sets), 1 if tag in ("edges", "sizes") else 7):
                        if len(sets[i]) > 10000:
                            continue
                        d, v = OC.first_k(sets[i], OC.columns(c.D)[name], k, desc)
                        lines.append(" ".join(map(str, [ci, k, int(desc), len(sets[i])] + sets[i].tolist() + [len(d)] + d.tolist() + v.tolist())))
    tag, c, texts, sets, names, ks = next(g for g in groups if g[0] == "sizes")
    for name in ("mod7", "hash"):
        ci, vals = col_index(c.D, name), OC.columns(c.D)[name]
        for k in (1, 10, 256):
            for desc in (False, True):
                three = [sets[0], sets[3], sets[0][::2]]  # (the first and the third share documents: equal keys of two parts)
                d, v = OC.blend([OC.first_k(s, vals, k, desc) for s in three], k, desc)
                blends.append(" ".join(map(str, [k, int(desc), 3] + sum(([ci, len(s)] + s.tolist() for s in three), []) + [len(d)] + d.tolist() + v.tolist())))
    vec = tmp_path / "order_vectors.txt"
    with open(vec, "w") as f:
        f.write("%d\n" % len(cols_out))
        for v in cols_out:
            f.write("%d %s\n" % (v.size, " ".join(map(str, v.tolist()))))
        f.write("%d\n%s\n%d\n%s\n" % (len(lines), "\n".join(lines), len(blends), "\n".join(blends)))
    binary = str(tmp_path / "order_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary, str(vec)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    assert res.stdout.split() == ["cases", str(len(lines)), "blends", str(len(blends)), "bad", "0"] and len(lines) > 100, res.stdout
