"""The yardstick of Trinity::intersect on the device, checked on the CPU (tests/isect_cases.py): the restatement of intersect.cpp:64-99 against the order-free H + C
derivation the engine takes, on the module's cases and on seeded random run-structured sequences; the numpy walk against the iterator-by-iterator merge of
:107-158; every case tells the right answer from three wrong ones and keeps the antichain at or below 255; csrc/host/isect_rows.hpp's replay, as a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer, over the vectors the module dumps."""
import os
import re
import subprocess

import numpy as np
import pytest

import isect_cases as IC
import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "isect_rows_cpu_test.cpp")


@pytest.fixture(scope="module")
def cases():
    cs = IC.cases()
    return cs, IC.masked_of(cs)


@pytest.fixture(scope="module")
def tall():
    return IC.tall_cases()


def test_geometry_mirrors():
    k = S.header_constants("dev_structs.hpp", "k_isect.hpp")
    assert (k["ISECT_SPAN"], k["ISECT_LDS_SLOTS"], k["PL_W"]) == (IC.SPAN, IC.LDS_SLOTS, IC.PL_W)
    assert IC.D // IC.PL_W == 3  # about three plane windows


def test_restatement_equals_the_derivation_on_the_cases(cases):
    cs, masked = cases
    for c in cs:
        g = c.posting_groups()
        want, H, largest = IC.restate(g, c.stop, masked)
        docs, masks, ok, _ = IC.walk(g, c.stop, masked)
        got = IC.derive(docs[ok].tolist(), masks[ok].tolist())
        assert got == want, c.name
        assert largest <= 255, c.name
        assert {m: v for m, v in IC.tables(docs[ok].tolist(), masks[ok].tolist())[0].items()} == H, c.name


def test_the_tall_cases(tall):
    for c in tall:
        g = c.posting_groups()
        want, _, largest = IC.restate(g, c.stop, (), top=c.top)
        docs, masks, ok, _ = IC.walk(g, c.stop, (), top=c.top)
        assert IC.derive(docs[ok].tolist(), masks[ok].tolist()) == want and largest <= 255, c.name
        assert IC.merge_literal(g) == list(zip(docs.tolist(), masks.tolist())), c.name
        for name, w in IC.wrong_answers(g, c.stop, (), top=c.top).items():
            assert w != want, (c.name, name)


def test_the_dense_cases_need_more_runs_than_their_groups_tell():
    for c in IC.dense_cases():
        g = c.posting_groups()
        want, H, largest = IC.restate(g, 0, c.masked)
        docs, masks, ok, _ = IC.walk(g, 0, c.masked)
        Ht, C = IC.tables(docs[ok].tolist(), masks[ok].tolist())
        assert IC.replay(Ht, C) == want and largest <= 255, c.name
        assert len(C) > 4 * 2 ** len(g), (c.name, len(C))
        for name, w in IC.wrong_answers(g, 0, c.masked).items():
            assert w != want, (c.name, name)


def test_the_walk_equals_the_literal_merge(cases):
    cs, _ = cases
    for c in cs:
        g = c.posting_groups()
        docs, masks, _, _ = IC.walk(g)
        assert IC.merge_literal(g) == list(zip(docs.tolist(), masks.tolist())), c.name


def test_every_case_tells_the_right_answer_from_three_wrong_ones(cases):
    cs, masked = cases
    for c in cs:
        want, _, _ = IC.restate(c.posting_groups(), c.stop, masked)
        if c.name == "unknown_all":
            assert want == []
            continue
        wrong = IC.wrong_answers(c.posting_groups(), c.stop, masked)
        assert set(wrong) == {"maximal_true_counts", "no_run_credit", "previous_document"}
        for name, w in wrong.items():
            assert w != want, (c.name, name)


def test_the_cases_are_what_their_names_say(cases):
    cs, masked = cases
    by = {c.name: c for c in cs}
    assert [c.name for c in cs] == ["step", "span", "empty_spans", "ends", "masked", "stop", "epochs", "mid_span", "spill", "wide", "synonyms", "one_window", "unknown_all"]

    def seq(c):
        docs, masks, ok, orig = IC.walk(c.posting_groups(), c.stop, masked)
        return docs, masks, ok, orig

    def runs(c, m):  # [(first, last)] of the runs of mask m among the considered documents
        docs, masks, ok, _ = seq(c)
        d, s = docs[ok].tolist(), masks[ok].tolist()
        out, i = [], 0
        while i < len(s):
            j = i
            while j + 1 < len(s) and s[j + 1] == s[i]:
                j += 1
            if s[i] == m and j > i:
                out.append((d[i], d[j]))
            i = j + 1
        return out

    assert any(a // 64 != b // 64 and a // IC.SPAN == b // IC.SPAN for a, b in runs(by["step"], 1))
    assert any(b // IC.SPAN == a // IC.SPAN + 1 for a, b in runs(by["span"], 1))
    a, b = runs(by["empty_spans"], 1)[0]
    docs = seq(by["empty_spans"])[0]
    spans = set((docs // IC.SPAN).tolist())
    assert b // IC.SPAN - a // IC.SPAN >= 4 and {a // IC.SPAN + 1, a // IC.SPAN + 2, a // IC.SPAN + 3}.isdisjoint(spans)
    tall = {c.name: c for c in IC.tall_cases()}
    docs, masks, ok, _ = IC.walk(tall["lookback"].posting_groups(), top=IC.D_TALL)
    gaps = np.diff(docs[ok] // IC.SPAN)
    assert gaps.max() > 64 and masks[ok][int(gaps.argmax())] == masks[ok][int(gaps.argmax()) + 1] == 1  # more than one 64-span look-back, inside a run
    docs, masks, ok, _ = IC.walk(tall["lookback64"].posting_groups(), top=IC.D_TALL)
    assert 64 in np.diff(docs[ok] // IC.SPAN).tolist() and int(docs[-1]) == IC.D_TALL
    r = runs(by["ends"], 1)
    assert r[0][0] == 1 and r[-1][1] == IC.D
    docs, masks, ok, orig = seq(by["masked"])
    a, b = runs(by["masked"], 1)[0]
    inside = (docs > a) & (docs < b) & ~ok
    assert set(docs[inside].tolist()) & set(by["masked"].masked) and (masks[inside] == orig).any()
    docs, masks, ok, orig = seq(by["stop"])
    a, b = runs(by["stop"], 1)[0]
    inside = (docs > a) & (docs < b) & ~ok
    assert inside.any() and (masks[inside] != orig).all() and not set(docs[inside].tolist()) & set(masked)
    # epochs: the three runs of {a} are credited to three different entries, two of which do not survive
    want, H, _ = IC.restate(by["epochs"].posting_groups(), 0, masked)
    assert dict(want) == {0b1011: H[0b1011][0] + 3, 0b1101: H[0b1101][0]} and len(runs(by["epochs"], 1)) == 3  # (the last run's four documents: three credits; the two earlier runs' went to entries since deleted)
    docs, masks, ok, _ = seq(by["mid_span"])
    first_super = int(docs[ok][masks[ok] == 3][0])
    assert first_super % IC.SPAN not in (0, IC.SPAN - 1) and any(a < first_super < b2 for a in [runs(by["mid_span"], 1)[0][0]] for b2 in [runs(by["mid_span"], 1)[-1][1]])
    docs, masks, ok, _ = seq(by["spill"])
    assert len(set((docs[ok] // IC.SPAN).tolist())) == 1 and len(set(masks[ok].tolist())) > IC.LDS_SLOTS
    docs, masks, ok, orig = seq(by["wide"])
    assert orig == IC.M64 and all(m >> 63 for m in masks[ok].tolist())
    docs, masks, ok, orig = seq(by["synonyms"])
    assert orig == 0 and 3 in masks[ok].tolist()
    c = by["one_window"]
    for t in ("b", "c"):
        d = c.lists[f"one_window.{t}"]
        assert (d // IC.PL_W == 1).all()
    assert IC.orig_mask(by["unknown_all"].posting_groups()) == (0, False)


def test_restatement_equals_the_derivation_on_random_sequences():
    differs = 0
    for docs, seq in IC.random_sequences(3000, 20241019):
        want, largest = IC.run_sequence(seq)
        assert IC.derive(docs, seq) == want
        assert largest <= 255
        differs += want != IC.run_sequence(seq, shortcut=False)[0]
    assert differs > 300  # the quirk is exercised: the shortcut changes the answer on a good share of them


def test_the_replay_header_under_sanitizers(tmp_path, cases):
    cs, masked = cases
    items = IC.random_sequences(1500, 7)
    for c in cs:
        docs, masks, ok, _ = IC.walk(c.posting_groups(), c.stop, masked)
        items.append((docs[ok].tolist(), masks[ok].tolist()))
    vec = str(tmp_path / "vectors.txt")
    IC.dump_vectors(vec, items)
    binary = str(tmp_path / "isect_rows_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary, vec], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok", res.stdout
    n, credited, deleted = (int(x) for x in re.search(r"replay: (\d+) cases, (\d+) with credits, (\d+) with deleted", res.stdout).groups())
    assert n == len(items) and credited > 100 and deleted > 100
