"""CPU checks of the collection-ranking cases (tests/crank_cases.py): on the oracle alone, that the three worlds CAN tell a right merge of the sources' ranked lists
from a wrong one — and ProximityRanker::blend (trinity_amd/csrc/host/trinity_gpu.hpp), the host form of the device merge, as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/crank_blend_test.cpp) against the same restatement."""
import os
import subprocess

import pytest

import crank_cases as CR
import oracle_lib as O
from wide_terms_cases import NARROW, NARROW_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "crank_blend_test.cpp")
TEXTS = list(dict.fromkeys(CR.PAIR_QUERIES + NARROW))


def progs():
    return [O.parse_query(t, some_min=NARROW_MIN) for t in TEXTS]


def test_the_inputs_can_tell_a_right_merge_from_a_wrong_one():
    all_three = tie_spans = not_in_source_order = empty_source = 0
    for text, prog in zip(TEXTS, progs()):
        lists = CR.source_rows(prog, CR.CAP, CR.ADJ, CR.w3)
        got = CR.want(prog, CR.K, CR.CAP, CR.ADJ, CR.w3)
        everything = CR.blend(lists, 1 << 30)
        all_three += {r[-1] for r in got} == {0, 1, 2}
        if len(got) == CR.K:
            tie_spans += len({r[-1] for r in everything if r[1] == got[-1][1]}) >= 2
        in_source_order = [r for rows in lists for r in rows[: CR.K]][: CR.K]
        not_in_source_order += [(r[0], r[1]) for r in in_source_order] != [(r[0], r[1]) for r in got]
        empty_source += any(not rows for rows in lists) and any(rows for rows in lists)
        # (the masks hold: no document of a newer source's range is left in an older source)
        assert all(r[0] > CR.UPDATES[1] for r in lists[0]) and all(r[0] > CR.UPDATES[2] for r in lists[1]), text
    assert all_three >= 1 and tie_spans >= 1 and not_in_source_order >= 1 and empty_source >= 1, (all_three, tie_spans, not_in_source_order, empty_source)


def test_without_masks_the_sources_share_docids():
    prog = O.parse_query("t5")
    got = CR.want(prog, 256, 1, 0.0, None, masked=False)
    docs = [r[0] for r in got]
    assert any(docs.count(d) >= 2 for d in docs)  # the same docID from two sources at one score: both stay ...
    for a, b in zip(got, got[1:]):
        if a[0] == b[0]:
            assert a[1] == b[1] and a[-1] < b[-1]  # ... the older source's first


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("crank_blend") / "crank_blend_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",  # (static runtimes: checked whatever the environment preloads)
                    "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",  # (the header's engine-calling inlines are never reached from main: dropped, so nothing of libtrinity_hip.so is linked)
                    "-o", out, SRC], check=True)  # fmt: skip
    return out


def test_blend_is_the_stable_merge(binary, tmp_path):
    want, lines = {}, []
    params = [("k1", 1, CR.CAP, CR.ADJ, CR.w3, True), ("k10", 10, CR.CAP, CR.ADJ, CR.w3, True), ("k256", 256, CR.CAP, CR.ADJ, CR.w3, True), ("ties", 10, 1, 0.0, None, True),
              ("shared", 256, 1, 0.0, None, False)]  # fmt: skip
    for qi, prog in enumerate(progs()):
        for tag, K, cap, adj, fn, masked in params:
            name = f"q{qi}-{tag}"
            lists = [rows[:K] for rows in CR.source_rows(prog, cap, adj, fn, masked)]  # (what each source's ranker keeps)
            lines.append(f"case {name} {K} {len(lists)}")
            lines += [" ".join([str(len(rows))] + [f"{r[0]}:{CR.bits(r[1])}" for r in rows]) for rows in lists]
            want[name] = [(r[0], CR.bits(r[1])) for r in CR.want(prog, K, cap, adj, fn, masked)]
    # a hand-made case: -0.0 and 0.0 tie (the docID decides), and the same pair from three sources stays three times
    nz, pz = CR.bits(-0.0), CR.bits(0.0)
    lines += ["case zeros 5 3", f"2 7:{nz} 9:{pz}", f"2 3:{pz} 7:{pz}", f"1 7:{nz}"]
    want["zeros"] = [(3, pz), (7, nz), (7, pz), (7, nz), (9, pz)]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    res = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    got = {}
    for l in res.stdout.splitlines():
        name, n, *pairs = l.split()
        assert int(n) == len(pairs)
        got[name] = [tuple(int(x) for x in p.split(":")) for p in pairs]
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name
