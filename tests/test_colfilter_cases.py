"""CPU tests of the column-filter cases (tests/colfilter_cases.py): the expected drop sets that tests/test_gpu_colfilter.py holds the engine to tell the right answer from
nine wrong implementations, one named case each —
  shift           a column read one docID off;
  signed          signed compares;
  hi_exclusive    an exclusive `hi`;
  no_negate       `negate` ignored;
  any_as_all      `any` taken as all;
  set_wrap        a SET value of 65536 or more wrapping into the set;
  modes_swapped   the modes swapped;
  no_also         `also` ignored;
  tail_unwritten  the last partial word left unwritten
— on the stream corpus (D = 2 SPAN_BITS + 37: it ends in a partial 64-document group and a partial word) and on the tiny fixture corpus (smaller than one chunk of
k_filter_columns); no case is vacuous; and csrc/host/column_pred.hpp — the validation behind tri_filters_from_columns and the host evaluation behind the operator surface's
ColumnPredicateFilter — equals the contract on every case and refuses every invalid shape: a stand-alone program built with -fsanitize=address,undefined (nothing
sanitised is loaded into Python).  No GPU here."""
import os
import subprocess

import numpy as np
import pytest

import colfilter_cases as CF
import oracle_lib as O
import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "colpred_cpu_test.cpp")
# which case tells which mutant (the case in both modes unless a mode is named)
TELLS = {
    "shift": "lo_eq_hi", "signed": "across_the_sign_bit", "hi_exclusive": "lo_eq_hi", "no_negate": "negated_range", "any_as_all": "two_any", "set_wrap": "set_with_65535",
    "modes_swapped": "docs_1_to_mid", "no_also": "also_create", "tail_unwritten": "last_partial_word/drop",
}  # fmt: skip


@pytest.fixture(scope="module")
def corpora():
    """name -> (D, columns, cases, {also kind: bool [D + 1]})."""
    out = {}
    c = S.stream_corpus()
    docset = c.evaluate(S.programs([(c.q(CF.ALSO_QUERY["stream"]), 1)])[0])
    out["stream"] = (c.D, CF.columns(c.D), CF.cases(c.D), {k: CF.also_bits(k, c.D, docset) for k in ("create", "docset")})
    t = CF.TINY
    ora = O.Index.generate(t["D"], t["V"], t["slots"], t["seed"])
    docset = ora.exec(O.parse_query(CF.ALSO_QUERY["tiny"]), O.FLAG_DOCUMENTS_ONLY)[0]
    out["tiny"] = (t["D"], CF.columns(t["D"]), CF.cases(t["D"]), {k: CF.also_bits(k, t["D"], docset) for k in ("create", "docset")})
    return out


def test_the_corpora_and_constants_are_what_the_cases_assume(corpora):
    assert CF.CHUNK == 2048 and CF.CHUNK % 64 == 0 and S.SPAN_BITS % CF.CHUNK == 0  # (a bitmap's extent is whole chunks)
    assert (CF.MAX_CLAUSES, CF.MAX_COLUMNS, CF.MAX_PREDS, CF.SET_LIMIT) == (8, 8, 256, 65536)
    D = corpora["stream"][0]
    assert D == 2 * S.SPAN_BITS + 37 and D % 64 == 37 and D % 32 == 5 and corpora["tiny"][0] < CF.CHUNK
    names = {c.name for c in corpora["stream"][2]}
    for m in range(CF.CHUNK, D + 1, CF.CHUNK):  # both sides of every multiple of the chunk lie in some `astride` case
        assert any(cl["lo"] == D - m and cl["hi"] == D - m + 1 for c in corpora["stream"][2] if c.name.startswith("astride_chunks") for cl in c.clauses), m
    assert {f"{k}_span_{m}/{md}" for k in ("below", "from", "astride") for m in (S.SPAN_BITS, 2 * S.SPAN_BITS) for md in ("keep", "drop")} <= names
    for name, (D, cols, cases, also) in corpora.items():
        assert set(cols) == set(CF.COLUMN_NAMES) and all(v.size == D + 1 and v.dtype == np.uint32 for v in cols.values())
        assert cols["hash"].max() >= 0x80000000 and cols["huge"].max() == CF.HUGE and cols["rev"][1] == D - 1 and cols["rev"][D] == 0
        for k, bits in also.items():
            assert 0 < bits[1:].sum() < D, (name, k)  # each `also` filter drops some documents and keeps others
        assert len(cases) == 2 * len(CF.predicates(D)) and sum(c.keep for c in cases) * 2 == len(cases)
        assert any(len(c.clauses) == 8 and len({cl["col"] for cl in c.clauses}) == 8 for c in cases) and any(len(c.clauses) == 8 and len({cl["col"] for cl in c.clauses}) == 1 for c in cases)
        assert {c.also for c in cases} == {None, "create", "docset"}


def test_no_case_is_vacuous(corpora):
    for name, (D, cols, cases, also) in corpora.items():
        for c in cases:
            n = int(CF.holds(c, cols)[1:].sum())
            if c.trivial:
                assert n == (D if c.trivial == "all" else 0), (name, c)
            else:
                assert 0 < n < D, (name, c, n)
            if c.also:  # the `also` filter changes the answer: it drops documents the predicate's own rule keeps
                assert not np.array_equal(CF.drop_bits(c, cols, D, also[c.also]), CF.drop_bits(c, cols, D)), (name, c)


@pytest.mark.parametrize("mutant", CF.MUTANTS)
def test_the_cases_tell_each_wrong_implementation(corpora, mutant):
    for name, (D, cols, cases, also) in corpora.items():
        told = [c.name for c in cases if not np.array_equal(CF.drop_bits(c, cols, D, also.get(c.also)), CF.drop_bits(c, cols, D, also.get(c.also), mutant))]
        named = [n for n in told if n == TELLS[mutant] or n.split("/")[0] == TELLS[mutant]]
        assert named and (len(named) == 2 or "/" in TELLS[mutant]), (name, mutant, told[:8])
        # ... and every case is told from the wrong answer it is about, in both modes, on both corpora
        print(f"{name}: {mutant} told by {len(told)} of {len(cases)} cases")


def test_words_and_bits_round_trip():
    D = 37 + 64
    bits = np.zeros(D + 1, dtype=bool)
    bits[[1, 31, 32, 33, 63, 64, D]] = True
    w = CF.words_of(bits, 8)
    assert w.dtype == np.uint32 and w.size == 8 and w[0] == (1 << 1) | (1 << 31) and w[1] == 3 | (1 << 31) and w[2] == 1 and w[3] == 1 << (D & 31)
    assert np.array_equal(CF.bits_of(w, D), bits)


def test_host_evaluation_equals_the_contract_under_sanitizers(corpora, tmp_path):
    """csrc/host/column_pred.hpp: validate() accepts every case and drops() equals the numpy contract for every document of every case on both corpora; every invalid
    shape of tri_filters_from_columns is refused with a message that names the predicate and the clause."""
    out, ncases = [len(corpora)], 0
    for name, (D, cols, cases, also) in corpora.items():
        out += [D, len(CF.COLUMN_NAMES)]
        for n in CF.COLUMN_NAMES:
            out += [cols[n].size] + cols[n].tolist()
        out.append(len(cases))
        nwords = D // 32 + 1
        for c in cases:
            out += [1 if c.keep else 0, int(c.any), len(c.clauses)]
            for cl in c.clauses:
                out += [CF.COLUMN_NAMES.index(cl["col"]), 0 if cl["kind"] == "range" else 1, int(cl["negate"]), cl["lo"], cl["hi"], len(cl["set"])] + cl["set"]
            if c.also:
                out += [1, nwords] + CF.words_of(also[c.also], nwords).tolist()
            else:
                out.append(0)
            out += [nwords] + CF.words_of(CF.drop_bits(c, cols, D, also.get(c.also)), nwords).tolist()
            ncases += 1
    vec = tmp_path / "colpred_vectors.bin"
    np.asarray(out, dtype=np.uint32).tofile(vec)
    binary = str(tmp_path / "colpred_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary, str(vec)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    words = res.stdout.split()
    assert words[:4] == ["cases", str(ncases), "bad", "0"] and ncases > 100, res.stdout
    assert words[4] == "refusals" and int(words[5]) >= 19 and words[6:8] == ["bad", "0"], res.stdout
