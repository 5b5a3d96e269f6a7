"""The percolator's contract on the CPU (tests/perc_cases.py): its two forms agree; for every program the reference compiled (tests/golden/ref_trees.json,
ref_random.json) the documents it matches are the reference's docset (count and hash); four deliberately wrong evaluators are each told from the right one by
their case family; and the C++ mirror's percolator_query::match (trinity_amd/csrc/host/trinity_gpu.hpp), run as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer, gives the restatement's pairs."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import perc_cases as PC
from random_programs import random_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "cpp", "perc_cpu_test.cpp")


def test_the_two_forms_agree():
    rng = np.random.default_rng(7)
    for name, fam in PC.FAMILIES.items():
        progs, docs, _ = fam()
        progs = progs + [[]]
        bits = PC.match_batch(progs, docs)
        for q, p in enumerate(progs):
            assert bits[q] == sum(1 << d for d, doc in enumerate(docs) if PC.match_one(p, doc)), (name, q)
    progs = [random_program(rng, True) for _ in range(300)]
    docs = [{int(t): [int(x) for x in np.sort(rng.integers(0, 6, size=rng.integers(0, 3)))] for t in rng.choice(40, size=rng.integers(0, 12), replace=False)} for _ in range(70)]
    bits = PC.match_batch(progs, docs)
    assert any(bits) and any(b == 0 for b in bits)
    for q, p in enumerate(progs):
        assert bits[q] == sum(1 << d for d, doc in enumerate(docs) if PC.match_one(p, doc)), q
    (q1, d1), (q2, d2), counts = PC.pairs_of(bits, len(docs))
    assert sorted(zip(q1.tolist(), d1.tolist())) == sorted(zip(q2.tolist(), d2.tolist())) and counts.sum() == q1.size
    assert list(zip(d2.tolist(), q2.tolist())) == sorted(zip(d2.tolist(), q2.tolist()))


def test_the_restatement_gives_the_reference_s_docsets():
    """Percolating documents 1 .. D of the fixtures' corpus against the programs the reference compiled gives, per program, the docset the reference returned: its
    count and its hash (document d of the batch = docID d + 1)."""
    seen = 0
    for name in ("ref_trees.json", "ref_random.json"):
        g = json.load(open(os.path.join(GOLDEN, name)))
        c = g["corpus"]
        ix = O.Index.generate(c["D"], c["V"], c["slots"], c["seed"])
        docs = PC.docs_of(*PC.corpus_batch(ix.corpus, c["D"]))
        progs = [O.program_from_exec_tree(r["tree"]) for r in g["results"]]
        bits = PC.match_batch(progs, docs)
        (q, d), _, _ = PC.pairs_of(bits, len(docs))
        for i, r in enumerate(g["results"]):
            mine = d[q == i] + 1
            assert mine.size == r["n"] and str(O.fnv1a_docs(mine)) == r["fnv"], r["q"]
            seen += 1
    assert seen == 549


@pytest.mark.parametrize("mutant", PC.MUTANTS)
def test_a_wrong_evaluator_is_told_apart(mutant):
    progs, docs, _ = PC.FAMILIES[mutant]()
    right = [[PC.match_one(p, doc) for doc in docs] for p in progs]
    wrong = [[PC.match_one(p, doc, mutant) for doc in docs] for p in progs]
    assert right != wrong, mutant
    for other in PC.MUTANTS:  # (and no family is blind to the rest by accident of construction: the right evaluator is the only one every family agrees with)
        fp, fd, _ = PC.FAMILIES[other]()
        assert [[PC.match_one(p, doc, other) for doc in fd] for p in fp] != [[PC.match_one(p, doc) for doc in fd] for p in fp]


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("perc_cpu") / "perc_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",  # (static runtimes: checked whatever the environment preloads)
                    "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",  # (the header's engine-calling inlines are never reached from main: dropped, so nothing of libtrinity_hip.so is linked)
                    "-o", out, SRC], check=True)  # fmt: skip
    return out


def test_the_mirror_s_recursion_gives_the_restatement_s_pairs(binary, tmp_path):
    rng = np.random.default_rng(11)
    programs, docs = [[]], []
    for fam in PC.FAMILIES.values():
        p, d, _ = fam()
        programs += p
        docs += d
    programs += [random_program(rng, True).tolist() for _ in range(60)]
    path = str(tmp_path / "cases.txt")
    PC.write_case_file(path, programs, docs)
    res = subprocess.run([binary, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    lines = res.stdout.split("\n")
    got = [tuple(int(x) for x in l.split()) for l in lines if l and not l.startswith("pairs")]
    (q, d), _, _ = PC.pairs_of(PC.match_batch(programs, docs), len(docs))
    assert got == list(zip(q.tolist(), d.tolist())) and f"pairs {q.size}" in lines and q.size > 50
