"""ProximityRanker::consider (trinity_amd/csrc/host/trinity_gpu.hpp) on the CPU: tests/cpp/rank_cpu_test.cpp — a stand-alone program, compiled with AddressSanitizer
and UndefinedBehaviorSanitizer and run directly — reads the oracle's default-mode records, feeds them to the ranker as matched_documents and prints the list it
keeps.  The list must be the restatement's (tests/rank_cases.py), bit for bit, on the cases of tests/test_gpu_rank.py's tests 1 - 3."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rank_cases as R
from wide_terms_cases import NARROW, NARROW_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rank_cpu_test.cpp")
NON_DYADIC = [0.1, -0.7, 1.0 / 3.0, 0.45, 2.3, 0.9]
# name suffix, topk, freq_cap, adjacency, weight of slot k
PARAMS = [("k1", 1, 3, 4.0, lambda k: 1 + k % 3), ("k10", 10, 3, 4.0, lambda k: 1 + k % 3), ("k256", 256, 3, 4.0, lambda k: 1 + k % 3),
          ("ties", 10, 1, 0.0, lambda k: 1.0), ("nondyadic", 256, 5, 0.3, lambda k: NON_DYADIC[k % 6])]  # fmt: skip


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rank_cpu") / "rank_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",  # (static runtimes: checked whatever the environment preloads)
                    "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",  # (the header's engine-calling inlines are never reached from main: dropped, so nothing of libtrinity_hip.so is linked)
                    "-o", out, SRC], check=True)  # fmt: skip
    return out


# (the large world under the parity parameters only: its records are written once per case)
@pytest.mark.parametrize("world,params", [((2000, 200, 10, 42), PARAMS), ((66000, 500, 10, 42), PARAMS[1:2]), ((6000, 400, 90, 11), PARAMS)], ids=["2000", "66000", "longdocs"])
def test_consider_keeps_the_restatements_list(binary, tmp_path, world, params):
    ora = O.Index.generate(*world)
    texts = NARROW + ["t3 t1 t0", " ".join(f"t{world[1] - 1 - i}" for i in range(5))]
    want, lines = {}, []
    for qi, text in enumerate(texts):
        prog = O.parse_query(text, some_min=NARROW_MIN)
        flat = ora.exec_rich(prog)[1]
        recs = R.records(flat)
        slot_terms, _ = R.slots(prog)
        for tag, K, cap, adj, fn in params:
            name = f"q{qi}-{tag}"
            w = [float(fn(k)) for k in range(len(slot_terms))]
            lines.append(" ".join(["case", name, str(K), str(cap), float(adj).hex(), str(len(slot_terms))] + [x.hex() for x in w] + [str(t) for t in slot_terms] + [str(len(flat))]))
            lines.append(" ".join(str(int(x)) for x in flat))
            rows = R.rows(recs, prog, cap, adj, R.token_weights([prog], fn))[:K]
            want[name] = [(r[0], int(np.array([r[1]], dtype=np.float64).view(np.uint64)[0])) for r in rows]
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
    assert any(len(v) == params[-1][1] for v in want.values()) and want[f"q{len(texts) - 1}-k10"] == []
