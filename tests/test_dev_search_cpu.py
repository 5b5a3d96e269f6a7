"""The kernels' scalar searches (trinity_amd/csrc/dev_search.hpp: first_ge, first_gt, gallop_ge, term_block_range) on the CPU:
tests/cpp/dev_search_cpu_test.cpp — a stand-alone program, compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run directly — compares them
with std::lower_bound, std::upper_bound and a linear scan on every sorted array of 0 .. 9 elements over five values (duplicates included, 0xffffffff among
them), every lo <= hi sub-range, ten keys (0 and 0xffffffff among them), every gallop start, and once through a permuting accessor."""
import os
import subprocess
from math import comb

import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dev_search_cpu_test.cpp")
VALUES, KEYS = 5, 10
TERM_BLOCKS, TERM_STRIDE = 40, 700  # term_run(): block b ends at docID 700 (b + 1)


def test_the_searches_equal_the_standard_ones(tmp_path):
    binary = str(tmp_path / "dev_search_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",  # (static runtimes: checked whatever the environment preloads)
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    arrays = [comb(n + VALUES - 1, VALUES - 1) for n in range(10)]  # sorted arrays of n elements over VALUES values
    ranges = sum(a * KEYS * (n + 1) * (n + 2) // 2 for n, a in enumerate(arrays))  # ... times every key and every lo <= hi
    starts = sum(a * KEYS * (n + 1) for n, a in enumerate(arrays))  # ... every key and every `from` in [0, n]
    cells = TERM_BLOCKS * TERM_STRIDE // S.CELL_DOCS + 3  # term_block_range: every cell-aligned d_lo <= d_hi below the last two cells
    terms = (cells - 1) * cells // 2
    assert lines[-1] == "ok", res.stdout
    assert lines[:-1] == [f"arrays: {sum(arrays)}", f"first_ge: {ranges} cases", f"first_gt: {ranges} cases", f"gallop_ge: {starts} cases",
                          f"permuted: {151 * 101} cases", f"terms: {terms} cases"], res.stdout  # fmt: skip
