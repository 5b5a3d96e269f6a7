"""The consumers' walk of a task's documents (trinity_amd/csrc/docset_walk.hpp: docset_for_each, by k_facet and k_stats) on the CPU: tests/cpp/docset_walk_cpu_test.cpp —
a stand-alone program, compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run directly — takes the shares of a workgroup's threads one after the other and
checks that every document of the task is handed over exactly once with the right docID: segments of 0, 1, WG - 1, WG and WG + 1 documents, and a RESULT_BITMAP task of
one window whose words are all zero, a single bit at position 0, a single bit at position 31 of the last word, and all ones."""
import os
import subprocess

import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "docset_walk_cpu_test.cpp")
WG = 256


def test_every_document_is_handed_over_exactly_once(tmp_path):
    binary = str(tmp_path / "docset_walk_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",  # (static runtimes: checked whatever the environment preloads)
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    assert res.stdout.splitlines() == [f"segment {c}: {c} documents" for c in (0, 1, WG - 1, WG, WG + 1)] + [
        "bitmap all zero: 0 documents", "bitmap bit 0: 1 documents", "bitmap bit 31 of the last word: 1 documents", f"bitmap all ones: {S.SPAN_BITS} documents", "ok"], res.stdout  # fmt: skip
