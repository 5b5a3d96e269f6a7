"""The read side's host transforms (trinity_amd/csrc/host/result_rows.hpp: widen, narrow, expand) on the CPU: tests/cpp/result_rows_cpu_test.cpp — a stand-alone
program, compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run directly — compares each with a naive out-of-place restatement on arrays of the
exact size: segment counts 0 .. 65 (at 1 a cell's low word lies in its own upper half), strided rows of 0 .. 2049 matches, bitmaps whose tasks counted one
document less and one more than they hold (both error returns, nothing stored at out[n])."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "result_rows_cpu_test.cpp")


def test_the_transforms_equal_their_restatements(tmp_path):
    binary = str(tmp_path / "result_rows_cpu_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",  # (static runtimes: checked whatever the environment preloads)
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok" and "widen: 36 cases" in lines and "narrow: 12 cases" in lines, res.stdout
    more, fewer = (int(x) for x in re.search(r"expand: more (\d+) fewer (\d+)", res.stdout).groups())
    assert more > 0 and fewer > 0  # both error returns occurred
