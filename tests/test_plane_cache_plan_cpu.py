"""The plane cache's bookkeeping (trinity_amd/csrc/plane_cache.hpp: plan_plane_growth, plane_row_tables, PlaneRows) on the CPU: tests/cpp/plane_cache_plan_test.cpp —
a stand-alone program, compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run directly — prints how each (state, request) pair grows the cache, the row
tables of a four-term index and the rows' parts through one cache's life.  Every expected line below is written out by hand from the expressions the growth had before
it became a function of its own (resize = want > cap; new high region = (needs high or one exists) and (resize or none exists); capacity = max(want, cap); outgrown =
plane 0 + the four rank buffers when rows move, + 1 when the high region does), not computed with the code under test.

State: (capacity, rows exist, high region exists); request: (plane_rows, needs high)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plane_cache_plan_test.cpp")

GROWTH = [
    "(0, 0, 0) <- (0, 0): resize 1 new_high 0 copy_rows 0 copy_high 0 cap 1 outgrown 0",  # empty: one row at the least, nothing to copy
    "(0, 0, 0) <- (3, 1): resize 1 new_high 1 copy_rows 0 copy_high 0 cap 3 outgrown 0",
    "(3, 1, 0) <- (2, 0): nothing",
    "(3, 1, 0) <- (2, 1): resize 0 new_high 1 copy_rows 0 copy_high 0 cap 3 outgrown 0",  # the rows stay where they are
    "(3, 1, 0) <- (5, 0): resize 1 new_high 0 copy_rows 1 copy_high 0 cap 5 outgrown 5",  # plane 0 + the four rank buffers
    "(3, 1, 1) <- (5, 0): resize 1 new_high 1 copy_rows 1 copy_high 1 cap 5 outgrown 6",  # the high region is resized too, though this batch does not read it
    "(5, 1, 1) <- (3, 1): nothing",
]
# df_rank = {2, 0, 5, 1}, documents = {7, 9, 4, 8}, capacity 4: a term whose rank is at or past the capacity is absent, a rank with no term adds nothing
TABLES = ["rank_term: 1 3 0 none", "hs_off: 0 9 17 24 24"]
# one cache through its life (a row's parts: 1 plane 0, 2 the high part, 4 rank records and hits entries); lists are (term, row) pairs; docbytes = {70, 90, 40, 80}
LIFE = [
    "cap 3 high 0 build 0 2 1 0 bytes 160",  # terms 0, 1, 2 -> rows 2, 0 and none (rank 5)
    "built 1 0 1",
    "again: build bytes 0",
    "rebuild: build 0 2 1 0 bytes 160",  # planes_rebuild: every row again
    "high added: cap 3 high 1 built 1 0 1 hs_off.size 4",  # no resize: plane 0 kept, no row has its high bit, the tables stay
    "scored: build 1 0 bytes 90",  # row 0 lacks its high part
    "grown: cap 5 high 1 built 3 0 1 0 0 hs_off.size 6",  # the parts move with the rows
    "phrases: pairs 3 1 0 2 max_blocks 8 first 0 pairs_n 2 built 3 5 5 0 0",  # term 3 named twice, taken once; term 2 has no row
    "phrases: pairs 1 0 2 4 max_blocks 9 first 2 pairs_n 4 built 7 5 5 0 5",  # appended behind the first run's pairs; row 1 has its records
]


def test_growth_plan_row_tables_and_row_parts(tmp_path):
    binary = str(tmp_path / "plane_cache_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",  # (static runtimes: checked whatever the environment preloads)
                    "-o", binary, SRC], check=True)  # fmt: skip
    res = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "AddressSanitizer" not in res.stderr and "runtime error:" not in res.stderr, res.stderr[-3000:]
    assert res.stdout.splitlines() == GROWTH + TABLES + LIFE + ["ok"], res.stdout
