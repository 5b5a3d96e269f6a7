"""The query shapes of the wide-report tests (option rich_max_terms: default-mode queries of 17 .. 64 reportable terms) — a helper module, imported by
tests/test_planner_wide_terms.py, tests/test_gpu_wide_terms.py and tests/test_host_mirror_wide_terms.py.  The expected totals are the CPU oracle's default
mode (exec_rich: matches / matched terms over all matches / hits over all matches) on Index.generate(D, V, 10, 42) at (D, V) = (2000, 200) and (66000, 500)."""


def _or(lo, hi):
    return " OR ".join(f"t{i}" for i in range(lo, hi))


# name, text, matchsome minimum, reportable terms, (n, terms_total, hits_total) at D = 2000 and at D = 66000
SHAPES = [
    ("or17", _or(0, 17), 1, 17, (2000, 8760, 11703), (65946, 256058, 333844)),  # 18 nodes: the narrow leaf kernel, the first width past 16
    ("or33", _or(0, 33), 1, 33, (2000, 10880, 13882), (65991, 317549, 397068)),  # narrow kernel, bit 32 in use
    ("or64", _or(0, 64), 1, 64, (2000, 13178, 16211), (66000, 380266, 460694)),  # 65 nodes: the wide leaf kernel, every bit
    ("or-of-and40", " OR ".join(f"(t{i} t{i + 1})" for i in range(40)), 1, 41, (1573, 4828, 6554), (45322, 127347, 168030)),  # 121 nodes
    ("some60", "[" + ", ".join(f"t{i}" for i in range(60)) + "]", 4, 60, (1979, 12918, 15893), (62283, 363654, 437322)),  # 61 nodes, narrow
    ("not-wide", f"({_or(0, 40)}) NOT ({_or(40, 60)})", 1, 40, (943, 5754, 7397), (35862, 191798, 240152)),  # the excluded side reports nothing
    ("opt-wide", "t1 <" + " OR ".join(f"(t{i} t{i + 3})" for i in range(2, 40)) + ">", 1, 42, (1186, 2214, 2841), (35244, 58227, 73284)),
    # 54 reportable terms, t0 is bit 31, t1 bit 32, t2 bit 33: the mask of "t0 t1" lies in both words
    ("straddle", f'{_or(40, 71)} OR "t0 t1" OR "t1 t2" OR {_or(80, 100)}', 1, 54, (1649, 3331, 3909), (49769, 92338, 105496)),
]  # fmt: skip
WORLDS = [(2000, 200, 10, 42), (66000, 500, 10, 42)]  # (under one RICH_TILE of 2048 matches; many tiles, and past the tree kernels' 65 536-document chunk)
OPTS = {"rich_max_terms": 64, "tree_max_nodes": 1024}
OR65 = _or(0, 65)  # one term more than the oracle's default mode holds: checked for its status only, never handed to exec_rich
# queries of at most 16 reportable terms, from the existing default-mode tests (test_gpu_parity.py, test_planner_wide.py)
NARROW = ["t0 t1", "t5", "t0 OR t1 OR t2", 't0 OR "t1 t2"', 't0 NOT ("t1 t2" t3)', "[t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11]", '"t0 t1" OR "t1 t2" OR "t2 t3"',
          't0 <"t1 t2">']  # fmt: skip
NARROW_MIN = 2  # (the matchsome's minimum)


def shape_programs(O):
    return [O.parse_query(text, some_min=mn) for _, text, mn, *_ in SHAPES]


def narrow_programs(O):
    return [O.parse_query(t, some_min=NARROW_MIN) for t in NARROW]


def mixed_programs(O):
    """The eight shapes interleaved with the eight narrow queries: wide, narrow, wide, narrow, ... -> (programs, indices of the narrow ones)"""
    out = []
    for a, b in zip(shape_programs(O), narrow_programs(O)):
        out += [a, b]
    return out, list(range(1, len(out), 2))
