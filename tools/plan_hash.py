"""A refactoring net for the host planner (no GPU).  One line per leg: the SHA-1 of the plan block (every array the device reads), of the
summary (sizes, offsets, counters), of the query maps (slot_of_query, qstatus), and the ten per-kind task counts.  Run it before and after a
change that must not alter a plan and diff the outputs: a byte-identical block means byte-identical launches.  Python only — the same file
(with tests/random_programs.py) runs in a checkout of an earlier commit against that commit's libtrinity_host.so.

The legs: the cfg2 - cfg5 parts over a 2 M-document segment in both codecs on 1 and 8 threads (cfg4's and cfg5's also in the default
mode); seeded random trees and the phrase-leaf trees in all three modes (truth tables, TASK_TREE with hidden phrase queries, left-out
queries); the structured corpora of tests/structured.py under its option sets; and every planner option on its own on a cfg2, a cfg3 and
a cfg5 part.  Exits non-zero when a task kind is reached by no leg.

usage: python tools/plan_hash.py > before.txt; ...; python tools/plan_hash.py | diff before.txt -"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import trinity_amd as T
from trinity_amd import hostplan as HP, workloads as W

KINDS = ["n_cand", "n_dense", "n_fused", "n_fused16", "n_fusedgen", "n_planes", "n_planes8", "n_pset", "n_probe", "n_tree"]
reached = dict.fromkeys(KINDS, 0)
legs = 0


def sha(b):
    return hashlib.sha1(b).hexdigest()[:16]


def leg(tag, hi, programs, flags, topk, threads, options=None):
    global legs
    legs += 1
    try:
        p = HP.HostPlan(hi, programs, flags, topk, threads=threads, options=options)
    except T.TrinityError as e:
        print(tag, "thr", threads, "refused", sha(str(e).encode()))
        return
    s = p.s
    for k in KINDS:
        reached[k] += s[k]
    maps = sha(p.slot_of_query.tobytes() + p.qstatus.tobytes())
    print(tag, "thr", threads, sha(bytes(p.block)), sha(",".join(f"{k}={s[k]}" for k in HP._SUMMARY).encode()), maps, len(p.block), *[s[k] for k in KINDS],
          "left_out", int((p.qstatus[: p.nq] != 0).sum()), "hidden", s["n_tree_hidden"])  # fmt: skip
    p.close()


def workload_legs(D, V, his):
    picked = {}
    for codec in (1, 2):
        for wl in ("cfg2", "cfg3", "cfg4", "cfg5"):
            parts, _ = W.build_parts(wl, D, V, 10, 42, 4096)
            for i, pt in enumerate(parts):
                if pt.codec != codec:
                    continue
                picked[wl, i] = pt
                modes = [(pt.flags, pt.topk, "own")] + ([(T.FLAG_MATCHED_TERMS, 0, "rich")] if wl in ("cfg4", "cfg5") else [])
                for flags, topk, mode in modes:
                    for thr in (1, 8):
                        leg(f"{wl} {pt.name[:12]!r} codec {codec} {mode}", his[codec], pt.programs, flags, topk, thr)
    return picked


def option_legs(his, picked):
    row_bytes = None
    for (wl, i) in (("cfg2", 0), ("cfg3", 0), ("cfg5", 0)):
        pt = picked[wl, i]
        hi = his[pt.codec]
        if row_bytes is None:
            p = HP.HostPlan(hi, pt.programs[:8], pt.flags, pt.topk)
            row_bytes = 3 * p.s["plw"] * 4  # (a plane row: PL_PLANES bitmaps over the docID space)
            p.close()
        sets = [{"probe_max_blocks": 64}, {"planes_order": 0}, {"planes_order": 2}, {"pset_order": 0}, {"cand_xcd": 0}, {"account_needed_bytes": 1}, {"fused": 0}, {"fused": 2},
                {"fused_halfwords": 0}, {"planes_split": 65536}, {"planes": 0}, {"result_bitmaps": 0}, {"scatter_bitmap_slack": 1}, {"fused_freq_cap": 3},
                {"plane_max_bytes": 10 * row_bytes}, {"frag_cache": 1}, {"frag_cache": 1}]  # fmt: skip  (the fragment cache: planned twice in a row)
        for opts in sets:
            for thr in (1, 8):
                leg(f"{wl}[{i}] codec {pt.codec} {opts}", hi, pt.programs, pt.flags, pt.topk, thr, opts)


MODES = ((T.FLAG_DOCUMENTS_ONLY, 0, "docs"), (T.FLAG_ACCUMULATED_SCORE, 10, "top10"), (T.FLAG_MATCHED_TERMS, 0, "rich"))


def tree_legs(his):
    import oracle_lib as O
    from random_programs import random_program

    rng = np.random.default_rng(4242)
    progs = [random_program(rng, True) for _ in range(900)]
    # trees with multi-word phrase leaves (hidden phrase queries), a tree of more than 64 nodes (left out), a matchsome over phrases
    big = " OR ".join(f"(t{2 * i} t{2 * i + 1})" for i in range(40))
    texts = ['t0 OR "t1 t2"', big, "t0 OR (t1 t2) OR (t3 t4) OR (t5 t6) OR (t7 t8)", '[t0, "t1 t2", "t2 t3 t4"]', 't3 "t4 t5" NOT t6']
    progs += [O.parse_query(t, some_min=2) for t in texts] * 60
    progs = [progs[i] for i in np.random.default_rng(7).permutation(len(progs))]
    for codec in (1, 2):
        for flags, topk, mode in MODES:
            for thr in (1, 4):
                leg(f"trees codec {codec} {mode}", his[codec], progs, flags, topk, thr)


def structured_legs():
    import structured as S

    for name, make in S.CORPORA.items():
        c = make()
        docs_q = S.programs(S.QUERIES[name](c))
        scored_q, ks = S.SCORED_CASES[name]
        scored_q = S.programs(scored_q(c))
        for codec in (1, 2):
            hi = c.host_index(codec)
            for opts, _ in S.DOCS_OPTION_SETS:
                leg(f"structured {name} codec {codec} docs {opts}", hi, docs_q, T.FLAG_DOCUMENTS_ONLY, 0, 4, opts)
            for opts, _ in S.SCORED_OPTION_SETS:
                leg(f"structured {name} codec {codec} top{ks[-1]} {opts}", hi, scored_q, T.FLAG_ACCUMULATED_SCORE, ks[-1], 4, opts)
            hi.close()


def main():
    T.build.build_host()
    D, V = 2_000_000, 200_000
    his = {codec: HP.HostIndex.from_segment(T.Segment(D, V, 10, 42, codec=codec)) for codec in (1, 2)}
    picked = workload_legs(D, V, his)
    option_legs(his, picked)
    tree_legs(his)
    structured_legs()
    print("legs", legs, "reached", *[f"{k}={reached[k]}" for k in KINDS])
    missing = [k for k in KINDS if not reached[k]]
    if missing:
        sys.exit("plan_hash: no leg reaches " + ", ".join(missing))


if __name__ == "__main__":
    main()
