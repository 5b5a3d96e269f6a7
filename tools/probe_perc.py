#!/usr/bin/env python3
"""tri_perc_match (the percolator) end to end: stored sets of 10^5 and 10^6 queries built from the workloads' Zipf terms in the cfg2 shape (two-term
conjunctions) and the cfg5 shape (50 % two-term AND, 30 % five-term mixed, 10 % five-way OR, 10 % phrases of two and three words), against batches of 64, 1024 and
4096 synthetic documents (100 distinct Zipf terms each, one position per term).  Per case: warm-up calls, then the median and the spread of repeated calls, end to end
on the host and per stage from tri_perc_result_info, with option perc_prune 1 and 0.  The baseline is the same answer on one host thread from
tools/perc_host_eval.cpp (compiled here into build/): the reference's walk per (query, document) behind a term -> queries candidate index; its pairs are compared
with the device's, pair for pair.    usage: tools/probe_perc.py [--out profiles/perc_probe.json] [--sets 100000,1000000] [--calls 7]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import trinity_amd as T  # noqa: E402
from trinity_amd import engine as E  # noqa: E402

V, DOC_TERMS = 200000, 100


def tokens(op, arg):
    return (np.uint32(op) << np.uint32(28)) | np.asarray(arg, dtype=np.uint32)


def rows_to_flat(rows, tail):
    """(n, k) term rows + the operator tokens that follow them -> an (n, k + len(tail)) token matrix"""
    n = rows.shape[0]
    return np.concatenate([tokens(T.OP_TERM, rows)] + [np.full((n, 1), t, dtype=np.uint32) for t in tail], axis=1)


def stored_set(shape, nq):
    """(flat program, (nq, 2) query table) in the workloads' shapes (trinity_amd/workloads.py: and2, mixed5's four forms, or5, phrases), built as token matrices"""
    mats = []
    if shape == "cfg2":
        mats.append(rows_to_flat(E.gen_queries(V, 1337, nq, 2), [T.tok(T.OP_AND, 2)]))
    else:
        n2, n3, no = nq // 2, (nq * 3) // 10, nq // 10
        n4 = nq - n2 - n3 - no
        mats.append(rows_to_flat(E.gen_queries(V, 1337, n2, 2), [T.tok(T.OP_AND, 2)]))
        r = E.gen_queries(V, 1338, n3, 5)
        k = n3 // 4
        a = r[:k]  # A B (C|D|E)
        mats.append(np.concatenate([tokens(T.OP_TERM, a), np.full((k, 1), T.tok(T.OP_OR, 3), np.uint32), np.full((k, 1), T.tok(T.OP_AND, 3), np.uint32)], axis=1))
        b = r[k : 2 * k]  # (A|B) (C|D) E
        o2, a3 = np.full((k, 1), T.tok(T.OP_OR, 2), np.uint32), np.full((k, 1), T.tok(T.OP_AND, 3), np.uint32)
        mats.append(np.concatenate([tokens(T.OP_TERM, b[:, :2]), o2, tokens(T.OP_TERM, b[:, 2:4]), o2, tokens(T.OP_TERM, b[:, 4:]), a3], axis=1))
        mats.append(rows_to_flat(r[2 * k : 3 * k], [T.tok(T.OP_AND, 5)]))
        mats.append(rows_to_flat(r[3 * k :], [T.tok(T.OP_OR, 5)]))
        mats.append(rows_to_flat(E.gen_queries(V, 1339, no, 5), [T.tok(T.OP_OR, 5)]))
        mats.append(rows_to_flat(E.gen_queries(V, 1340, n4 // 2, 2), [T.tok(T.OP_PHRASE, 2)]))
        mats.append(rows_to_flat(E.gen_queries(V, 1341, n4 - n4 // 2, 3), [T.tok(T.OP_PHRASE, 3)]))
    flat = np.concatenate([m.reshape(-1) for m in mats]).astype(np.uint32)
    lens = np.concatenate([np.full(m.shape[0], m.shape[1], dtype=np.uint32) for m in mats])
    q = np.zeros((lens.size, 2), dtype=np.uint32)
    q[:, 1] = lens
    q[1:, 0] = np.cumsum(lens[:-1], dtype=np.uint64).astype(np.uint32)
    return flat, q


def documents(ndocs):
    """ndocs documents of DOC_TERMS distinct Zipf terms; term k of a document stands at position k + 1 of it in draw order, so drawn neighbours are adjacent"""
    rows = E.gen_queries(V, 4242, ndocs, DOC_TERMS)
    pos = np.tile(np.arange(1, DOC_TERMS + 1, dtype=np.uint16), (ndocs, 1))
    order = np.argsort(rows, axis=1, kind="stable")
    terms = np.take_along_axis(rows, order, axis=1).reshape(-1)
    positions = np.take_along_axis(pos, order, axis=1).reshape(-1)
    return np.arange(0, (ndocs + 1) * DOC_TERMS, DOC_TERMS, dtype=np.uint64), terms.astype(np.uint32), np.ones(terms.size, np.uint32), positions


def host_lib():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    so = os.path.join(ROOT, "build", "libperc_host_eval.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "perc_host_eval.cpp")], check=True)
    L = C.CDLL(so)
    L.perc_host_build.restype = C.c_void_p
    L.perc_host_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
    L.perc_host_free.argtypes = [C.c_void_p]
    L.perc_host_match.restype = C.c_uint64
    L.perc_host_match.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    return L


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perc_probe.json"))
    ap.add_argument("--sets", default="100000,1000000")
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-max-docs", type=int, default=1024, help="the host baseline runs on batches of at most this many documents")
    a = ap.parse_args()
    T.build_all()
    H = host_lib()
    dev = T.Device(0)
    out = {"method": f"{a.warmup} warm-up calls, then {a.calls} timed ones per case: median / min / max in ms; total = the call on the host clock, stages = HIP events "
                     "(tri_perc_result_info); host = tools/perc_host_eval.cpp, one thread, candidate index built beforehand (host_build_ms)",
           "vocabulary": V, "doc_terms": DOC_TERMS, "cases": []}  # fmt: skip
    batches = {n: documents(n) for n in (int(x) for x in a.batches.split(","))}
    for shape in ("cfg2", "cfg5"):
        for nq in (int(x) for x in a.sets.split(",")):
            flat, q = stored_set(shape, nq)
            t0 = time.perf_counter()
            p = T.Percolator.from_flat(dev, flat, q, V)
            create_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            hs = H.perc_host_build(flat.ctypes.data, q.ctypes.data, len(q), V)
            host_build_ms = (time.perf_counter() - t0) * 1e3
            info = p.info
            for ndocs, docs in batches.items():
                case = {"shape": shape, "queries": len(q), "ndocs": ndocs, "create_ms": round(create_ms, 2), "host_build_ms": round(host_build_ms, 2), "set": info}
                pairs = None
                for prune in (1, 0):
                    dev.set_option("perc_prune", prune)
                    runs = []
                    try:
                        for i in range(a.warmup + a.calls):
                            r = p.match(*docs)
                            if i >= a.warmup:
                                runs.append(r.info)
                            if i == a.warmup + a.calls - 1 and prune == 1:
                                pairs = r.pairs(T.PERC_BY_DOCUMENT)
                            r.close()
                    except T.TrinityError as e:
                        case[f"prune{prune}"] = {"refused": str(e)[:200]}
                        continue
                    case[f"prune{prune}"] = {k: spread([x[k] for x in runs]) for k in ("total_ms", "rows_ms", "phrases_ms", "select_ms", "eval_ms", "compact_ms")}
                    case[f"prune{prune}"].update({k: runs[-1][k] for k in ("leaf_rows", "phrase_rows", "evaluated", "hit_queries", "pairs", "scratch_bytes")})
                dev.set_option("perc_prune", 1)
                if ndocs <= a.host_max_docs and pairs is not None:
                    cap = pairs[0].size + 16
                    hq, hd, walks = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), C.c_uint64()
                    t0 = time.perf_counter()
                    n = H.perc_host_match(hs, docs[0].ctypes.data, docs[1].ctypes.data, docs[2].ctypes.data, docs[3].ctypes.data, ndocs, hq.ctypes.data, hd.ctypes.data, cap, C.byref(walks))
                    case["host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                    case["host_walks"] = walks.value
                    case["host_pairs_equal"] = bool(n == pairs[0].size and np.array_equal(hq[:n], pairs[0]) and np.array_equal(hd[:n], pairs[1]))
                out["cases"].append(case)
                print(json.dumps(case), flush=True)
            H.perc_host_free(hs)
            p.close()
    dev.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    return 0 if all(c.get("host_pairs_equal", True) for c in out["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
