#!/usr/bin/env python3
"""Perf probe (GPU): the ranked list of a COLLECTION, merged on the device (tri_cbatch_ranked, csrc/k_rich_rank.hpp: k_rank_merge_sources) against the merge an
application had to do itself.  SOURCES segments of DOCS / SOURCES documents each (seeds 42, 43, ...: one vocabulary, no masks, so docIDs recur across sources), one
TRI_FLAG_MATCHED_TERMS batch of 2-term conjunctions and 5-term unions per source (Zipf terms, query seed 1337 — tools/probe_rank.py's queries), every part with the
same ranker.  After the same run + sync of the collection batch, two ways to the collection's top-K lists:
  (a) every part's ranked() read back, and the lists merged in numpy (a stable sort by score descending, docID ascending over the parts in source order);
  (b) CollectionBatch.ranked().
Prints, and writes as JSON (OUT=path), the wall time of run + sync, of (a) and of (b) (host clock; every read-back ends in a device synchronise; each of RUNS timed
runs after a warm-up one, all values kept), the bytes each way copies to the host, and the merge kernel's device time (HIP events: option crank_merge_last_us).  The
two ways' lists are compared bit for bit before any time is taken.
   NQ=128 DOCS=10000000 VOCAB=1000000 SOURCES=4 RUNS=5 K=10 OUT=profiles/crank_probe.json python tools/probe_crank.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import workloads as W

D, V, NQ, RUNS = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), int(os.environ.get("NQ", 128)), int(os.environ.get("RUNS", 5))
K, CAP, ADJ, NSRC = int(os.environ.get("K", 10)), 3, 4.0, int(os.environ.get("SOURCES", 4))


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def read_parts(parts):
    lists = [b.ranked() for b in parts]
    return lists, sum(d.nbytes + s.nbytes + c.nbytes for d, s, c in lists)


def host_merge(lists):
    """The parts' lists one after the other, per query sorted stably by (-score, docID) and cut to K; rows past the count zero"""
    d = np.zeros((NQ, K), dtype=np.uint32)
    s = np.zeros((NQ, K), dtype=np.float64)
    c = np.zeros(NQ, dtype=np.uint32)
    for q in range(NQ):
        docs = np.concatenate([pd[q, : pc[q]] for pd, _, pc in lists])
        scores = np.concatenate([ps[q, : pc[q]] for _, ps, pc in lists])
        order = np.lexsort((docs, -scores))[:K]  # (lexsort is stable: equal (score, docID) pairs stay in source order)
        c[q] = len(order)
        d[q, : len(order)], s[q, : len(order)] = docs[order], scores[order]
    return d, s, c


def main():
    progs = W.and2(T.gen_queries(V, 1337, NQ // 2, 2)) + W.or5(T.gen_queries(V, 1339, NQ - NQ // 2, 5))
    dev = T.Device(0)
    ixs = [T.Index.from_segment(dev, T.Segment(D // NSRC, V, 10, 42 + i)) for i in range(NSRC)]
    print(f"{NSRC} segments of {D // NSRC} documents uploaded", flush=True)
    parts = [T.Batch(ix, progs, T.FLAG_MATCHED_TERMS) for ix in ixs]
    for b in parts:
        b.set_ranker(K, CAP, ADJ)
    cb = T.CollectionBatch(parts)
    cb.run()  # (warm-up: code objects, the pool's first growth, the plane rows, the merged blocks)
    cb.sync()
    lists, bytes_a = read_parts(parts)
    merged_a, merged_b = host_merge(lists), cb.ranked()
    for x, y in zip(merged_a, merged_b):  # the same lists, bit for bit, before any time is taken
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    bytes_b = sum(x.nbytes for x in merged_b)
    res = {"docs": D, "sources": NSRC, "docs_per_source": D // NSRC, "vocab": V, "queries": NQ, "shape": f"{NQ // 2} 2-term conjunctions + {NQ - NQ // 2} 5-term unions", "topk": K,
           "freq_cap": CAP, "adjacency": ADJ, "runs": RUNS, "lists_equal": True, "matches": int(cb.counts().sum()), "entries_merged": int(sum(int(c.sum()) for _, _, c in lists)),
           "bytes_to_host_a": int(bytes_a), "bytes_to_host_b": int(bytes_b), "run_sync_ms": [], "a_read_parts_ms": [], "a_numpy_merge_ms": [], "b_ranked_ms": [], "merge_kernel_us": []}  # fmt: skip
    for i in range(RUNS):
        _, t = timed(lambda: (cb.run(), cb.sync()))
        res["run_sync_ms"].append(t)
        res["merge_kernel_us"].append(dev.get_option("crank_merge_last_us"))
        for way in ("ab", "ba")[i % 2]:  # (alternating which way goes first)
            if way == "a":
                (lists, _), t = timed(lambda: read_parts(parts))
                res["a_read_parts_ms"].append(t)
                _, t = timed(lambda: host_merge(lists))
                res["a_numpy_merge_ms"].append(t)
            else:
                _, t = timed(cb.ranked)
                res["b_ranked_ms"].append(t)
    print(f"{res['shape']}; {NSRC} sources of {D // NSRC} documents, {res['matches']} matches, top-{K}: {res['entries_merged']} entries merged into {int(merged_b[2].sum())}")
    print(f"  run + sync of the collection batch: {min(res['run_sync_ms']):.2f} .. {max(res['run_sync_ms']):.2f} ms")
    print(f"  (a) parts' ranked() + numpy merge : {min(res['a_read_parts_ms']):.3f} .. {max(res['a_read_parts_ms']):.3f} ms + {min(res['a_numpy_merge_ms']):.3f} .. {max(res['a_numpy_merge_ms']):.3f} ms;"
          f"  {bytes_a} bytes to the host ({NSRC} x (nq x K x 12 + nq x 4))")
    print(f"  (b) CollectionBatch.ranked()      : {min(res['b_ranked_ms']):.3f} .. {max(res['b_ranked_ms']):.3f} ms;  {bytes_b} bytes to the host (nq x K x 12 + nq x 4)")
    print(f"  merge kernel, HIP events: {min(res['merge_kernel_us'])} .. {max(res['merge_kernel_us'])} us")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    cb.close()
    for b in parts:
        b.close()
    for ix in ixs:
        ix.close()
    dev.close()


if __name__ == "__main__":
    main()
