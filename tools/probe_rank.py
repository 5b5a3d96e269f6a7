#!/usr/bin/env python3
"""Perf probe (GPU): what ranking the default mode's matches on the device saves (tri_batch_set_ranker, csrc/k_rich_rank.hpp).  One TRI_FLAG_MATCHED_TERMS batch of
2-term conjunctions and 5-term unions (Zipf terms, query seed 1337), two ways to the same top-K lists:
  (a) what the engine offered before: run + sync, then docset + matched_terms for EVERY query and the proximity score and the top-K in numpy on the host;
  (b) set_ranker + run + sync + ranked().
Prints, and writes as JSON (OUT=path), the wall time of each path and of its parts (host clock around work that ends in a device synchronise, best and worst of
RUNS), the device time of the WRITE pass and of the rank pass behind it (HIP events: options rich_write_last_us / rank_last_us), and the bytes each path copies to
the host.  The two paths' lists are compared bit for bit before any time is reported.
   NQ=128 DOCS=10000000 VOCAB=1000000 RUNS=3 K=10 OUT=profiles/rank_probe.json python tools/probe_rank.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import workloads as W

D, V, NQ, RUNS = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), int(os.environ.get("NQ", 128)), int(os.environ.get("RUNS", 3))
K, CAP, ADJ = int(os.environ.get("K", 10)), 3, 4.0


def host_rank(docs, present, freq, pos):
    """The contract's score over one query's matched terms (every slot's weight 1.0: slot order = the order matched_terms reports), and its top K."""
    n, nt = freq.shape
    score = np.zeros(n, dtype=np.float64)
    for k in range(nt):
        score = np.where((present >> np.uint32(k)) & np.uint32(1), score + 1.0 * np.minimum(freq[:, k], CAP).astype(np.float64), score)
    pairs = np.zeros(n, dtype=np.int64)
    if nt > 1 and pos.size:
        f64 = freq.astype(np.int64)
        owner = np.repeat(np.arange(n * nt), f64.ravel())  # per hit: match * nt + slot (pos is match-major, term-minor)
        key = (owner // nt) * 65536 + pos.astype(np.int64)
        slot = owner % nt
        for k in range(nt - 1):
            a = key[(slot == k) & (pos != 0)]
            b = key[slot == k + 1]
            hit = a[np.isin(a + 1, b)]
            pairs += np.bincount(hit // 65536, minlength=n)
    score = score + ADJ * pairs.astype(np.float64)
    order = np.lexsort((docs, -score))[:K]
    return docs[order], score[order]


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def main():
    progs = W.and2(T.gen_queries(V, 1337, NQ // 2, 2)) + W.or5(T.gen_queries(V, 1339, NQ - NQ // 2, 5))
    seg = T.Segment(D, V, 10, 42)
    dev = T.Device(0)
    ix = T.Index.from_segment(dev, seg)
    print(f"segment of {D} documents uploaded", flush=True)
    res = {"docs": D, "vocab": V, "queries": NQ, "shape": f"{NQ // 2} 2-term conjunctions + {NQ - NQ // 2} 5-term unions", "topk": K, "freq_cap": CAP, "adjacency": ADJ, "runs": RUNS}
    # ---- (a)
    a = T.Batch(ix, progs, T.FLAG_MATCHED_TERMS)
    a.run()  # (warm-up: code objects, the pool's first growth, the plane rows)
    a.sync()
    ta = {"run_sync_ms": [], "fetch_ms": [], "numpy_ms": []}
    for _ in range(RUNS):
        _, t = timed(lambda: (a.run(), a.sync()))
        ta["run_sync_ms"].append(t)
        counts = a.counts()

        def fetch():
            out, nbytes = [], 0
            for q in range(NQ):
                docs = a.docset(q, int(counts[q]))
                terms, present, freq, pos = a.matched_terms(q, len(docs))
                nbytes += docs.nbytes + present.nbytes + freq.nbytes + pos.nbytes
                out.append((docs, present, freq, pos))
            return out, nbytes

        (rows, bytes_a), t = timed(fetch)
        ta["fetch_ms"].append(t)
        lists_a, t = timed(lambda: [host_rank(*r) for r in rows])
        ta["numpy_ms"].append(t)
        del rows
        print(f"  (a) run {len(ta['numpy_ms'])}: {ta['run_sync_ms'][-1]:.1f} + {ta['fetch_ms'][-1]:.1f} + {ta['numpy_ms'][-1]:.1f} ms", flush=True)
    info = a.info()
    res.update(matches=int(info["matches"]), kernels_ms_unranked=float(info["last_run_ms"]))
    a.close()
    # ---- (b)
    b = T.Batch(ix, progs, T.FLAG_MATCHED_TERMS)
    b.set_ranker(K, CAP, ADJ)
    b.run()
    b.sync()
    tb = {"run_sync_ms": [], "ranked_ms": [], "write_pass_us": [], "rank_pass_us": []}
    for _ in range(RUNS):
        _, t = timed(lambda: (b.run(), b.sync()))
        tb["run_sync_ms"].append(t)
        (d, s, c), t = timed(b.ranked)
        tb["ranked_ms"].append(t)
        tb["write_pass_us"].append(dev.get_option("rich_write_last_us"))
        tb["rank_pass_us"].append(dev.get_option("rank_last_us"))
    b.close()
    for q in range(NQ):  # the same lists, bit for bit
        n = int(c[q])
        assert n == len(lists_a[q][0]) and np.array_equal(d[q, :n], lists_a[q][0]) and np.array_equal(s[q, :n].view(np.uint64), lists_a[q][1].view(np.uint64)), q
    bytes_b = d.nbytes + s.nbytes + c.nbytes
    res.update(a=ta, b=tb, bytes_to_host_a=int(bytes_a), bytes_to_host_b=int(bytes_b), lists_equal=True,
               wall_a_ms=[x + y + z for x, y, z in zip(ta["run_sync_ms"], ta["fetch_ms"], ta["numpy_ms"])], wall_b_ms=[x + y for x, y in zip(tb["run_sync_ms"], tb["ranked_ms"])])
    print(f"{res['shape']}; D = {D}, {res['matches']} matches, top-{K}")
    print(f"  (a) host ranking : wall {min(res['wall_a_ms']):10.2f} .. {max(res['wall_a_ms']):10.2f} ms  = run+sync {min(ta['run_sync_ms']):.2f} + docset/matched_terms {min(ta['fetch_ms']):.2f} + numpy {min(ta['numpy_ms']):.2f};"
          f"  {bytes_a} bytes to the host")
    print(f"  (b) device ranker: wall {min(res['wall_b_ms']):10.2f} .. {max(res['wall_b_ms']):10.2f} ms  = run+sync {min(tb['run_sync_ms']):.2f} + ranked {min(tb['ranked_ms']):.2f};"
          f"  {bytes_b} bytes to the host (nq x K x 12 + nq x 4)")
    print(f"  device time, HIP events: WRITE pass {min(tb['write_pass_us'])} us, rank pass (k_rich_rank + k_rank_merge) {min(tb['rank_pass_us'])} us")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ix.close()
    dev.close()


if __name__ == "__main__":
    main()
