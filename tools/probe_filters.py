#!/usr/bin/env python3
"""Perf probe (GPU): what a batch with per-query document filters costs (tri_batch_set_filters, csrc/k_filter.hpp).  cfg3's shape — 5-term mixed AND/OR, lucene_codec,
BM25 top-100 — once without filters and once with 1, 16 and 256 distinct filters that each drop a random half of the documents, the queries naming them round-robin.
Prints the step time of each (best of RUNS, HIP events) and the time of k_filter_rows: the difference of the runs' first stage (the plane rows' stage, which the
filter rows are launched in) between the filtered batch and the same batch before it had filters.
   NQ=8192 DOCS=10000000 VOCAB=1000000 RUNS=5 python tools/probe_filters.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import workloads as W

D, V, NQ, RUNS = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), int(os.environ.get("NQ", 8192)), int(os.environ.get("RUNS", 5))
progs, flags, topk, codec, desc = W.build("cfg3", D, V, 10, 42, NQ)
seg = T.Segment(D, V, 10, 42, codec=codec)
dev = T.Device(0)
ix = T.Index.from_segment(dev, seg)
b = T.Batch(ix, progs, flags, topk=topk)


def best():
    out = None
    for _ in range(RUNS):
        b.run()
        b.sync()
        i = b.info()
        if out is None or i["last_run_ms"] < out[0]:
            out = (i["last_run_ms"], i["term_planes_ms"], int(i["matches"]))
    return out


b.run()  # (the index's plane rows are built by the first run)
b.sync()
plain = best()
print(f"{desc}; {NQ} queries, D = {D}")
print(f"  no filters          : step {plain[0]:8.3f} ms   first stage {plain[1]:.3f} ms   matches {plain[2]}")
rng = np.random.default_rng(7)
for nf in (1, 16, 256):
    filters = [T.Filter(ix, np.nonzero(rng.random(D) < 0.5)[0].astype(np.uint32) + 1) for _ in range(nf)]
    b.set_filters(filters, np.arange(NQ, dtype=np.uint32) % nf)
    f = best()
    print(f"  {nf:3d} distinct filters: step {f[0]:8.3f} ms   first stage {f[1]:.3f} ms (k_filter_rows ~ {f[1] - plain[1]:.3f} ms, {nf} rows of {(D // 131072 + 2) * 16} KB)   matches {f[2]}")
    b.set_filters([])
    for x in filters:
        x.close()
again = best()
print(f"  filters cleared     : step {again[0]:8.3f} ms")
b.close()
ix.close()
dev.close()
