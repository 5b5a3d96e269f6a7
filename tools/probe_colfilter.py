#!/usr/bin/env python3
"""Perf probe (GPU): what tri_filters_from_columns costs (csrc/k_filter_columns.hpp) next to the only path there was before it.  10 M documents, two resident columns
(price: a hash of the docID below 1000; category: docID % 50); predicate i = "price in a 300-wide band AND category among three values", np of them a call for np in
1, 16, 256.
  device   best of RUNS calls of tri_filters_from_columns (wall time of the call: it returns once all np bitmaps stand);
  host     the same predicates evaluated in numpy over the host copies of the columns, then np calls of tri_filter_create with the kept docIDs (allow-lists) — best of
           BASE_RUNS (1 at np = 256: a pass takes tens of seconds).
Prints a table and writes the JSON (stdout's last line) with both times, the column bytes a call reads once, the bitmap bytes it writes and the implied GB/s.
   DOCS=10000000 RUNS=5 BASE_RUNS=2 python tools/probe_colfilter.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T

D, RUNS, BASE_RUNS = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("RUNS", 5)), int(os.environ.get("BASE_RUNS", 2))
seg = T.Segment(D, 1000, 2, 42)  # (the postings do not matter here: the filters span the segment's docIDs)
dev = T.Device(0)
ix = T.Index.from_segment(dev, seg)
d = np.arange(D + 1, dtype=np.uint64)
price = (((d * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) % np.uint64(1000)).astype(np.uint32)
category = (d % np.uint64(50)).astype(np.uint32)
cprice, ccat = T.Column(ix, price), T.Column(ix, category)
words = (D // 131072 + 2) * 4096


def spec(i):
    return (i * 37) % 700, (i * 37) % 700 + 300, [(i * 7) % 50, (i * 7 + 11) % 50, (i * 7 + 23) % 50]


def device(n):
    preds = [T.Predicate([T.Clause.range(cprice, spec(i)[0], spec(i)[1]), T.Clause.among(ccat, spec(i)[2])]) for i in range(n)]
    t0 = time.perf_counter()
    fl = T.Filter.from_columns(ix, preds, keep=True)
    dt = time.perf_counter() - t0
    return dt, fl


def host(n):
    t0 = time.perf_counter()
    fl = []
    for i in range(n):
        lo, hi, cats = spec(i)
        keep = (price >= lo) & (price <= hi) & np.isin(category, cats)
        keep[0] = False
        fl.append(T.Filter(ix, np.nonzero(keep)[0].astype(np.uint32), keep=True))
    dt = time.perf_counter() - t0
    return dt, fl


def close(fl):
    for f in fl:
        f.close()


close(device(1)[1])  # (warm: the pool's buffers, the kernel's code object)
rows = []
print(f"D = {D}, two columns ({2 * (D + 1) * 4 / 1e6:.1f} MB read once a call), a bitmap = {words * 4 / 1e6:.2f} MB")
for n in (1, 16, 256):
    best_dev, same = None, None
    for _ in range(RUNS):
        dt, fl = device(n)
        if same is None:  # the two paths build the same bitmaps (documents 1 .. D)
            ref = host(1)[1]
            a, b = fl[0].bitmap(), ref[0].bitmap()
            bits = lambda w: np.unpackbits(w.view(np.uint8), bitorder="little")[1 : D + 1]  # noqa: E731
            same = bool(np.array_equal(bits(a), bits(b)))
            close(ref)
        close(fl)
        best_dev = dt if best_dev is None else min(best_dev, dt)
    best_host = None
    for _ in range(1 if n == 256 else BASE_RUNS):
        dt, fl = host(n)
        close(fl)
        best_host = dt if best_host is None else min(best_host, dt)
    col_bytes, bitmap_bytes = 2 * (D + 1) * 4, n * words * 4
    rows.append({"np": n, "device_ms": best_dev * 1e3, "host_ms": best_host * 1e3, "column_bytes_read_once": col_bytes, "bitmap_bytes_written": bitmap_bytes,
                 "device_gb_per_s": (col_bytes + bitmap_bytes) / best_dev / 1e9, "speedup": best_host / best_dev, "bitmaps_equal": same})  # fmt: skip
    print(f"  np {n:3d}: device {best_dev * 1e3:9.3f} ms ({rows[-1]['device_gb_per_s']:7.1f} GB/s over {col_bytes / 1e6:.1f} + {bitmap_bytes / 1e6:.1f} MB)   host {best_host * 1e3:10.1f} ms   x{best_host / best_dev:.0f}   equal {same}")
out = {"probe": "colfilter", "docs": D, "columns": 2, "clauses_per_predicate": 2, "runs": RUNS, "rows": rows}
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
print(json.dumps(out))
for c in (cprice, ccat):
    c.close()
ix.close()
dev.close()
