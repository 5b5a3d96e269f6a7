#!/usr/bin/env python3
"""Perf probe (GPU): what counting facets on the device saves (tri_batch_set_facets, csrc/k_facet.hpp).  The cfg2 workload — NQ two-term conjunctions (Zipf terms, query
seed 1337) over the L corpus, DocumentsOnly — with one column of BUCKETS values (a multiplicative hash of the docID: no locality for the gather to lean on), two ways to
the same [NQ, BUCKETS + 1] rows:
  (a) what the engine offered before: run + sync, tri_batch_docsets into pinned host memory, numpy.bincount per query.  The delivery alone is reported too: the floor of
      ANY host approach;
  (b) set_facets + run + sync + facets(0).
Reports, per path, the host clock around work that ends in a device synchronise (all RUNS, after one warm-up of each shape), the step without facets next to the step
with them, and the device time of the row zeroing + k_facet (HIP events: option facet_last_us).  The two paths' rows are compared, integer for integer, before any time
is reported.   NQ=16384 DOCS=10000000 VOCAB=1000000 BUCKETS=1024 RUNS=5 OUT=profiles/facet_probe.json python tools/probe_facets.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import workloads as W

D, V, NQ, RUNS = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), int(os.environ.get("NQ", 16384)), int(os.environ.get("RUNS", 5))
NB = int(os.environ.get("BUCKETS", 1024))


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def main():
    import torch

    progs, flags, _, _, desc = W.build("cfg2", D, V, 10, 42, NQ)
    seg = T.Segment(D, V, 10, 42)
    dev = T.Device(0)
    ix = T.Index.from_segment(dev, seg)
    d = np.arange(D + 1, dtype=np.uint64)
    values = ((((d * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(9)) % np.uint64(NB)).astype(np.uint32)
    del d
    col = T.Column(ix, values)
    print(f"segment of {D} documents and a column of {NB} values uploaded", flush=True)
    res = {"workload": desc, "docs": D, "vocab": V, "queries": NQ, "buckets": NB, "runs": RUNS}
    # ---- (a) deliver, then count on the host
    a = T.Batch(ix, progs, flags)
    a.run()  # (warm-up: code objects, the pool's first growth, the plane rows)
    a.sync()
    total = int(a.counts().sum())
    pinned = torch.empty(total + 64, dtype=torch.int32).pin_memory()
    a.docsets(out=pinned)
    flat = pinned.numpy().view(np.uint32)
    ta = {"run_sync_ms": [], "deliver_ms": [], "bincount_ms": []}
    rows_a = None
    for _ in range(RUNS):
        _, t = timed(lambda: (a.run(), a.sync()))
        ta["run_sync_ms"].append(t)
        (_, offs), t = timed(lambda: a.docsets(out=pinned))
        ta["deliver_ms"].append(t)

        def count():
            out = np.zeros((NQ, NB + 1), dtype=np.uint32)
            for q in range(NQ):
                out[q] = np.bincount(np.minimum(values[flat[int(offs[q]) : int(offs[q + 1])]], NB), minlength=NB + 1)
            return out

        rows_a, t = timed(count)
        ta["bincount_ms"].append(t)
        print(f"  (a) run {len(ta['bincount_ms'])}: {ta['run_sync_ms'][-1]:.2f} + {ta['deliver_ms'][-1]:.2f} + {ta['bincount_ms'][-1]:.1f} ms", flush=True)
    info = a.info()
    res.update(matches=int(info["matches"]), docid_bytes=total * 4, kernels_ms_without_facets=float(info["last_run_ms"]), launches_without_facets=int(info["launches"]))
    a.close()
    del pinned, flat
    # ---- (b) count on the device
    b = T.Batch(ix, progs, flags)
    b.set_facets([(col, NB)])
    b.run()
    b.sync()
    b.facets(0)
    tb = {"run_sync_ms": [], "facets_ms": [], "facet_last_us": [], "kernels_ms": []}
    rows_b = None
    for _ in range(RUNS):
        _, t = timed(lambda: (b.run(), b.sync()))
        tb["run_sync_ms"].append(t)
        rows_b, t = timed(lambda: b.facets(0))
        tb["facets_ms"].append(t)
        tb["facet_last_us"].append(int(dev.get_option("facet_last_us")))
        tb["kernels_ms"].append(float(b.info()["last_run_ms"]))
    res["launches_with_facets"] = int(b.info()["launches"])
    b.close()
    assert np.array_equal(rows_a, rows_b), "the device's rows differ from numpy's"
    assert int(rows_b.sum(dtype=np.uint64)) == res["matches"]
    res.update(rows_equal=True, row_bytes_to_host=int(rows_b.nbytes), a={k: spread(v) for k, v in ta.items()}, b={k: spread(v) for k, v in tb.items()},
               wall_a_ms=spread([x + y + z for x, y, z in zip(ta["run_sync_ms"], ta["deliver_ms"], ta["bincount_ms"])]),
               wall_b_ms=spread([x + y for x, y in zip(tb["run_sync_ms"], tb["facets_ms"])]))
    res["delivery_floor_GBps"] = res["docid_bytes"] / (res["a"]["deliver_ms"]["median"] * 1e-3) / 1e9
    res["device_beats_delivery_floor"] = bool(res["wall_b_ms"]["max"] < res["a"]["deliver_ms"]["min"])
    print(f"{desc}; D = {D}, {NQ} queries, {res['matches']} matches, a column of {NB} buckets")
    print(f"  (a) deliver + numpy : wall {res['wall_a_ms']['min']:.2f} .. {res['wall_a_ms']['max']:.2f} ms = run+sync {res['a']['run_sync_ms']['median']:.2f} + docsets {res['a']['deliver_ms']['median']:.2f} "
          f"({res['docid_bytes']} bytes, {res['delivery_floor_GBps']:.1f} GB/s) + bincount {res['a']['bincount_ms']['median']:.1f}")
    print(f"  (b) facets on device: wall {res['wall_b_ms']['min']:.2f} .. {res['wall_b_ms']['max']:.2f} ms = run+sync {res['b']['run_sync_ms']['median']:.2f} + facets() {res['b']['facets_ms']['median']:.2f} "
          f"({res['row_bytes_to_host']} bytes); zeroing + k_facet {res['b']['facet_last_us']['min']} .. {res['b']['facet_last_us']['max']} us of the step's kernels' "
          f"{res['b']['kernels_ms']['median']:.2f} ms ({res['kernels_ms_without_facets']:.2f} ms without facets)")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    col.close()
    ix.close()
    dev.close()


if __name__ == "__main__":
    main()
