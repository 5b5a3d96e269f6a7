#!/usr/bin/env python3
"""Perf probe (GPU): what ordering by a column on the device saves (tri_batch_set_order, csrc/k_order.hpp).  The cfg2 workload — NQ two-term conjunctions (Zipf terms,
query seed 1337) over the L corpus, DocumentsOnly — with one column (a multiplicative hash of the docID: no locality for the gather to lean on), K = 10 and 256, both
directions, two ways to the same [NQ, K] rows:
  (a) what the engine offered before: run + sync, tri_batch_docsets into pinned host memory, numpy.lexsort per query.  The delivery alone is reported too: the floor of
      ANY host approach.  The sort's cost does not depend on the direction or on K (the whole set is sorted, then cut): it is timed ascending, RUNS times, and run once
      more descending for the comparison;
  (b) set_order + run + sync + ordered(), RUNS times per (K, direction) after one warm-up of each.
Reports, per path, the host clock around work that ends in a device synchronise, the step without an order next to the step with one, the device time of k_order and
its merge (HIP events: option order_last_us) and, for scale, of k_facet with one 1024-bucket facet on the same column (option facet_last_us).  The two paths' rows are
compared, integer for integer, before any time is reported.   NQ=16384 DOCS=10000000 VOCAB=1000000 RUNS=5 OUT=profiles/order_probe.json python tools/probe_order.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import workloads as W

D, V, NQ, RUNS = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), int(os.environ.get("NQ", 16384)), int(os.environ.get("RUNS", 5))
KS = (10, 256)


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
    values = ((d * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    del d
    col = T.Column(ix, values)
    print(f"segment of {D} documents and a hashed column uploaded", flush=True)
    res = {"workload": desc, "docs": D, "vocab": V, "queries": NQ, "ks": list(KS), "runs": RUNS}
    # ---- (a) deliver, then sort on the host
    a = T.Batch(ix, progs, flags)
    a.run()  # (warm-up: code objects, the pool's first growth, the plane rows)
    a.sync()
    total = int(a.counts().sum())
    pinned = torch.empty(total + 64, dtype=torch.int32).pin_memory()
    a.docsets(out=pinned)
    flat = pinned.numpy().view(np.uint32)
    kmax = max(KS)

    def sort_rows(offs, descending):
        docs_out, n_out = np.zeros((NQ, kmax), dtype=np.uint32), np.zeros(NQ, dtype=np.uint32)
        for q in range(NQ):
            ids = flat[int(offs[q]) : int(offs[q + 1])]
            v = values[ids].astype(np.int64)
            first = ids[np.lexsort((ids, -v if descending else v))[:kmax]]
            docs_out[q, : first.size], n_out[q] = first, first.size
        return docs_out, n_out

    ta = {"run_sync_ms": [], "deliver_ms": [], "lexsort_ms": []}
    want = {}
    for _ in range(RUNS):
        _, t = timed(lambda: (a.run(), a.sync()))
        ta["run_sync_ms"].append(t)
        (_, offs), t = timed(lambda: a.docsets(out=pinned))
        ta["deliver_ms"].append(t)
        want[False], t = timed(lambda: sort_rows(offs, False))
        ta["lexsort_ms"].append(t)
        print(f"  (a) run {len(ta['lexsort_ms'])}: {ta['run_sync_ms'][-1]:.2f} + {ta['deliver_ms'][-1]:.2f} + {ta['lexsort_ms'][-1]:.1f} ms", flush=True)
    want[True] = sort_rows(offs, True)
    print("  (a) descending rows sorted once more for the comparison", flush=True)
    info = a.info()
    res.update(matches=int(info["matches"]), docid_bytes=total * 4, kernels_ms_without_order=float(info["last_run_ms"]), launches_without_order=int(info["launches"]))
    a.close()
    del pinned, flat
    # ---- (b) select on the device
    b = T.Batch(ix, progs, flags)
    res["b"] = {}
    worst = 0.0
    for k in KS:
        for descending in (False, True):
            b.set_order(col, k, descending)
            b.run()
            b.sync()
            b.ordered()
            tb = {"run_sync_ms": [], "ordered_ms": [], "order_last_us": [], "kernels_ms": []}
            got = None
            for _ in range(RUNS):
                _, t = timed(lambda: (b.run(), b.sync()))
                tb["run_sync_ms"].append(t)
                got, t = timed(lambda: b.ordered())
                tb["ordered_ms"].append(t)
                tb["order_last_us"].append(int(dev.get_option("order_last_us")))
                tb["kernels_ms"].append(float(b.info()["last_run_ms"]))
            docs_w, n_w = want[descending]
            n_k = np.minimum(n_w, k)
            live = np.arange(k)[None, :] < n_k[:, None]
            assert np.array_equal(got[2], n_k), "the device's counts differ from numpy's"
            assert np.array_equal(got[0], np.where(live, docs_w[:, :k], 0)), "the device's docIDs differ from numpy's"
            assert np.array_equal(got[1], np.where(live, values[got[0]], 0)), "the device's values are not the column's"
            wall = [x + y for x, y in zip(tb["run_sync_ms"], tb["ordered_ms"])]
            worst = max(worst, max(wall))
            key = f"k{k}_{'down' if descending else 'up'}"
            res["b"][key] = dict({n: spread(v) for n, v in tb.items()}, wall_ms=spread(wall), row_bytes_to_host=int(NQ * (k * 8 + 4)), launches=int(b.info()["launches"]))
            print(f"  (b) {key}: wall {min(wall):.2f} .. {max(wall):.2f} ms, k_order + merge {min(tb['order_last_us'])} .. {max(tb['order_last_us'])} us", flush=True)
    # ---- for scale: one facet on the same column (the gather alone, and 1025 counters a query)
    b.clear_order()
    b.set_facets([(col, 1024)])
    b.run()
    b.sync()
    fus = []
    for _ in range(RUNS):
        b.run()
        b.sync()
        fus.append(int(dev.get_option("facet_last_us")))
    b.close()
    res.update(rows_equal=True, a={n: spread(v) for n, v in ta.items()}, facet_last_us=spread(fus),
               wall_a_ms=spread([x + y + z for x, y, z in zip(ta["run_sync_ms"], ta["deliver_ms"], ta["lexsort_ms"])]))
    res["delivery_floor_GBps"] = res["docid_bytes"] / (res["a"]["deliver_ms"]["median"] * 1e-3) / 1e9
    res["device_worst_wall_ms"] = worst
    res["device_beats_delivery_floor_in_every_run"] = bool(worst < res["a"]["deliver_ms"]["min"])
    print(f"{desc}; D = {D}, {NQ} queries, {res['matches']} matches")
    print(f"  (a) deliver + lexsort: wall {res['wall_a_ms']['min']:.1f} .. {res['wall_a_ms']['max']:.1f} ms = run+sync {res['a']['run_sync_ms']['median']:.2f} + docsets "
          f"{res['a']['deliver_ms']['min']:.2f} .. {res['a']['deliver_ms']['max']:.2f} ({res['docid_bytes']} bytes, {res['delivery_floor_GBps']:.1f} GB/s) + lexsort {res['a']['lexsort_ms']['median']:.0f}")
    print(f"  (b) ordered on device: worst wall of all runs {worst:.2f} ms; below the delivery leg alone in every run: {res['device_beats_delivery_floor_in_every_run']}; "
          f"matching alone {res['kernels_ms_without_order']:.2f} ms, k_facet (1024 buckets) {res['facet_last_us']['min']} .. {res['facet_last_us']['max']} us")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    col.close()
    ix.close()
    dev.close()


if __name__ == "__main__":
    main()
