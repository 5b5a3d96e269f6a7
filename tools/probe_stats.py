#!/usr/bin/env python3
"""Perf probe (GPU): what aggregating a column on the device saves (tri_batch_set_stats, csrc/k_stats.hpp).  The cfg2 workload — NQ two-term conjunctions (Zipf terms,
query seed 1337) over the L corpus, DocumentsOnly — with a value column `hash` (a multiplicative hash of the docID: 32 random bits, no locality for the gather to lean
on).  Five legs:
  (1) what the engine offered before: run + sync, tri_batch_docsets into pinned host memory, a numpy reduction per query (count, sum, min, max of hash).  The delivery
      alone is reported too: the floor of ANY host approach;
  (2) on the device, one ungrouped stat over hash (the register regime);
  (3) one grouped stat: a group column of BUCKETS hashed values, the value column hash.  At the default 1024 buckets the row has 1025 records, more than
      STATS_LDS_BUCKETS: the DIRECT regime, four global atomics per match;
  (4) the same with the group column `one` (two records: the ON-CHIP regime) — every document of a task on ONE LDS record: the worst contention there is;
  (5) beside the issue's four: the group column of leg 3 folded to CHIP_BUCKETS (512) values — the on-chip regime with the buckets spread, the leg to hold leg 4
      against.
Reports, per leg, the host clock around work that ends in a device synchronise (all RUNS, after one warm-up of each shape), and for the device legs the step's kernels
and the device time of the rows' initialisation + k_stats (HIP events: option stats_last_us).  Every device leg's rows are compared with numpy's, integer for integer,
before any time is reported.   NQ=16384 DOCS=10000000 VOCAB=1000000 BUCKETS=1024 RUNS=5 OUT=profiles/stats_probe.json python tools/probe_stats.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import workloads as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import structured  # noqa: E402  (header_constants: the kernel's thresholds as dev_structs.hpp names them)

S_CONST = structured.header_constants("dev_structs.hpp")

D, V, NQ, RUNS = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000)), int(os.environ.get("NQ", 16384)), int(os.environ.get("RUNS", 5))
NB = int(os.environ.get("BUCKETS", 1024))
NB_CHIP = int(os.environ.get("CHIP_BUCKETS", 512))
HUGE = 0xFFFFFFFF


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def reduce_per_query(flat, offs, value):
    """Leg 1's host work: per query the count, sum, min and max of value over its docID set."""
    out = T.Stats(np.zeros((NQ, 1), np.uint64), np.zeros((NQ, 1), np.uint32), np.full((NQ, 1), HUGE, np.uint32), np.zeros((NQ, 1), np.uint32))
    for q in range(NQ):
        a, b = int(offs[q]), int(offs[q + 1])
        if a == b:
            continue
        v = value[flat[a:b]]
        out.counts[q, 0], out.sums[q, 0], out.mins[q, 0], out.maxs[q, 0] = b - a, v.sum(dtype=np.uint64), v.min(), v.max()
    return out


def grouped_reference(flat, offs, group, nb, value, chunk=512):
    """numpy's rows of a grouped stat, a chunk of queries at a time (untimed: the yardstick of legs 3 and 4)."""
    w = nb + 1
    out = T.Stats(np.zeros((NQ, w), np.uint64), np.zeros((NQ, w), np.uint32), np.full((NQ, w), HUGE, np.uint32), np.zeros((NQ, w), np.uint32))
    for q0 in range(0, NQ, chunk):
        q1 = min(NQ, q0 + chunk)
        a, b = int(offs[q0]), int(offs[q1])
        docs = flat[a:b]
        lens = np.diff(offs[q0 : q1 + 1]).astype(np.int64)
        key = np.repeat(np.arange(q1 - q0, dtype=np.int64), lens) * w + np.minimum(group[docs], nb).astype(np.int64)
        v = value[docs]
        out.counts[q0:q1] = np.bincount(key, minlength=(q1 - q0) * w).reshape(q1 - q0, w)
        np.add.at(out.sums[q0:q1].reshape(-1), key, v.astype(np.uint64))
        np.minimum.at(out.mins[q0:q1].reshape(-1), key, v)
        np.maximum.at(out.maxs[q0:q1].reshape(-1), key, v)
    return out


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def main():
    import torch

    progs, flags, _, _, desc = W.build("cfg2", D, V, 10, 42, NQ)
    seg = T.Segment(D, V, 10, 42)
    dev = T.Device(0)
    ix = T.Index.from_segment(dev, seg)
    d = np.arange(D + 1, dtype=np.uint64)
    hashed = ((d * np.uint64(2654435761)) & np.uint64(HUGE)).astype(np.uint32)
    groups = ((hashed >> np.uint32(9)) % np.uint32(NB)).astype(np.uint32)
    del d
    groups_chip = (groups % np.uint32(NB_CHIP)).astype(np.uint32)
    cols = {"hash": T.Column(ix, hashed), "group": T.Column(ix, groups), "group_chip": T.Column(ix, groups_chip), "one": T.Column(ix, np.zeros(D + 1, np.uint32))}
    print(f"segment of {D} documents and four columns uploaded", flush=True)
    lds = S_CONST["STATS_LDS_BUCKETS"]
    res = {"workload": desc, "docs": D, "vocab": V, "queries": NQ, "buckets": NB, "chip_buckets": NB_CHIP, "runs": RUNS, "STATS_LDS_BUCKETS": lds,
           "STATS_SHORT_SEGMENT": S_CONST["STATS_SHORT_SEGMENT"]}
    # ---- (1) deliver, then reduce on the host
    a = T.Batch(ix, progs, flags)
    a.run()  # (warm-up: code objects, the pool's first growth, the plane rows)
    a.sync()
    total = int(a.counts().sum())
    pinned = torch.empty(total + 64, dtype=torch.int32).pin_memory()
    a.docsets(out=pinned)
    flat = pinned.numpy().view(np.uint32)
    t1 = {"run_sync_ms": [], "deliver_ms": [], "reduce_ms": []}
    want_ungrouped = offs = None
    for _ in range(RUNS):
        _, t = timed(lambda: (a.run(), a.sync()))
        t1["run_sync_ms"].append(t)
        (_, offs), t = timed(lambda: a.docsets(out=pinned))
        t1["deliver_ms"].append(t)
        want_ungrouped, t = timed(lambda: reduce_per_query(flat, offs, hashed))
        t1["reduce_ms"].append(t)
        print(f"  (1) run {len(t1['reduce_ms'])}: {t1['run_sync_ms'][-1]:.2f} + {t1['deliver_ms'][-1]:.2f} + {t1['reduce_ms'][-1]:.1f} ms", flush=True)
    info = a.info()
    res.update(matches=int(info["matches"]), docid_bytes=total * 4, kernels_ms_without_stats=float(info["last_run_ms"]), launches_without_stats=int(info["launches"]))
    a.close()
    assert int(want_ungrouped.counts.sum(dtype=np.uint64)) == res["matches"]
    want_grouped = grouped_reference(flat, offs, groups, NB, hashed)
    assert np.array_equal(want_grouped.sums.sum(axis=1), want_ungrouped.sums[:, 0]) and np.array_equal(want_grouped.mins.min(axis=1), want_ungrouped.mins[:, 0])
    want_chip = grouped_reference(flat, offs, groups_chip, NB_CHIP, hashed)
    empty = T.Stats(np.zeros((NQ, 1), np.uint64), np.zeros((NQ, 1), np.uint32), np.full((NQ, 1), HUGE, np.uint32), np.zeros((NQ, 1), np.uint32))
    want_one = T.Stats(*(np.concatenate([x, e], axis=1) for x, e in zip(want_ungrouped, empty)))  # (every document in bucket 0; the overflow bucket stays empty)
    del pinned, flat
    print("numpy's rows of the four device legs stand", flush=True)
    res["a"] = {k: spread(v) for k, v in t1.items()}
    res["wall_a_ms"] = spread([x + y + z for x, y, z in zip(t1["run_sync_ms"], t1["deliver_ms"], t1["reduce_ms"])])
    res["delivery_floor_GBps"] = res["docid_bytes"] / (res["a"]["deliver_ms"]["median"] * 1e-3) / 1e9
    # ---- (2) .. (4) on the device
    legs = [("ungrouped_hash", (None, 0, cols["hash"]), want_ungrouped), ("grouped_%d_hash" % NB, (cols["group"], NB, cols["hash"]), want_grouped),
            ("grouped_one_hash", (cols["one"], 1, cols["hash"]), want_one), ("grouped_%d_hash" % NB_CHIP, (cols["group_chip"], NB_CHIP, cols["hash"]), want_chip)]  # fmt: skip
    res["legs"] = {}
    for name, spec, want in legs:
        b = T.Batch(ix, progs, flags)
        b.set_stats([spec])
        b.run()
        b.sync()
        b.stats(0)
        tb = {"run_sync_ms": [], "stats_ms": [], "stats_last_us": [], "kernels_ms": []}
        rows = None
        for _ in range(RUNS):
            _, t = timed(lambda: (b.run(), b.sync()))
            tb["run_sync_ms"].append(t)
            rows, t = timed(lambda: b.stats(0))
            tb["stats_ms"].append(t)
            tb["stats_last_us"].append(int(dev.get_option("stats_last_us")))
            tb["kernels_ms"].append(float(b.info()["last_run_ms"]))
        launches = int(b.info()["launches"])
        b.close()
        assert same(rows, want), f"{name}: the device's rows differ from numpy's"
        leg = {k: spread(v) for k, v in tb.items()}
        records = spec[1] + 1 if spec[0] is not None else 0
        leg.update(regime="registers" if spec[0] is None else "on chip (segments of STATS_SHORT_SEGMENT matches and more)" if records <= lds else "direct", lds_records=records,
                   rows_equal=True, launches=launches, row_bytes_to_host=int(sum(x.nbytes for x in rows)),
                   wall_ms=spread([x + y for x, y in zip(tb["run_sync_ms"], tb["stats_ms"])]))
        leg["beats_delivery_floor"] = bool(leg["wall_ms"]["max"] < res["a"]["deliver_ms"]["min"])
        res["legs"][name] = leg
        print(f"  {name} [{leg['regime']}]: rows equal numpy's; wall {leg['wall_ms']['min']:.2f} .. {leg['wall_ms']['max']:.2f} ms = run+sync {leg['run_sync_ms']['median']:.2f} + stats() "
              f"{leg['stats_ms']['median']:.2f} ({leg['row_bytes_to_host']} bytes); initialisation + k_stats {leg['stats_last_us']['min']} .. {leg['stats_last_us']['max']} us of the "
              f"step's kernels' {leg['kernels_ms']['median']:.2f} ms", flush=True)
    print(f"{desc}; D = {D}, {NQ} queries, {res['matches']} matches")
    print(f"  (1) deliver + numpy : wall {res['wall_a_ms']['min']:.2f} .. {res['wall_a_ms']['max']:.2f} ms = run+sync {res['a']['run_sync_ms']['median']:.2f} + docsets "
          f"{res['a']['deliver_ms']['median']:.2f} ({res['docid_bytes']} bytes, {res['delivery_floor_GBps']:.1f} GB/s) + reduction {res['a']['reduce_ms']['median']:.1f}; "
          f"the step's kernels without stats {res['kernels_ms_without_stats']:.2f} ms")
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for c in cols.values():
        c.close()
    ix.close()
    dev.close()


if __name__ == "__main__":
    main()
