#!/usr/bin/env python3
"""Perf probe (GPU): Trinity::intersect on the device (tri_isect_run; csrc/k_isect.hpp) on the cfg2 segment — requests of 2, 4, 8 and 16 Zipf tokens (one term a
token, query seed 1337, distinct within a request), one request a call, timed END TO END around the call (host wall clock: the row build, both passes, the
read-backs and the replay; the call is synchronous).  Beside it the same answer on the host from tri_decode_terms' lists: the decode call (device decode + the
copy of the lists to the host) and a k-way merge with the reference's shape — a linear scan over the open lists per document, the antichain with its shortcut —
in one host thread (tools/isect_host_merge.cpp, compiled by the probe).  Every request's two answers are compared.  Per token count: the median over the requests
of each request's median over RUNS timed calls after WARMUP untimed ones, and the spread (min .. max over the requests' medians).
   DOCS=10000000 VOCAB=1000000 REQUESTS=8 RUNS=5 WARMUP=2 python tools/probe_isect.py        -> profiles/isect_probe.json"""
import ctypes as C
import json
import os
import platform
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import trinity_amd as T
from trinity_amd import engine as E

D, V = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("VOCAB", 1_000_000))
NREQ, RUNS, WARMUP = int(os.environ.get("REQUESTS", 8)), int(os.environ.get("RUNS", 5)), int(os.environ.get("WARMUP", 2))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "isect_probe.json"))


def timed(call):
    for _ in range(WARMUP):
        call()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), r


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def host_merge_lib():
    """tools/isect_host_merge.cpp compiled into build/ (the probe's own baseline; no library of the product holds it)"""
    src, out = os.path.join(ROOT, "tools", "isect_host_merge.cpp"), os.path.join(ROOT, "build", "libisect_host_merge.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-o", out, src], check=True)
    return C.CDLL(out)


H = host_merge_lib()
H.tri_host_isect_merge.restype = C.c_uint64
H.tri_host_isect_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]

t0 = time.perf_counter()
seg = T.Segment(D, V, 10, 42)
dev = T.Device(0)
ix = T.Index.from_segment(dev, seg)
print(f"segment: {D} documents, {V} terms, google_codec ({time.perf_counter() - t0:.1f} s to build and upload)", flush=True)
result = {"workload": f"cfg2 segment: {D} documents, {V} terms, google_codec, corpus seed 42; requests of k Zipf tokens (seed 1337), one request a call",
          "method": f"wall clock around the call; per request the median of {RUNS} calls after {WARMUP} warm-up calls; per k the median, min and max over {NREQ} requests",
          "host": {"cpu": cpu_name(), "threads_used": 1, "cpus_visible": os.cpu_count()}, "by_tokens": {}}  # fmt: skip
for k in (2, 4, 8, 16):
    rows = [r.tolist() for r in E.gen_queries(V, 1337 + k, NREQ, k)]
    dev_ms, dec_ms, merge_ms, postings, entries, passes, hs, cs = [], [], [], [], [], [], [], []
    for row in rows:
        req = [([[t] for t in row], 0)]

        def run_dev():
            x = ix.intersect(req)
            out = x.results(0), x.info()
            x.close()
            return out

        ms, (got, info) = timed(run_dev)
        dev_ms.append(ms)
        passes.append(info["passes"])
        hs.append(info["h_size"][0])
        cs.append(info["c_size"][0])
        df = seg.terms[row, 0].astype(np.int64)
        ms, (docs, _, offs) = timed(lambda: ix.decode_terms(row, df, want_freqs=False))
        dec_ms.append(ms)
        known = [i for i in range(k) if df[i]]
        orig = sum(1 << i for i in known) if len(known) == k else 0
        grp = np.arange(k, dtype=np.uint8)
        m, c = np.zeros(1 << 16, dtype=np.uint64), np.zeros(1 << 16, dtype=np.uint32)
        ms, n = timed(lambda: H.tri_host_isect_merge(docs.ctypes.data, offs.ctypes.data, grp.ctypes.data, k, orig, 0, None, m.ctypes.data, c.ctypes.data, m.size))
        merge_ms.append(ms)
        assert n <= m.size and got == list(zip(m[:n].tolist(), c[:n].tolist())), (k, row)
        postings.append(int(df.sum()))
        entries.append(len(got))
    result["by_tokens"][str(k)] = {"requests": NREQ, "postings_median": int(statistics.median(postings)), "list_entries_median": int(statistics.median(entries)), "kernel_passes": sorted(set(passes)), "h_entries_max": max(hs), "c_entries_max": max(cs),
                                   "tri_isect_run": spread(dev_ms), "host_decode_terms": spread(dec_ms), "host_kway_merge": spread(merge_ms),
                                   "host_total": spread([a + b for a, b in zip(dec_ms, merge_ms)])}  # fmt: skip
    print(k, json.dumps(result["by_tokens"][str(k)]), flush=True)
ix.close()
dev.close()
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", OUT)
