#!/usr/bin/env python3
"""Perf probe (GPU): tri_decode_hits over payload-carrying postings, the same postings committed through both codecs (tri_commit_google,
tri_commit_lucene_payloads) — positions only and positions + payloads on the Lucene segment, positions + payloads on the Google segment.  A first timing of
the Lucene payload path (csrc/lucene_pay_stream.hpp: k_decode_hit_payloads behind k_decode_hits); no threshold hangs on it.  Times are DEVICE time between two
HIP events recorded on the engine's stream around the call (best of RUNS): the call's kernels, its copies back to the host and the host round trip between its
passes.  Writes one JSON object (default profiles/lpay_probe.json).
   TERMS=64 DOCS=20000 RUNS=5 python tools/probe_lpay.py [out.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import engine as E

TERMS, DOCS, RUNS = int(os.environ.get("TERMS", 64)), int(os.environ.get("DOCS", 20000)), int(os.environ.get("RUNS", 5))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lpay_probe.json")
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def device_ms(stream, call):
    best = None
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    for i in range(RUNS + 1):  # (the first run warms up)
        assert hip.hipEventRecord(e0, stream) == 0
        assert call() == 0
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if i:
            best = ms.value if best is None else min(best, ms.value)
    return best


# the session: every term in every second document on average, 1 .. 4 hits a document; within a document the non-zero payload lengths never fall, so the two
# codecs' readers answer the same (include/trinity_hip.h, tri_decode_hits) and the outputs can be compared
rng = np.random.default_rng(7)
held = rng.random((DOCS, TERMS)) < 0.5
doc_of, term_of = np.nonzero(held)
freqs = rng.integers(1, 5, size=doc_of.size).astype(np.uint32)
post_of = np.repeat(np.arange(doc_of.size), freqs)
first = np.concatenate([[0], np.cumsum(freqs)[:-1]])
rank = np.arange(post_of.size) - first[post_of]
pos = (1 + 3 * rank + rng.integers(0, 3, size=post_of.size)).astype(np.uint16)
top = rng.integers(0, 9, size=doc_of.size)  # a document's lengths: 0 .. top, rising with the hit's rank
plen = np.minimum(top[post_of], 2 * rank + (top[post_of] > 0)).astype(np.uint8)
words = rng.integers(0, 2**63, size=post_of.size, dtype=np.uint64)
words = np.where(plen >= 8, words, words & ((np.uint64(1) << (np.uint64(8) * plen.astype(np.uint64))) - np.uint64(1)))
words = np.where(plen == 0, np.uint64(0), words)
tids, docs = (term_of + 1).astype(np.uint32), (doc_of + 1).astype(np.uint32)

dev = T.Device(0)
stream = C.c_void_p(E.hip_lib().tri_dev_stream(dev.h))
gi, _, gt, _ = dev.commit_google(tids, docs, freqs, pos, plen, words)
li, lh, _, lt, _ = dev.commit_lucene(tids, docs, freqs, pos, plen, words)
gix = T.Index(dev, gi, gt, DOCS)
lix = T.Index(dev, li, lt, DOCS, codec=E.CODEC_LUCENE, hits=lh)
terms = np.arange(gt.shape[0], dtype=np.uint32)
offs = np.zeros(terms.size + 1, dtype=np.uint64)
assert E.hip_lib().tri_decode_hits(lix.h, terms.ctypes.data, terms.size, None, None, None, 0, offs.ctypes.data) == 0
nhits = int(offs[-1])
p, ln, wd = np.zeros(nhits, np.uint16), np.zeros(nhits, np.uint8), np.zeros(nhits, np.uint64)
L = E.hip_lib()
res = {"terms": int(terms.size), "documents": DOCS, "postings": int(doc_of.size), "hits": nhits, "payload_bytes": int(plen.sum()), "hits_data_bytes": int(lh.size),
       "google_index_bytes": int(gi.size), "runs": RUNS}  # fmt: skip
res["lucene_positions_ms"] = device_ms(stream, lambda: L.tri_decode_hits(lix.h, terms.ctypes.data, terms.size, p.ctypes.data, None, None, nhits, offs.ctypes.data))
res["lucene_payloads_ms"] = device_ms(stream, lambda: L.tri_decode_hits(lix.h, terms.ctypes.data, terms.size, p.ctypes.data, ln.ctypes.data, wd.ctypes.data, nhits, offs.ctypes.data))
lucene = (p.copy(), ln.copy(), wd.copy())
res["google_payloads_ms"] = device_ms(stream, lambda: L.tri_decode_hits(gix.h, terms.ctypes.data, terms.size, p.ctypes.data, ln.ctypes.data, wd.ctypes.data, nhits, offs.ctypes.data))
res["outputs_equal"] = bool(np.array_equal(lucene[0], p) and np.array_equal(lucene[1], ln) and np.array_equal(lucene[2], wd) and int(ln.sum()) == int(plen.sum()))
for k in ("lucene_positions_ms", "lucene_payloads_ms", "google_payloads_ms"):
    res[k.replace("_ms", "_ghits_per_s")] = round(nhits / res[k] / 1e6, 3)
    res[k] = round(res[k], 4)
print(json.dumps(res))
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
lix.close()
gix.close()
dev.close()
