#!/usr/bin/env python3
"""Perf probe (GPU): the codec seam's two whole-list calls on the same head terms — tri_decode_terms (docIDs + frequencies) and tri_decode_hits (every document's
positions; csrc/k_decode_hits.hpp) — over the synthetic corpus, both codecs.  Times are DEVICE time between two HIP events recorded on the engine's stream around
the call (best of RUNS), so they hold the call's kernels, its copies back to the host and the host round trip between its passes (tri_decode_hits reads the totals
back before it sizes the output); the sizing call (count + scan passes only) is timed apart.  Prints the hit bytes per second the decode figure implies.
   DOCS=300000 VOCAB=30000 HEADS=16 RUNS=5 python tools/probe_decode_hits.py        (the `medium` world of the tests; DOCS=10000000 VOCAB=1000000: cfg4's index)"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trinity_amd as T
from trinity_amd import engine as E

D, V, HEADS, RUNS = int(os.environ.get("DOCS", 300_000)), int(os.environ.get("VOCAB", 30_000)), int(os.environ.get("HEADS", 16)), int(os.environ.get("RUNS", 5))
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def device_ms(stream, call):
    best = None
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    for _ in range(RUNS + 1):  # (the first run warms up)
        assert hip.hipEventRecord(e0, stream) == 0
        call()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if _:
            best = ms.value if best is None else min(best, ms.value)
    return best


def hit_bytes(seg, terms):
    """The bytes of the terms' hits as the codec stores them: GOOGLE, the chunk minus its document bytes and skiplist; LUCENE, the positions chunk in hits.data."""
    out = 0
    for t in terms:
        _, off, size = (int(x) for x in seg.terms[t])
        if seg.codec == E.CODEC_LUCENE:
            out += int(np.frombuffer(seg.index[off + 8 : off + 12].tobytes(), dtype="<u4")[0])
        else:
            out += size - 8 * int(np.frombuffer(seg.index[off : off + 2].tobytes(), dtype="<u2")[0])
    return out


dev = T.Device(0)
stream = C.c_void_p(E.hip_lib().tri_dev_stream(dev.h))
for codec, name in ((E.CODEC_GOOGLE, "GOOGLE"), (E.CODEC_LUCENE, "LUCENE")):
    seg = T.Segment(D, V, 10, 42, codec=codec)
    ix = T.Index.from_segment(dev, seg)
    heads = np.argsort(-seg.terms[:, 0].astype(np.int64), kind="stable")[:HEADS].astype(np.uint32)
    df = seg.terms[heads, 0]
    hb = hit_bytes(seg, heads.tolist())
    if codec == E.CODEC_GOOGLE:
        hb -= int(ix.term_docbytes(heads).sum())
    offs = np.zeros(HEADS + 1, dtype=np.uint64)
    docs, freqs, doffs = np.zeros(int(df.sum()), dtype=np.uint32), np.zeros(int(df.sum()), dtype=np.uint32), np.zeros(HEADS + 1, dtype=np.uint64)  # (every call into buffers touched before)
    t_terms = device_ms(stream, lambda: E.hip_lib().tri_decode_terms(ix.h, heads.ctypes.data, heads.size, docs.ctypes.data, freqs.ctypes.data, doffs.ctypes.data))
    t_size = device_ms(stream, lambda: E.hip_lib().tri_decode_hits(ix.h, heads.ctypes.data, heads.size, None, None, None, 0, offs.ctypes.data))
    nhits = int(offs[-1])
    pos, lens, words = np.zeros(nhits, dtype=np.uint16), np.zeros(nhits, dtype=np.uint8), np.zeros(nhits, dtype=np.uint64)
    t_pos = device_ms(stream, lambda: E.hip_lib().tri_decode_hits(ix.h, heads.ctypes.data, heads.size, pos.ctypes.data, None, None, nhits, offs.ctypes.data))
    t_all = device_ms(stream, lambda: E.hip_lib().tri_decode_hits(ix.h, heads.ctypes.data, heads.size, pos.ctypes.data, lens.ctypes.data, words.ctypes.data, nhits, offs.ctypes.data))
    print(f"{name}: D = {D}, the {HEADS} head terms: {int(df.sum())} postings, {nhits} hits, {hb} hit bytes")
    print(f"  tri_decode_terms (docIDs + freqs)        : {t_terms:8.3f} ms   {int(df.sum()) / t_terms / 1e6:8.2f} G postings/s")
    print(f"  tri_decode_hits, sizing call             : {t_size:8.3f} ms")
    print(f"  tri_decode_hits, positions               : {t_pos:8.3f} ms   {nhits / t_pos / 1e6:8.2f} G hits/s   {hb / t_pos / 1e6:8.2f} GB/s of hit bytes")
    print(f"  tri_decode_hits, positions + payloads    : {t_all:8.3f} ms   {nhits / t_all / 1e6:8.2f} G hits/s   {hb / t_all / 1e6:8.2f} GB/s of hit bytes")
    ix.close()
dev.close()
