"""The per-query document filters and queries that tests/test_filters_abi.py (CPU: the oracle's side of the top-K comparison rule) and tests/test_gpu_filters.py (the
engine) share.  A filter here is (docids, keep): the C-ABI's pair — docids dropped (TRI_FILTER_DROP), or the only documents a query may match (TRI_FILTER_KEEP)."""
import numpy as np

import structured as S

K = 10  # the top-K the filtered batches are scored at


def around(points, D):
    """{p - 1, p, p + 1} for every point, inside 1 .. D."""
    d = np.unique(np.concatenate([np.asarray(points, dtype=np.int64) + x for x in (-1, 0, 1)]))
    return d[(d >= 1) & (d <= D)].astype(np.uint32)


def stream_filters(D=S.D_STREAM):
    """name -> (docids, keep) over the stream corpus (three SPAN_BITS windows):
    span     drops 1, D and k * SPAN_BITS + {-1, 0, 1}: the documents on the bitmap windows' edges (every list of the corpus holds them);
    windows  drops the same offsets around the multiples of PL_W and FUS_W (k_planes' and k_fused's windows; 2 FUS_W is k_fused's 16-bit window);
    one      keeps ONE document per SPAN_BITS window (documents every head list holds);
    all      drops every document: every count 0, every top-K empty;
    empty    drops nothing (n = 0): equal to no filter."""
    span = np.unique(np.concatenate([[1, D], around([k * S.SPAN_BITS for k in range(1, D // S.SPAN_BITS + 1)], D)])).astype(np.uint32)
    mult = [k * w for w in (S.PL_W, S.FUS_W) for k in range(1, D // w + 1)]
    return {
        "span": (span, False),
        "windows": (around(mult, D), False),
        "one": (np.array([S.SPAN_BITS - 1, S.SPAN_BITS + 1, D], dtype=np.uint32), True),
        "all": (np.arange(1, D + 1, dtype=np.uint32), False),
        "empty": (np.zeros(0, dtype=np.uint32), False),
    }


def dropped(flt, D):
    """The documents of 1 .. D a (docids, keep) filter drops, ascending."""
    ids, keep = flt
    ids = np.unique(ids[(ids >= 1) & (ids <= D)])
    return np.setdiff1d(np.arange(1, D + 1, dtype=np.uint32), ids, assume_unique=True).astype(np.uint32) if keep else ids.astype(np.uint32)


# a tree over nine terms (more than a truth table holds: TASK_TREE), a phrase under an OR (a hidden phrase query feeds the tree: the phrase of the two rarest heads
# with written positions — k_phrase's time goes with the phrase's candidates), a rare lead against head terms (k_probe when probe_max_blocks allows), unions with
# rare terms (k_psets' scatter)
STREAM_EXTRA = [
    "{h0} OR ({h1} {h2}) OR ({h3} {h4}) OR ({h5} {h6}) OR ({h7} {h8})",
    '{h6} OR "{h4} {h5}"',
    "{r2} {h0} {h1}",
    "{r1} {h3}",
    "{h0} OR {h1} OR {r2}",
    "{h2} OR {r0} OR {r1}",
]


def stream_queries(c):
    """(text, some_min) pairs: the stream corpus' docs-only shapes (ANDs, unions, CNFs, head terms with rare ones) over every other head term — document
    frequencies D / 2 .. D / 157 — and STREAM_EXTRA."""
    return S.stream_docs_queries(c, S.STREAM_HEADS[::2]) + [(c.q(t), 1) for t in STREAM_EXTRA]
