"""CPU tests of the surface of ordering by a column (include/trinity_hip.h: tri_batch_set_order / tri_batch_ordered / tri_cbatch_ordered): the symbols are declared,
exported by the built library and bound in engine.py with the header's signatures; the limit agrees between the header, the binding and the kernels' constants
(TRI_ORDER_MAX_TOPK == TOPK_MAX); every export's header comment cites the reference's consumer (exec.h:12-23); the calls refuse null handles without a device.  No GPU
compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import structured as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tri_batch_set_order", "tri_batch_ordered", "tri_cbatch_ordered"]
TRI_ERR_INVALID = -1
SIGNATURES = {
    "tri_batch_set_order": ("int", ["tri_batch *", "const tri_order *spec"]),
    "tri_batch_ordered": ("int", ["tri_batch *", "uint32_t *docids", "uint32_t *values", "uint32_t *counts"]),
    "tri_cbatch_ordered": ("int", ["tri_cbatch *", "uint32_t *docids", "uint32_t *values", "uint32_t *counts"]),
}


@pytest.fixture(scope="module")
def L():
    import trinity_amd
    from trinity_amd.engine import hip_lib

    trinity_amd.build_all()
    return hip_lib()


def raw_header():
    return open(os.path.join(ROOT, "include", "trinity_hip.h")).read()


def header():
    return re.sub(r"/\*.*?\*/", "", raw_header(), flags=re.S)


def test_the_calls_are_declared_exported_and_bound_with_the_headers_signatures(L):
    from trinity_amd.engine import ABI_SYMBOLS

    src = header()
    for n in NAMES:
        m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(2).split(",")]
        assert (m.group(1), params) == SIGNATURES[n], (n, m.group(1), params)
        assert n in ABI_SYMBOLS, n
        fn = getattr(L, n)
        assert len(fn.argtypes) == len(params), n
        for p, a in zip(params, fn.argtypes):
            assert "*" in p and (a is C.c_void_p or issubclass(a, C._Pointer)), (n, p, a)
        assert fn.restype is C.c_int, n
    assert re.search(r"typedef\s+struct\s+tri_order\s*\{\s*tri_column\s*\*column;\s*uint32_t\s+topk;\s*uint32_t\s+descending;\s*uint32_t\s+reserved;\s*\}\s*tri_order\s*;", src)
    assert L.tri_abi_version() == 9  # (additions within 9)


def test_every_exports_comment_cites_the_references_consumer():
    raw = raw_header()
    for n in NAMES:
        assert re.search(r"\* %s \(exec\.h:12-23\)" % n, raw), n
    assert "order_last_us" in raw


def test_the_limit_agrees_between_header_binding_and_kernels():
    import trinity_amd as T
    from trinity_amd.engine import TriOrder

    kmax = int(re.search(r"#define\s+TRI_ORDER_MAX_TOPK\s+(\d+)\b", header()).group(1))
    k = S.header_constants("dev_structs.hpp")
    assert kmax == T.ORDER_MAX_TOPK == k["ORDER_MAX_TOPK"] == k["TOPK_MAX"] == S.TOPK_MAX == 256
    assert k["ORDER_BUF"] == k["ORDER_PRUNE_AT"] + k["ORDER_TILE"] and k["ORDER_PRUNE_AT"] >= k["ORDER_MAX_TOPK"] and k["ORDER_TILE"] == 64 and k["ORDER_WG"] == 64 * k["ORDER_WAVES"]
    assert k["ORDER_WAVES"] * k["ORDER_BUF"] * 8 <= 16 * 1024  # (a workgroup's LDS: nine workgroups a CU keep theirs, the registers allow eight — they decide the occupancy)
    assert 2 <= k["ORDER_FANIN"] <= 64
    assert C.sizeof(TriOrder) == 24 and TriOrder.topk.offset == 8 and TriOrder.descending.offset == 12 and TriOrder.reserved.offset == 16
    assert callable(T.Batch.set_order) and callable(T.Batch.clear_order) and callable(T.Batch.ordered) and callable(T.CollectionBatch.ordered)


def test_null_handles_are_refused_without_a_device(L):
    from trinity_amd.engine import TriOrder

    out = np.zeros(4, dtype=np.uint32)
    spec = TriOrder(None, 10, 0, 0)
    p = out.ctypes.data
    for call, name in ((lambda: L.tri_batch_set_order(None, C.byref(spec)), b"tri_batch_set_order"), (lambda: L.tri_batch_set_order(None, None), b"tri_batch_set_order"),
                       (lambda: L.tri_batch_ordered(None, p, p, p), b"tri_batch_ordered"), (lambda: L.tri_cbatch_ordered(None, p, p, p), b"tri_cbatch_ordered")):  # fmt: skip
        assert call() == TRI_ERR_INVALID and name in L.tri_last_error(), name
    assert not out.any()
