"""The C-ABI of Trinity::intersect on the device (CPU: no device is touched): the tri_isect_* entry points are exported, engine.py lists and binds them, the ABI
version did not move, include/trinity_hip.h declares each with its intersect.cpp citation, and NULL arguments are refused with nothing written."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["tri_isect_run", "tri_isect_status", "tri_isect_results", "tri_isect_histogram", "tri_isect_get_info", "tri_isect_destroy"]


@pytest.fixture(scope="module")
def L():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd.engine.hip_lib()


def test_the_exports_resolve_and_the_version_stays(L):
    import trinity_amd

    for name in EXPORTS:
        assert getattr(L, name) is not None, name
        assert name in trinity_amd.engine.ABI_SYMBOLS, name
    assert L.tri_abi_version() == 9


def test_the_header_declares_them_and_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "trinity_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b(?:int|void)\s+%s\s*\(" % name, text), name
    block = text[text.index("token-set co-occurrence") : text.index("tri_isect_destroy(tri_isect *);")]
    assert "intersect.cpp:5-170" in block and "intersect.h:15-18" in block and "indexPrev" in block
    for name in ("tri_isect_run", "tri_isect_status", "tri_isect_results", "tri_isect_histogram", "tri_isect_get_info"):
        assert re.search(r"^ \* %s\b" % name, block, re.M), name


def test_the_structs_match_the_binding():
    import trinity_amd.engine as E

    assert C.sizeof(E.TriIsectRequest) == 16 and E.TriIsectRequest.stopwords_mask.offset == 8
    assert E.TriIsectInfo.row_bytes.offset == 32 and E.TriIsectInfo.h_size.offset == 48 and C.sizeof(E.TriIsectInfo) == 72


def test_null_arguments_are_refused(L):
    n = C.c_size_t(77)
    buf = (C.c_uint64 * 4)()
    out = C.c_void_p(5)
    assert L.tri_isect_run(None, buf, 1, buf, buf, C.byref(out)) == -1 and b"tri_isect_run: null argument" in L.tri_last_error()  # TRI_ERR_INVALID
    assert out.value == 5
    assert L.tri_isect_status(None, buf) == -1 and b"tri_isect_status" in L.tri_last_error()
    assert L.tri_isect_results(None, 0, buf, buf, 4, C.byref(n)) == -1 and b"tri_isect_results" in L.tri_last_error()
    assert L.tri_isect_histogram(None, 0, buf, buf, buf, 4, C.byref(n)) == -1 and b"tri_isect_histogram" in L.tri_last_error()
    assert L.tri_isect_get_info(None, None) == -1 and b"tri_isect_get_info" in L.tri_last_error()
    L.tri_isect_destroy(None)
    assert n.value == 77 and not any(buf)


def test_the_options_exist_and_the_binding_has_the_methods():
    import trinity_amd

    text = open(os.path.join(ROOT, "trinity_amd", "csrc", "trinity_hip.hip")).read()
    for name in ("isect_max_bytes", "isect_max_masks", "isect_max_runs"):
        assert '{"%s", &tri_options::%s}' % (name, name) in text
    assert callable(trinity_amd.Index.intersect)
    for name in ("status", "results", "histogram", "info", "close"):
        assert callable(getattr(trinity_amd.engine.Intersection, name))
