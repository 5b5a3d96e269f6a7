"""The C-ABI of the default mode over a collection (CPU: no device is touched): tri_cbatch_ranked, tri_cbatch_matched_terms[_wide], tri_cbatch_matched_payloads and
the Python binding's CollectionBatch methods exist, the ABI version did not move, and NULL arguments are refused."""
import ctypes as C

import pytest

EXPORTS = ["tri_cbatch_ranked", "tri_cbatch_matched_terms", "tri_cbatch_matched_terms_wide", "tri_cbatch_matched_payloads", "tri_cbatch_docset"]


@pytest.fixture(scope="module")
def L():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd.engine.hip_lib()


def test_the_exports_resolve_and_the_version_stays(L):
    for name in EXPORTS:
        assert getattr(L, name) is not None, name
    assert L.tri_abi_version() == 9


def test_null_arguments_are_refused(L):
    n = C.c_size_t(77)
    buf = (C.c_uint64 * 4)()
    assert L.tri_cbatch_ranked(None, buf, buf, buf) == -1 and b"null argument" in L.tri_last_error()  # TRI_ERR_INVALID
    assert L.tri_cbatch_matched_terms(None, 0, None, None, None, 0, C.byref(n)) == -1 and b"tri_cbatch_matched_terms" in L.tri_last_error()
    assert L.tri_cbatch_matched_terms_wide(None, 0, None, None, None, 0, C.byref(n)) == -1 and b"tri_cbatch_matched_terms_wide" in L.tri_last_error()
    assert L.tri_cbatch_matched_payloads(None, 0, None, None, 0, C.byref(n)) == -1 and b"tri_cbatch_matched_payloads" in L.tri_last_error()
    assert n.value == 77 and not any(buf)


def test_the_binding_has_the_methods():
    import trinity_amd

    for name in ("ranked", "matched_terms", "matched_terms_wide", "matched_payloads"):
        assert callable(getattr(trinity_amd.CollectionBatch, name))
