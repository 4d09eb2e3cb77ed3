"""tfidf_search_batch_all / tfidf_reader_search_batch_all argument checks that
need no GPU: a NULL index (reader), hit_offsets or n_out is refused with
TFIDF_E_INVALID_ARG before the handle is read or any device touched (the
non-NULL handles below point at plain host bytes, never at an index)."""
import ctypes as C

import numpy as np
import pytest

from tfidf_amd import _lib as L

FUNCS = ("tfidf_search_batch_all", "tfidf_reader_search_batch_all")


def _call(name, handle, hit_offsets, n_out):
    fn = getattr(L.load(), name)
    q = b"fast food"
    offs = np.array([0, len(q)], np.uint64)
    docs = np.zeros(4, np.uint32)
    scores = np.zeros(4, np.float32)
    return fn(handle, q, L.ptr(offs, C.c_uint64), 1, L.ptr(docs, C.c_uint32), L.ptr(scores, C.c_float), 4,
              hit_offsets, n_out)


@pytest.mark.parametrize("name", FUNCS)
def test_null_arguments_are_invalid(name):
    fake = C.create_string_buffer(64)                 # stands for a handle; must never be read
    handle = C.cast(fake, C.c_void_p)
    ho = np.zeros(2, np.uint64)
    n = C.c_uint64(7)
    assert _call(name, None, L.ptr(ho, C.c_uint64), C.byref(n)) == L.E_INVALID_ARG
    assert _call(name, handle, None, C.byref(n)) == L.E_INVALID_ARG
    assert _call(name, handle, L.ptr(ho, C.c_uint64), None) == L.E_INVALID_ARG
    assert b"NULL" in L.load().tfidf_last_error()
    assert fake.raw == b"\0" * 64 and n.value == 7 and ho.tolist() == [0, 0]
