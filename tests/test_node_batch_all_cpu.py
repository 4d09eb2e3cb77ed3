"""Node-level all-hits batch entry points (tfidf_dist_search_batch_all,
tfidf_node_search_batch_all, tfidf_dist_shard_search_batch,
tfidf_node_search_names_batch, tfidf_dist_last_names_batch,
tfidf_node_last_names_batch): argument checks that need no GPU.  A NULL handle,
NULL hit_offsets / name_offsets or NULL n_out is refused with
TFIDF_E_INVALID_ARG before any handle is read or any device touched (the
non-NULL handles below point at plain host bytes, never at an index, a
communicator or a node)."""
import ctypes as C

import numpy as np
import pytest

from tfidf_amd import _lib as L

Q = b"fast food"


def _fake():
    buf = C.create_string_buffer(64)                  # stands for a handle; must never be read
    return buf, C.cast(buf, C.c_void_p)


def _offs():
    return np.array([0, len(Q)], np.uint64)


def _batch_all(name, handles, hit_offsets, n_out):
    offs = _offs()
    docs = np.zeros(4, np.uint64)
    scores = np.zeros(4, np.float32)
    fn = getattr(L.load(), name)
    head = list(handles) + ([0] if name.startswith("tfidf_dist") else [])       # doc_base
    return fn(*head, Q, L.ptr(offs, C.c_uint64), 1, L.ptr(docs, C.c_uint64), L.ptr(scores, C.c_float), 4,
              hit_offsets, n_out)


@pytest.mark.parametrize("name, n_handles", [("tfidf_dist_search_batch_all", 2), ("tfidf_node_search_batch_all", 1)])
def test_search_batch_all_null_arguments(name, n_handles):
    fakes = [_fake() for _ in range(n_handles)]
    hs = [h for _, h in fakes]
    ho = np.zeros(2, np.uint64)
    n = C.c_uint64(7)
    for i in range(n_handles):                        # each handle NULL in turn
        assert _batch_all(name, hs[:i] + [None] + hs[i + 1:], L.ptr(ho, C.c_uint64), C.byref(n)) == L.E_INVALID_ARG
    assert _batch_all(name, hs, None, C.byref(n)) == L.E_INVALID_ARG
    assert _batch_all(name, hs, L.ptr(ho, C.c_uint64), None) == L.E_INVALID_ARG
    assert b"NULL" in L.load().tfidf_last_error()
    assert all(f.raw == b"\0" * 64 for f, _ in fakes) and n.value == 7 and ho.tolist() == [0, 0]


@pytest.mark.parametrize("name, n_handles", [("tfidf_dist_shard_search_batch", 2),
                                             ("tfidf_node_search_names_batch", 1)])
def test_names_batch_null_arguments(name, n_handles):
    fakes = [_fake() for _ in range(n_handles)]
    hs = [h for _, h in fakes]
    offs = _offs()
    n, nb = C.c_uint64(7), C.c_uint64(9)
    fn = getattr(L.load(), name)
    for i in range(n_handles):
        assert fn(*(hs[:i] + [None] + hs[i + 1:]), Q, L.ptr(offs, C.c_uint64), 1, C.byref(n),
                  C.byref(nb)) == L.E_INVALID_ARG
    assert fn(*hs, Q, L.ptr(offs, C.c_uint64), 1, None, C.byref(nb)) == L.E_INVALID_ARG
    assert b"NULL" in L.load().tfidf_last_error()
    assert all(f.raw == b"\0" * 64 for f, _ in fakes) and (n.value, nb.value) == (7, 9)


@pytest.mark.parametrize("name", ["tfidf_dist_last_names_batch", "tfidf_node_last_names_batch"])
def test_last_names_batch_null_arguments(name):
    fake, h = _fake()
    buf = C.create_string_buffer(16)
    offs = np.zeros(3, np.uint64)
    sc = np.zeros(2, np.float64)
    qo = np.zeros(2, np.uint64)
    n, nb = C.c_uint64(7), C.c_uint64(9)
    fn = getattr(L.load(), name)

    def call(handle, name_offsets, n_out, n_bytes):
        return fn(handle, buf, 16, L.ptr(offs, C.c_uint64), L.ptr(sc, C.c_double), 2, name_offsets, n_out, n_bytes)

    assert call(None, L.ptr(qo, C.c_uint64), C.byref(n), C.byref(nb)) == L.E_INVALID_ARG
    assert call(h, None, C.byref(n), C.byref(nb)) == L.E_INVALID_ARG
    assert call(h, L.ptr(qo, C.c_uint64), None, C.byref(nb)) == L.E_INVALID_ARG
    assert b"NULL" in L.load().tfidf_last_error()
    assert fake.raw == b"\0" * 64 and (n.value, nb.value) == (7, 9) and qo.tolist() == [0, 0]
