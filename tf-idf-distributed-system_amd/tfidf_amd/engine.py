"""ShardIndex: one GPU shard of the engine — the per-worker Lucene index of the
reference (Worker.java:54-55 ``luceneDir`` + ``indexWriter``) behind the C ABI.
"""
import ctypes as C
import os

import numpy as np

from . import _lib as L


def analyze(text: bytes):
    """StandardAnalyzer (Worker.java:71,225) as the engine runs it: lower-cased
    UTF-8 tokens of ``text`` (host side of the device scanner, unicode_scan.h)."""
    cap = 2 * len(text) + 64
    buf = C.create_string_buffer(cap)
    nt, nb = C.c_uint64(), C.c_uint64()
    L.check(L.load().tfidf_analyze(text, len(text), buf, cap, C.byref(nt), C.byref(nb)))
    return buf.raw[:nb.value].split(b"\0")[:nt.value]


def term_key(term: bytes):
    """128-bit device key (lo, hi) of an analysed (lower-cased) token."""
    lo, hi = C.c_uint64(), C.c_uint64()
    L.check(L.load().tfidf_term_key(term, len(term), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def _batch_all_arrays(fn, handle, queries, cap):
    """tfidf_search_batch_all / tfidf_reader_search_batch_all: one call with
    ``cap`` result slots, and once more with the size the library reports when
    that was too small.  -> (docs uint32[], scores float32[], offsets uint64[n_q + 1])."""
    nq = len(queries)
    offs = np.zeros(nq + 1, np.uint64)
    if nq:
        offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    blob = b"".join(queries)
    hit_offs = np.zeros(nq + 1, np.uint64)
    n = C.c_uint64()
    for _ in range(2):
        docs = np.empty(max(cap, 1), np.uint32)
        scores = np.empty(max(cap, 1), np.float32)
        rc = fn(handle, blob, L.ptr(offs, C.c_uint64), nq, L.ptr(docs, C.c_uint32), L.ptr(scores, C.c_float), cap,
                L.ptr(hit_offs, C.c_uint64), C.byref(n))
        if rc != L.E_BUFFER:
            break
        cap = n.value
    L.check(rc)
    return docs[:n.value], scores[:n.value], hit_offs


def _key_arrays(keys):
    """list of bytes -> (blob, uint64 offsets[n + 1])."""
    koffs = np.zeros(len(keys) + 1, np.uint64)
    if len(keys):
        koffs[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
    return b"".join(keys), koffs


def _doc_text(fn, handle, doc):
    """tfidf_doc_text / tfidf_reader_doc_text: size first, then the bytes."""
    n = C.c_uint64()
    rc = fn(handle, doc, None, 0, C.byref(n))
    if rc not in (L.OK, L.E_BUFFER):
        L.check(rc)
    buf = C.create_string_buffer(max(n.value, 1))
    L.check(fn(handle, doc, buf, n.value, C.byref(n)))
    return buf.raw[:n.value]


def query_positive_terms(q: bytes):
    """Positive terms of a query in ordinal order (tfidf_query_positive_terms):
    the analysed terms of every clause that is not MUST_NOT, distinct, by first
    appearance.  The ordinals of matches index this list."""
    cap = 2 * len(q) + 64
    buf = C.create_string_buffer(cap)
    nt, nb = C.c_uint64(), C.c_uint64()
    L.check(L.load().tfidf_query_positive_terms(q, len(q), buf, cap, C.byref(nt), C.byref(nb)))
    return buf.raw[:nb.value].split(b"\0")[:nt.value]


def _doc_array(docs):
    return np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)


def _match_lists(starts, lens, ords, offs):
    s, l, o, f = starts.tolist(), lens.tolist(), ords.tolist(), offs.tolist()
    return [list(zip(s[f[i]:f[i + 1]], l[f[i]:f[i + 1]], o[f[i]:f[i + 1]])) for i in range(len(f) - 1)]


def _matches_arrays(fn, handle, query, docs, cap=None):
    """tfidf_matches / tfidf_reader_matches: one call with ``cap`` match slots,
    and once more with the size the library reports when that was too small.
    -> (starts uint64[], lens uint32[], ordinals uint32[], offsets uint64[n + 1], ms_device)."""
    d = _doc_array(docs)
    n = len(d)
    offs = np.zeros(n + 1, np.uint64)
    total, ms = C.c_uint64(), C.c_float()
    cap = 64 * max(n, 1) if cap is None else cap
    for _ in range(2):
        st = np.empty(max(cap, 1), np.uint64)
        ln = np.empty(max(cap, 1), np.uint32)
        od = np.empty(max(cap, 1), np.uint32)
        rc = fn(handle, query, len(query), L.ptr(d, C.c_uint32), n, L.ptr(st, C.c_uint64), L.ptr(ln, C.c_uint32),
                L.ptr(od, C.c_uint32), cap, L.ptr(offs, C.c_uint64), C.byref(total), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        cap = total.value
    L.check(rc)
    m = total.value
    return st[:m], ln[:m], od[:m], offs, ms.value


def _snippets_arrays(fn, handle, query, docs, max_bytes, m_cap=None):
    """tfidf_snippets / tfidf_reader_snippets: the text buffer is sized in
    advance (n x max_bytes), the match buffers once more when too small.
    -> (text bytes, text offsets, doc_starts, starts, lens, ordinals, match offsets, ms_device)."""
    d = _doc_array(docs)
    n = len(d)
    t_cap = n * min(max(int(max_bytes), 0), 65536)
    text = np.empty(max(t_cap, 1), np.uint8)
    t_offs = np.zeros(n + 1, np.uint64)
    m_offs = np.zeros(n + 1, np.uint64)
    d_starts = np.zeros(max(n, 1), np.uint64)
    nt, nm, ms = C.c_uint64(), C.c_uint64(), C.c_float()
    m_cap = 16 * max(n, 1) if m_cap is None else m_cap
    for _ in range(2):
        st = np.empty(max(m_cap, 1), np.uint64)
        ln = np.empty(max(m_cap, 1), np.uint32)
        od = np.empty(max(m_cap, 1), np.uint32)
        rc = fn(handle, query, len(query), L.ptr(d, C.c_uint32), n, max_bytes, text.ctypes.data_as(C.c_void_p), t_cap,
                L.ptr(t_offs, C.c_uint64), L.ptr(d_starts, C.c_uint64), L.ptr(st, C.c_uint64),
                L.ptr(ln, C.c_uint32), L.ptr(od, C.c_uint32), m_cap, L.ptr(m_offs, C.c_uint64), C.byref(nt),
                C.byref(nm), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap = nm.value
    L.check(rc)
    return (text[:nt.value].tobytes(), t_offs, d_starts[:n], st[:nm.value], ln[:nm.value], od[:nm.value], m_offs,
            ms.value)


def _snippet_lists(arrays):
    text, t_offs, d_starts, st, ln, od, m_offs, _ = arrays
    t = t_offs.tolist()
    ms = _match_lists(st, ln, od, m_offs)
    return [(int(d_starts[i]), text[t[i]:t[i + 1]], ms[i]) for i in range(len(t) - 1)]


def _batch_rows(queries, docs_per_query, dtype):
    """(query blob, q offsets, docs array, doc offsets) of a highlighting batch:
    query i owns rows doc_offsets[i] .. doc_offsets[i + 1] of docs."""
    queries = list(queries)
    per = [np.asarray(d, dtype=dtype).reshape(-1) for d in docs_per_query]
    if len(per) != len(queries):
        raise ValueError("one list of documents per query")
    blob, q_offs = _key_arrays(queries)
    d_offs = np.zeros(len(per) + 1, np.uint64)
    if per:
        d_offs[1:] = np.cumsum([len(d) for d in per], dtype=np.uint64)
    docs = np.ascontiguousarray(np.concatenate(per) if per else np.zeros(0, dtype), dtype=dtype)
    return blob, q_offs, docs, d_offs


def _matches_batch_arrays(fn, handle, queries, docs_per_query, cap=None, dtype=np.uint32):
    """tfidf_[reader_|node_]matches_batch: one call with ``cap`` match slots,
    once more with the reported size when that was too small.
    -> (starts, lens, ordinals, match offsets uint64[R + 1], doc offsets uint64[n_q + 1], ms_device)."""
    blob, q_offs, d, d_offs = _batch_rows(queries, docs_per_query, dtype)
    R = len(d)
    offs = np.zeros(R + 1, np.uint64)
    total, ms = C.c_uint64(), C.c_float()
    cap = 64 * max(R, 1) if cap is None else cap
    for _ in range(2):
        st = np.empty(max(cap, 1), np.uint64)
        ln = np.empty(max(cap, 1), np.uint32)
        od = np.empty(max(cap, 1), np.uint32)
        rc = fn(handle, blob, L.ptr(q_offs, C.c_uint64), len(q_offs) - 1, L.ptr(d, np.ctypeslib.as_ctypes_type(dtype)),
                L.ptr(d_offs, C.c_uint64), L.ptr(st, C.c_uint64), L.ptr(ln, C.c_uint32), L.ptr(od, C.c_uint32), cap,
                L.ptr(offs, C.c_uint64), C.byref(total), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        cap = total.value
    L.check(rc)
    m = total.value
    return st[:m], ln[:m], od[:m], offs, d_offs, ms.value


def _snippets_batch_arrays(fn, handle, queries, docs_per_query, max_bytes, m_cap=None, dtype=np.uint32):
    """tfidf_[reader_|node_]snippets_batch: the text buffer is sized in advance
    (R x max_bytes), the match buffers once more when too small.  -> (text
    bytes, text offsets, doc_starts, starts, lens, ordinals, match offsets,
    ms_device, doc offsets uint64[n_q + 1]); the first eight as snippets_arrays."""
    blob, q_offs, d, d_offs = _batch_rows(queries, docs_per_query, dtype)
    R = len(d)
    t_cap = R * min(max(int(max_bytes), 0), 65536)
    text = np.empty(max(t_cap, 1), np.uint8)
    t_offs = np.zeros(R + 1, np.uint64)
    m_offs = np.zeros(R + 1, np.uint64)
    d_starts = np.zeros(max(R, 1), np.uint64)
    nt, nm, ms = C.c_uint64(), C.c_uint64(), C.c_float()
    m_cap = 16 * max(R, 1) if m_cap is None else m_cap
    for _ in range(2):
        st = np.empty(max(m_cap, 1), np.uint64)
        ln = np.empty(max(m_cap, 1), np.uint32)
        od = np.empty(max(m_cap, 1), np.uint32)
        rc = fn(handle, blob, L.ptr(q_offs, C.c_uint64), len(q_offs) - 1, L.ptr(d, np.ctypeslib.as_ctypes_type(dtype)),
                L.ptr(d_offs, C.c_uint64), max_bytes, text.ctypes.data_as(C.c_void_p), t_cap,
                L.ptr(t_offs, C.c_uint64), L.ptr(d_starts, C.c_uint64), L.ptr(st, C.c_uint64),
                L.ptr(ln, C.c_uint32), L.ptr(od, C.c_uint32), m_cap, L.ptr(m_offs, C.c_uint64), C.byref(nt),
                C.byref(nm), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap = nm.value
    L.check(rc)
    return (text[:nt.value].tobytes(), t_offs, d_starts[:R], st[:nm.value], ln[:nm.value], od[:nm.value], m_offs,
            ms.value, d_offs)


def _fuzzy_batch_arrays(fn, handle, terms, max_edits, prefix_len, max_out, df_dtype=np.uint32):
    """tfidf_[reader_|node_]fuzzy_terms_batch: one call with room for max_out
    candidates per term (32 bytes each on average), once more with the sizes
    the library reports when that was too small.  -> (cand offsets uint64[n +
    1], n_within uint64[n], term offsets uint64[m + 1], term blob bytes, df[m],
    dist uint8[m], ms_device)."""
    terms = list(terms)
    blob, t_offs = _key_arrays(terms)
    n = len(terms)
    c_offs = np.zeros(n + 1, np.uint64)
    within = np.zeros(max(n, 1), np.uint64)
    nc, nb, ms = C.c_uint64(), C.c_uint64(), C.c_float()
    dfc = np.ctypeslib.as_ctypes_type(df_dtype)
    m_cap = min(n * max(int(max_out), 0), 1 << 20)
    b_cap = 32 * m_cap
    for _ in range(2):
        t_out = np.zeros(m_cap + 1, np.uint64)
        text = np.empty(max(b_cap, 1), np.uint8)
        df = np.zeros(max(m_cap, 1), df_dtype)
        dist = np.zeros(max(m_cap, 1), np.uint8)
        rc = fn(handle, blob, L.ptr(t_offs, C.c_uint64), n, max_edits, prefix_len, max_out,
                L.ptr(c_offs, C.c_uint64), L.ptr(within, C.c_uint64), L.ptr(t_out, C.c_uint64),
                text.ctypes.data_as(C.c_void_p), b_cap, L.ptr(df, dfc), L.ptr(dist, C.c_uint8), m_cap, C.byref(nc),
                C.byref(nb), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap, b_cap = nc.value, nb.value
    L.check(rc)
    m, b = nc.value, nb.value
    return c_offs, within[:n], t_out[:m + 1], text[:b].tobytes(), df[:m], dist[:m], ms.value


def _fuzzy_lists(arrays):
    """-> per input term ([(term bytes, df, dist)], n_within)."""
    c_offs, within, t_out, text, df, dist, _ = arrays
    c, t, f, d = c_offs.tolist(), t_out.tolist(), df.tolist(), dist.tolist()
    cands = [(text[t[j]:t[j + 1]], f[j], d[j]) for j in range(len(t) - 1)]
    return [(cands[c[i]:c[i + 1]], int(within[i])) for i in range(len(c) - 1)]


def _fuzzy_single(fn, handle, term, max_edits, prefix_len, max_out):
    """tfidf_fuzzy_terms / tfidf_reader_fuzzy_terms, sized as _fuzzy_batch_arrays sizes the batch."""
    within, nc, nb, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
    m_cap = min(max(int(max_out), 0), 1 << 20)
    b_cap = 32 * m_cap
    for _ in range(2):
        t_out = np.zeros(m_cap + 1, np.uint64)
        text = np.empty(max(b_cap, 1), np.uint8)
        df = np.zeros(max(m_cap, 1), np.uint32)
        dist = np.zeros(max(m_cap, 1), np.uint8)
        rc = fn(handle, term, len(term), max_edits, prefix_len, max_out, C.byref(within), L.ptr(t_out, C.c_uint64),
                text.ctypes.data_as(C.c_void_p), b_cap, L.ptr(df, C.c_uint32), L.ptr(dist, C.c_uint8), m_cap,
                C.byref(nc), C.byref(nb), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap, b_cap = nc.value, nb.value
    L.check(rc)
    raw, t = text[:nb.value].tobytes(), t_out.tolist()
    return [(raw[t[j]:t[j + 1]], int(df[j]), int(dist[j])) for j in range(nc.value)], within.value


def _fuzzy_expand_arrays(fn, handle, terms, max_edits, prefix_len, max_expansions):
    """tfidf_[reader_]fuzzy_expand_batch, sized as _fuzzy_batch_arrays sizes the
    lookup.  -> (cand offsets uint64[n + 1], n_within uint64[n], term offsets
    uint64[m + 1], term blob bytes, df uint32[m], dist uint8[m], boosts
    float32[m], ms_device)."""
    terms = list(terms)
    blob, t_offs = _key_arrays(terms)
    n = len(terms)
    c_offs = np.zeros(n + 1, np.uint64)
    within = np.zeros(max(n, 1), np.uint64)
    nc, nb, ms = C.c_uint64(), C.c_uint64(), C.c_float()
    m_cap = min(n * min(max(int(max_expansions), 0), 64), 1 << 20)
    b_cap = 32 * m_cap
    for _ in range(2):
        t_out = np.zeros(m_cap + 1, np.uint64)
        text = np.empty(max(b_cap, 1), np.uint8)
        df = np.zeros(max(m_cap, 1), np.uint32)
        dist = np.zeros(max(m_cap, 1), np.uint8)
        boosts = np.zeros(max(m_cap, 1), np.float32)
        rc = fn(handle, blob, L.ptr(t_offs, C.c_uint64), n, max_edits, prefix_len, max_expansions,
                L.ptr(c_offs, C.c_uint64), L.ptr(within, C.c_uint64), L.ptr(t_out, C.c_uint64),
                text.ctypes.data_as(C.c_void_p), b_cap, L.ptr(df, C.c_uint32), L.ptr(dist, C.c_uint8),
                L.ptr(boosts, C.c_float), m_cap, C.byref(nc), C.byref(nb), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap, b_cap = nc.value, nb.value
    L.check(rc)
    m, b = nc.value, nb.value
    return c_offs, within[:n], t_out[:m + 1], text[:b].tobytes(), df[:m], dist[:m], boosts[:m], ms.value


def _fuzzy_expand_lists(arrays):
    """-> per input term ([(term bytes, df, dist, boost)], n_within); boost is a Python float holding the float32."""
    c_offs, within, t_out, text, df, dist, boosts, _ = arrays
    c, t, f, d, bo = c_offs.tolist(), t_out.tolist(), df.tolist(), dist.tolist(), boosts.tolist()
    cands = [(text[t[j]:t[j + 1]], f[j], d[j], bo[j]) for j in range(len(t) - 1)]
    return [(cands[c[i]:c[i + 1]], int(within[i])) for i in range(len(c) - 1)]


def _fuzzy_expand_single(fn, handle, term, max_edits, prefix_len, max_expansions):
    """tfidf_fuzzy_expand / tfidf_reader_fuzzy_expand -> ([(term bytes, df, dist, boost)], n_within)."""
    within, nc, nb, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
    m_cap = min(max(int(max_expansions), 0), 64)
    b_cap = 32 * m_cap
    for _ in range(2):
        t_out = np.zeros(m_cap + 1, np.uint64)
        text = np.empty(max(b_cap, 1), np.uint8)
        df = np.zeros(max(m_cap, 1), np.uint32)
        dist = np.zeros(max(m_cap, 1), np.uint8)
        boosts = np.zeros(max(m_cap, 1), np.float32)
        rc = fn(handle, term, len(term), max_edits, prefix_len, max_expansions, C.byref(within),
                L.ptr(t_out, C.c_uint64), text.ctypes.data_as(C.c_void_p), b_cap, L.ptr(df, C.c_uint32),
                L.ptr(dist, C.c_uint8), L.ptr(boosts, C.c_float), m_cap, C.byref(nc), C.byref(nb), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap, b_cap = nc.value, nb.value
    L.check(rc)
    raw, t = text[:nb.value].tobytes(), t_out.tolist()
    return ([(raw[t[j]:t[j + 1]], int(df[j]), int(dist[j]), float(boosts[j])) for j in range(nc.value)],
            within.value)


def _fuzzy_search_arrays(fn, handle, terms, max_edits, prefix_len, max_expansions, cap=None, dtype=np.uint32):
    """tfidf_[reader_|node_]search_fuzzy_batch: one call with ``cap`` hit slots,
    once more with the size the library reports when that was too small.  ->
    (docs, scores float32[], hit offsets uint64[n + 1], n_expanded uint32[n], ms_device)."""
    terms = list(terms)
    blob, t_offs = _key_arrays(terms)
    n = len(terms)
    offs = np.zeros(n + 1, np.uint64)
    n_exp = np.zeros(max(n, 1), np.uint32)
    total, ms = C.c_uint64(), C.c_float()
    cap = min(4096 * max(n, 1), 1 << 24) if cap is None else cap
    for _ in range(2):
        docs = np.empty(max(cap, 1), dtype)
        scores = np.empty(max(cap, 1), np.float32)
        rc = fn(handle, blob, L.ptr(t_offs, C.c_uint64), n, max_edits, prefix_len, max_expansions,
                L.ptr(docs, np.ctypeslib.as_ctypes_type(dtype)), L.ptr(scores, C.c_float), cap,
                L.ptr(offs, C.c_uint64), L.ptr(n_exp, C.c_uint32), C.byref(total), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        cap = total.value
    L.check(rc)
    m = total.value
    return docs[:m], scores[:m], offs, n_exp[:n], ms.value


def _fuzzy_search_lists(arrays):
    """-> per input term [(doc, score)]."""
    docs, scores, offs, _, _ = arrays
    d, s, o = docs.tolist(), scores.tolist(), offs.tolist()
    return [list(zip(d[o[i]:o[i + 1]], s[o[i]:o[i + 1]])) for i in range(len(o) - 1)]


def _fuzzy_search_single(fn, handle, term, max_edits, prefix_len, max_expansions):
    """tfidf_search_fuzzy / tfidf_reader_search_fuzzy -> (docs uint32[], scores float32[], n_expanded)."""
    total, ms, n_exp = C.c_uint64(), C.c_float(), C.c_uint32()
    cap = 4096
    for _ in range(2):
        docs = np.empty(max(cap, 1), np.uint32)
        scores = np.empty(max(cap, 1), np.float32)
        rc = fn(handle, term, len(term), max_edits, prefix_len, max_expansions, L.ptr(docs, C.c_uint32),
                L.ptr(scores, C.c_float), cap, C.byref(n_exp), C.byref(total), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        cap = total.value
    L.check(rc)
    return docs[:total.value], scores[:total.value], n_exp.value


# Compound queries: a query is a list of clauses, a clause the tuple (occur, kind,
# payload, params...) with params = (slop,) for a phrase and (max_edits,
# prefix_len, max_expansions) for a fuzzy term.  The constructors below build the
# (kind, payload, params...) part, the occur wrappers put the occur in front:
# must(phrase(b"a b", slop=1)), should(text(b"gpu")), must_not(fuzzy(b"nvidia", 1)).
def text(payload: bytes):
    return (L.CLAUSE_TEXT, bytes(payload))


def phrase(payload: bytes, slop=0):
    return (L.CLAUSE_PHRASE, bytes(payload), int(slop))


def wildcard(payload: bytes):
    return (L.CLAUSE_WILDCARD, bytes(payload))


def regex(payload: bytes):
    return (L.CLAUSE_REGEX, bytes(payload))


def fuzzy(payload: bytes, max_edits=2, prefix_len=0, max_expansions=50):
    return (L.CLAUSE_FUZZY, bytes(payload), int(max_edits), int(prefix_len), int(max_expansions))


def should(clause):
    return (L.OCCUR_SHOULD,) + tuple(clause)


def must(clause):
    return (L.OCCUR_MUST,) + tuple(clause)


def must_not(clause):
    return (L.OCCUR_MUST_NOT,) + tuple(clause)


def filter_(clause):
    return (L.OCCUR_FILTER,) + tuple(clause)


def group(children, min_should_match=0):
    """A clause group of the nested calls: ``children`` are occurred clauses or
    occurred groups, must(group([should(text(b"a")), should(text(b"b"))], 2))."""
    return (L.CLAUSE_GROUP, tuple(children), int(min_should_match))


def _fill_clause(rec, occur, kind, params):
    if not (0 <= occur <= 255 and 0 <= kind <= 255):
        raise ValueError("occur and kind are bytes")
    rec.occur, rec.kind = occur, kind
    if kind == L.CLAUSE_PHRASE:
        rec.slop = params[0] if params else 0
    elif kind == L.CLAUSE_FUZZY:
        me, pl, mx = (tuple(params) + (2, 0, 50)[len(params):])[:3]
        rec.max_edits, rec.prefix_len, rec.max_expansions = min(me, 255), pl, min(max(mx, 0), 255)


def _clause_arrays(queries):
    """[[clause]] -> (payload blob, uint64 payload offsets, Clause array, uint64 clause offsets per query)."""
    flat = [c for q in queries for c in q]
    q_offs = np.zeros(len(queries) + 1, np.uint64)
    if len(queries):
        q_offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    blob, c_offs = _key_arrays([c[2] for c in flat])
    arr = (L.Clause * max(len(flat), 1))()
    for i, c in enumerate(flat):
        _fill_clause(arr[i], int(c[0]), int(c[1]), c[3:])
    return blob, c_offs, arr, q_offs


def _as_root(query):
    """A nested query: a group(...) tuple, or a plain list of occurred clauses, which is a root with m = 0."""
    if isinstance(query, tuple) and len(query) == 3 and query[0] == L.CLAUSE_GROUP:
        return query
    return group(query)


def _qnode_arrays(queries):
    """[nested query] -> (payload blob, uint64 payload offsets, QNode array, uint64 node offsets per query): every
    tree in pre-order, the root first."""
    flat, sizes = [], []                      # (occur, kind, payload, params, parent, m)

    def walk(occur, node, parent, first):
        kind = int(node[0])
        at = len(flat) - first
        if kind == L.CLAUSE_GROUP:
            flat.append((occur, kind, b"", (), parent, int(node[2])))
            for child in node[1]:
                walk(int(child[0]), child[1:], at, first)
        else:
            flat.append((occur, kind, node[1], node[2:], parent, 0))

    for q in queries:
        first = len(flat)
        walk(L.OCCUR_SHOULD, _as_root(q), L.QNODE_ROOT, first)
        sizes.append(len(flat) - first)
    q_offs = np.zeros(len(queries) + 1, np.uint64)
    if len(queries):
        q_offs[1:] = np.cumsum(sizes, dtype=np.uint64)
    blob, c_offs = _key_arrays([n[2] for n in flat])
    arr = (L.QNode * max(len(flat), 1))()
    for i, (occur, kind, _, params, parent, m) in enumerate(flat):
        _fill_clause(arr[i], occur, kind, params)
        arr[i].parent, arr[i].min_should_match = parent, m
    return blob, c_offs, arr, q_offs


def _compound_arrays(fn, handle, queries, cap=None, dtype=np.uint32, arrays=None):
    """tfidf_[reader_|node_]search_compound_batch: one call with ``cap`` hit
    slots, once more with the size the library reports when that was too small.
    -> (docs, scores float32[], hit offsets uint64[n_q + 1], ms_device).
    ``arrays``: the (blob, payload offsets, records, query offsets) builder;
    _qnode_arrays for the nested calls."""
    queries = list(queries) if arrays else [list(q) for q in queries]
    blob, c_offs, arr, q_offs = (arrays or _clause_arrays)(queries)
    nq = len(queries)
    offs = np.zeros(nq + 1, np.uint64)
    total, ms = C.c_uint64(), C.c_float()
    cap = min(4096 * max(nq, 1), 1 << 24) if cap is None else cap
    for _ in range(2):
        docs = np.empty(max(cap, 1), dtype)
        scores = np.empty(max(cap, 1), np.float32)
        rc = fn(handle, blob, L.ptr(c_offs, C.c_uint64), arr, L.ptr(q_offs, C.c_uint64), nq,
                L.ptr(docs, np.ctypeslib.as_ctypes_type(dtype)), L.ptr(scores, C.c_float), cap,
                L.ptr(offs, C.c_uint64), C.byref(total), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        cap = total.value
    L.check(rc)
    m = total.value
    return docs[:m], scores[:m], offs, ms.value


def _compound_lists(arrays):
    """-> per query [(doc, score)]."""
    docs, scores, offs, _ = arrays
    d, s, o = docs.tolist(), scores.tolist(), offs.tolist()
    return [list(zip(d[o[i]:o[i + 1]], s[o[i]:o[i + 1]])) for i in range(len(o) - 1)]


def _wildcard_terms_arrays(fn, handle, patterns, max_out, df_dtype=np.uint32):
    """tfidf_[reader_|node_]wildcard_terms_batch, sized as _fuzzy_batch_arrays
    sizes the fuzzy batch.  -> (cand offsets uint64[n + 1], n_matched
    uint64[n], term offsets uint64[m + 1], term blob bytes, df[m], ms_device)."""
    patterns = list(patterns)
    blob, p_offs = _key_arrays(patterns)
    n = len(patterns)
    c_offs = np.zeros(n + 1, np.uint64)
    matched = np.zeros(max(n, 1), np.uint64)
    nc, nb, ms = C.c_uint64(), C.c_uint64(), C.c_float()
    dfc = np.ctypeslib.as_ctypes_type(df_dtype)
    m_cap = min(n * max(int(max_out), 0), 1 << 20)
    b_cap = 32 * m_cap
    for _ in range(2):
        t_out = np.zeros(m_cap + 1, np.uint64)
        text = np.empty(max(b_cap, 1), np.uint8)
        df = np.zeros(max(m_cap, 1), df_dtype)
        rc = fn(handle, blob, L.ptr(p_offs, C.c_uint64), n, max_out, L.ptr(c_offs, C.c_uint64),
                L.ptr(matched, C.c_uint64), L.ptr(t_out, C.c_uint64), text.ctypes.data_as(C.c_void_p), b_cap,
                L.ptr(df, dfc), m_cap, C.byref(nc), C.byref(nb), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap, b_cap = nc.value, nb.value
    L.check(rc)
    m, b = nc.value, nb.value
    return c_offs, matched[:n], t_out[:m + 1], text[:b].tobytes(), df[:m], ms.value


def _wildcard_term_lists(arrays):
    """-> per pattern ([(term bytes, df)], n_matched)."""
    c_offs, matched, t_out, text, df, _ = arrays
    c, t, f = c_offs.tolist(), t_out.tolist(), df.tolist()
    cands = [(text[t[j]:t[j + 1]], f[j]) for j in range(len(t) - 1)]
    return [(cands[c[i]:c[i + 1]], int(matched[i])) for i in range(len(c) - 1)]


def _wildcard_terms_single(fn, handle, pattern, max_out):
    """tfidf_wildcard_terms / tfidf_reader_wildcard_terms -> ([(term bytes, df)], n_matched)."""
    matched, nc, nb, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
    m_cap = min(max(int(max_out), 0), 1 << 20)
    b_cap = 32 * m_cap
    for _ in range(2):
        t_out = np.zeros(m_cap + 1, np.uint64)
        text = np.empty(max(b_cap, 1), np.uint8)
        df = np.zeros(max(m_cap, 1), np.uint32)
        rc = fn(handle, pattern, len(pattern), max_out, C.byref(matched), L.ptr(t_out, C.c_uint64),
                text.ctypes.data_as(C.c_void_p), b_cap, L.ptr(df, C.c_uint32), m_cap, C.byref(nc), C.byref(nb),
                C.byref(ms))
        if rc != L.E_BUFFER:
            break
        m_cap, b_cap = nc.value, nb.value
    L.check(rc)
    raw, t = text[:nb.value].tobytes(), t_out.tolist()
    return [(raw[t[j]:t[j + 1]], int(df[j])) for j in range(nc.value)], matched.value


def _wildcard_docs_arrays(fn, handle, patterns, cap=None, dtype=np.uint32):
    """tfidf_[reader_|node_]search_wildcard_batch: one call for the sizes (or
    with ``cap`` hit slots), then again with the size reported while that was too small.
    -> (doc ids dtype[], hit offsets uint64[n + 1], n_matched uint64[n], ms_device)."""
    patterns = list(patterns)
    blob, p_offs = _key_arrays(patterns)
    n = len(patterns)
    h_offs = np.zeros(n + 1, np.uint64)
    matched = np.zeros(max(n, 1), np.uint64)
    total, ms = C.c_uint64(), C.c_float()
    dc = np.ctypeslib.as_ctypes_type(dtype)
    cap = 0 if cap is None else int(cap)
    for _ in range(8):                      # beside commits the index may have grown between two calls: ask again
        docs = np.empty(max(cap, 1), dtype)
        rc = fn(handle, blob, L.ptr(p_offs, C.c_uint64), n, L.ptr(docs, dc) if cap else None, cap,
                L.ptr(h_offs, C.c_uint64), L.ptr(matched, C.c_uint64), C.byref(total), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        cap = total.value
    L.check(rc)
    return docs[:total.value], h_offs, matched[:n], ms.value


def _wildcard_doc_lists(arrays):
    """-> per pattern (ascending doc ids, n_matched)."""
    docs, h_offs, matched, _ = arrays
    d, o = docs.tolist(), h_offs.tolist()
    return [(d[o[i]:o[i + 1]], int(matched[i])) for i in range(len(o) - 1)]


def _wildcard_docs_single(fn, handle, pattern):
    """tfidf_search_wildcard / tfidf_reader_search_wildcard -> (ascending doc ids, n_matched)."""
    matched, total, ms = C.c_uint64(), C.c_uint64(), C.c_float()
    cap = 0
    for _ in range(8):                      # as _wildcard_docs_arrays
        docs = np.empty(max(cap, 1), np.uint32)
        rc = fn(handle, pattern, len(pattern), L.ptr(docs, C.c_uint32) if cap else None, cap, C.byref(matched),
                C.byref(total), C.byref(ms))
        if rc != L.E_BUFFER:
            break
        cap = total.value
    L.check(rc)
    return docs[:total.value].tolist(), matched.value


def _per_query(rows, d_offs):
    f = d_offs.tolist()
    return [rows[f[i]:f[i + 1]] for i in range(len(f) - 1)]


def _hit_lists(docs, scores, offs):
    d, s, o = docs.tolist(), scores.tolist(), offs.tolist()
    return [list(zip(d[o[i]:o[i + 1]], s[o[i]:o[i + 1]])) for i in range(len(o) - 1)]


def _phrase_batch_arrays(fn, handle, phrases, cap=None, dtype=np.uint32, slops=None):
    """tfidf_[reader_|node_]search_phrase[_slop]_batch: one call for the sizes
    (or with ``cap`` result slots), one more for the payload when that was too
    small.  -> (docs dtype[], scores float32[], freqs uint32[], offsets
    uint64[n_p + 1]); with ``slops`` (one per phrase: the _slop_ calls) freqs is
    float32[]."""
    n_p = len(phrases)
    blob, offs = _key_arrays(phrases)
    extra, ft, fct = (), np.uint32, C.c_uint32
    if slops is not None:
        slops = np.ascontiguousarray(slops, np.uint32)
        if slops.shape != (n_p,):
            raise ValueError("one slop per phrase")
        extra, ft, fct = (L.ptr(slops, C.c_uint32),), np.float32, C.c_float
    hit_offs = np.zeros(n_p + 1, np.uint64)
    n = C.c_uint64()
    ct = C.c_uint32 if dtype == np.uint32 else C.c_uint64
    cap = 0 if cap is None else cap
    for _ in range(2):
        docs = np.empty(max(cap, 1), dtype)
        scores = np.empty(max(cap, 1), np.float32)
        freqs = np.empty(max(cap, 1), ft)
        rc = fn(handle, blob, L.ptr(offs, C.c_uint64), *extra, n_p, L.ptr(docs, ct) if cap else None,
                L.ptr(scores, C.c_float) if cap else None, L.ptr(freqs, fct) if cap else None, cap,
                L.ptr(hit_offs, C.c_uint64), C.byref(n))
        if rc != L.E_BUFFER:
            break
        cap = n.value
    L.check(rc)
    return docs[:n.value], scores[:n.value], freqs[:n.value], hit_offs


def _phrase_lists(docs, scores, freqs, offs):
    d, s, f, o = docs.tolist(), scores.tolist(), freqs.tolist(), offs.tolist()
    return [list(zip(d[o[i]:o[i + 1]], s[o[i]:o[i + 1]], f[o[i]:o[i + 1]])) for i in range(len(o) - 1)]


def _phrase_single(fn, handle, phrase, slop=None):
    """tfidf_[reader_]search_phrase[_slop] -> [(doc, score, freq)]; with
    ``slop`` (the _slop calls) freq is a float."""
    n = C.c_uint64()
    cap = 0
    extra, ft, fct = ((), np.uint32, C.c_uint32) if slop is None else ((slop,), np.float32, C.c_float)
    for _ in range(8):                      # as _wildcard_docs_arrays
        docs = np.empty(max(cap, 1), np.uint32)
        scores = np.empty(max(cap, 1), np.float32)
        freqs = np.empty(max(cap, 1), ft)
        rc = fn(handle, phrase, len(phrase), *extra, L.ptr(docs, C.c_uint32) if cap else None,
                L.ptr(scores, C.c_float) if cap else None, L.ptr(freqs, fct) if cap else None, cap, C.byref(n))
        if rc != L.E_BUFFER:
            break
        cap = n.value
    L.check(rc)
    m = n.value
    return list(zip(docs[:m].tolist(), scores[:m].tolist(), freqs[:m].tolist()))


def mlt_params(min_tf=None, min_df=None, max_df=None, max_terms=None):
    """tfidf_mlt_params with Lucene's MoreLikeThis defaults (min_tf 2, min_df 5,
    max_df 0 = no upper bound, max_terms 25) where an argument is None."""
    p = L.MltParams()
    L.check(L.load().tfidf_mlt_params_init(C.byref(p)))
    for name, v in (("min_tf", min_tf), ("min_df", min_df), ("max_df", max_df), ("max_terms", max_terms)):
        if v is not None:
            setattr(p, name, v)
    return p


def _mlt_terms_arrays(fn, handle, docs, params, term_cap=None, bytes_cap=None):
    """tfidf_[reader_]mlt_terms_batch: one call for the sizes (or with the given
    caps), one more for the payload when that was too small.  -> (term offsets
    uint64[n + 1], n_candidates uint64[n], blob offsets uint64[m + 1], term blob
    bytes, tf uint32[m], df uint32[m], score float32[m])."""
    seeds = np.ascontiguousarray(docs, np.uint32)
    n = len(seeds)
    t_offs = np.zeros(n + 1, np.uint64)
    cand = np.zeros(max(n, 1), np.uint64)
    nt, nb = C.c_uint64(), C.c_uint64()
    t_cap = 0 if term_cap is None else term_cap
    b_cap = 0 if bytes_cap is None else bytes_cap
    for _ in range(2):
        b_offs = np.zeros(t_cap + 1, np.uint64)
        blob = np.empty(max(b_cap, 1), np.uint8)
        tf = np.zeros(max(t_cap, 1), np.uint32)
        df = np.zeros(max(t_cap, 1), np.uint32)
        score = np.zeros(max(t_cap, 1), np.float32)
        rc = fn(handle, L.ptr(seeds, C.c_uint32), n, C.byref(params), L.ptr(t_offs, C.c_uint64),
                L.ptr(cand, C.c_uint64), L.ptr(b_offs, C.c_uint64) if t_cap else None,
                blob.ctypes.data_as(C.c_void_p) if b_cap else None, b_cap, L.ptr(tf, C.c_uint32) if t_cap else None,
                L.ptr(df, C.c_uint32) if t_cap else None, L.ptr(score, C.c_float) if t_cap else None, t_cap,
                C.byref(nt), C.byref(nb))
        if rc != L.E_BUFFER or term_cap is not None or bytes_cap is not None:
            break
        t_cap, b_cap = nt.value, nb.value
    L.check(rc)
    m = nt.value
    return t_offs, cand[:n], b_offs[:m + 1], blob[:nb.value].tobytes(), tf[:m], df[:m], score[:m]


def _mlt_terms_lists(arrays):
    """-> per seed ([(term bytes, tf, df, score)], n_candidates)."""
    t_offs, cand, b_offs, blob, tf, df, score = arrays
    o, b, f, d, s = t_offs.tolist(), b_offs.tolist(), tf.tolist(), df.tolist(), score.tolist()
    terms = [(blob[b[j]:b[j + 1]], f[j], d[j], s[j]) for j in range(len(b) - 1)]
    return [(terms[o[i]:o[i + 1]], int(cand[i])) for i in range(len(o) - 1)]


def _mlt_batch_arrays(fn, handle, docs, k, exclude_seed, params):
    """tfidf_[reader_]more_like_this_batch -> (docs uint32[n, k], scores float32[n, k], counts uint32[n])."""
    seeds = np.ascontiguousarray(docs, np.uint32)
    n = len(seeds)
    out_d = np.zeros((max(n, 1), max(k, 1)), np.uint32)
    out_s = np.zeros((max(n, 1), max(k, 1)), np.float32)
    cnt = np.zeros(max(n, 1), np.uint32)
    L.check(fn(handle, L.ptr(seeds, C.c_uint32), n, C.byref(params), k, L.MLT_EXCLUDE_SEED if exclude_seed else 0,
               L.ptr(out_d, C.c_uint32), L.ptr(out_s, C.c_float), L.ptr(cnt, C.c_uint32)))
    return out_d[:n], out_s[:n], cnt[:n]


def _mlt_single(fn, handle, doc, k, exclude_seed, params):
    """tfidf_[reader_]more_like_this -> [(doc, score)]."""
    out_d = np.zeros(max(k, 1), np.uint32)
    out_s = np.zeros(max(k, 1), np.float32)
    cnt = C.c_uint32()
    L.check(fn(handle, doc, C.byref(params), k, L.MLT_EXCLUDE_SEED if exclude_seed else 0, L.ptr(out_d, C.c_uint32),
               L.ptr(out_s, C.c_float), C.byref(cnt)))
    return list(zip(out_d[:cnt.value].tolist(), out_s[:cnt.value].tolist()))


def _topk_lists(docs, scores, counts):
    return [list(zip(docs[i, :c].tolist(), scores[i, :c].tolist())) for i, c in enumerate(counts.tolist())]


class ShardIndex:
    def __init__(self, device=0, k1=1.2, b=0.75, vocab_capacity_log2=18, stats_mode=L.STATS_SHARD,
                 inversion=L.INVERSION_AUTO):
        lib = L.load()
        cfg = L.Config()
        L.check(lib.tfidf_config_init(C.byref(cfg)))
        cfg.k1, cfg.b, cfg.device = k1, b, device
        cfg.vocab_capacity_log2 = vocab_capacity_log2
        cfg.stats_mode = stats_mode
        cfg.inversion = inversion
        h = C.c_void_p()
        L.check(lib.tfidf_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.device = device

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if self._h:
            L.load().tfidf_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- indexing (Worker.addDocToIndex / IndexWriter.commit) ----------------
    def add_documents(self, texts, keys=None):
        """texts: list of bytes; keys: list of bytes (relative paths) or None."""
        n = len(texts)
        offs = np.zeros(n + 1, np.uint64)
        if n:
            offs[1:] = np.cumsum([len(t) for t in texts], dtype=np.uint64)
        blob = b"".join(texts)
        kb, koffs = None, None
        if keys is not None:
            assert len(keys) == n
            koffs = np.zeros(n + 1, np.uint64)
            if n:
                koffs[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
            kb = b"".join(keys)
        L.check(L.load().tfidf_add_docs(self._h, blob, L.ptr(offs, C.c_uint64), n, kb,
                                        None if koffs is None else L.ptr(koffs, C.c_uint64)))

    def add_documents_buffer(self, text, offsets):
        """Host corpus as one uint8 buffer + uint64 offsets[n + 1] (no per-doc
        Python objects): the loader path the reference's Worker.init feeds."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        L.check(L.load().tfidf_add_docs(self._h, C.c_void_p(text.ctypes.data), L.ptr(offsets, C.c_uint64),
                                        len(offsets) - 1, None, None))

    def save(self, path):
        """Persist the staged corpus + keys (tfidf_save); the index is rebuilt by commit() after load()."""
        L.check(L.load().tfidf_save(self._h, os.fsencode(path)))

    def load(self, path):
        """Stage a saved index file into this (empty) index; call commit() next."""
        L.check(L.load().tfidf_load(self._h, os.fsencode(path)))

    def clear(self):
        """Drop all staged/committed documents; device buffers are kept for reuse."""
        L.check(L.load().tfidf_clear(self._h))

    def add_documents_device(self, d_text, d_offsets, n_docs, total_bytes):
        L.check(L.load().tfidf_add_docs_device(self._h, C.c_void_p(d_text), C.c_void_p(d_offsets), n_docs,
                                               total_bytes))

    def commit(self):
        L.check(L.load().tfidf_commit(self._h))

    # -- document lifecycle (IndexWriter.deleteDocuments / segment merges) -----
    def delete_documents(self, keys):
        """Stage the deletion of the documents named by keys (list of bytes;
        a keyless document's key is its decimal ordinal).  Returns how many
        documents went from live to dead; visible to searches after commit()."""
        kb, koffs = _key_arrays(list(keys))
        n = C.c_uint64()
        L.check(L.load().tfidf_delete_docs(self._h, kb, L.ptr(koffs, C.c_uint64), len(koffs) - 1, C.byref(n)))
        return n.value

    def compact(self):
        """Reclaim the dead documents of the staged corpus (tfidf_compact)."""
        nb, ms = C.c_uint64(), C.c_float()
        L.check(L.load().tfidf_compact(self._h, C.byref(nb), C.byref(ms)))
        return {"bytes_reclaimed": nb.value, "ms_device": ms.value}

    def set_compact_threshold(self, pct):
        """commit() compacts first when dead text >= pct % of the staged text (0 = never)."""
        L.check(L.load().tfidf_set_compact_threshold(self._h, pct))

    def doc_text(self, doc):
        """The committed document's bytes as they were added."""
        return _doc_text(L.load().tfidf_doc_text, self._h, doc)

    def matches(self, query: bytes, docs):
        """Per document of ``docs``: [(start, len, ordinal)] of the tokens that
        are positive terms of ``query``, in document bytes, on the snapshot
        published now (tfidf_matches)."""
        return _match_lists(*_matches_arrays(L.load().tfidf_matches, self._h, query, docs)[:4])

    def snippets(self, query: bytes, docs, max_bytes=160):
        """Per document of ``docs``: (doc_start, snippet bytes, [(start, len,
        ordinal)] in snippet bytes) — the passage of at most ``max_bytes``
        bytes with the most distinct query terms (tfidf_snippets)."""
        return _snippet_lists(_snippets_arrays(L.load().tfidf_snippets, self._h, query, docs, max_bytes))

    def matches_batch(self, queries, docs_per_query):
        """[matches(q, docs) for q, docs in zip(queries, docs_per_query)] in
        one pass (tfidf_matches_batch); a query that does not parse has no
        matches."""
        a = _matches_batch_arrays(L.load().tfidf_matches_batch, self._h, queries, docs_per_query)
        return _per_query(_match_lists(*a[:4]), a[4])

    def snippets_batch(self, queries, docs_per_query, max_bytes=160):
        """[snippets(q, docs, max_bytes) for q, docs in zip(queries,
        docs_per_query)] in one pass (tfidf_snippets_batch); the rows of a
        query that does not parse get head-of-document snippets."""
        a = _snippets_batch_arrays(L.load().tfidf_snippets_batch, self._h, queries, docs_per_query, max_bytes)
        return _per_query(_snippet_lists(a[:8]), a[8])

    def last_highlight_chunks(self):
        """(item chunks, row chunks) of the last batched highlighting call on
        this index or one of its readers (tfidf_last_highlight_chunks)."""
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_last_highlight_chunks(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fuzzy_terms(self, term: bytes, max_edits=2, prefix_len=0, max_out=10):
        """([(term bytes, df, dist)], n_within): the vocabulary terms within
        ``max_edits`` (0..2) edits of ``term`` (optimal string alignment over
        code points) that share its first ``prefix_len`` code points, in
        (dist, df descending, bytes) order, at most ``max_out`` (1..1024) of
        the n_within there are; df is this shard's own (tfidf_fuzzy_terms)."""
        return _fuzzy_single(L.load().tfidf_fuzzy_terms, self._h, term, max_edits, prefix_len, max_out)

    def fuzzy_terms_batch(self, terms, max_edits=2, prefix_len=0, max_out=10):
        """[fuzzy_terms(t, ...) for t in terms] from one pass over the
        dictionary per chunk of terms (tfidf_fuzzy_terms_batch); a term that is
        empty, not UTF-8 or longer than 255 UTF-16 units gives ([], 0)."""
        return _fuzzy_lists(_fuzzy_batch_arrays(L.load().tfidf_fuzzy_terms_batch, self._h, terms, max_edits,
                                                prefix_len, max_out))

    def fuzzy_expand(self, term: bytes, max_edits=2, prefix_len=0, max_expansions=50):
        """([(term bytes, df, dist, boost)], n_within): the expansion of
        Lucene's FuzzyQuery(term, max_edits, prefix_len, max_expansions) under
        its top-terms rewrite (tfidf_fuzzy_expand): the candidates of
        fuzzy_terms with m = min(code points of the candidate, of the term) >
        dist, boost 1 - dist / m in float32, the first max_expansions (1..64)
        in (boost descending, term bytes ascending) order."""
        return _fuzzy_expand_single(L.load().tfidf_fuzzy_expand, self._h, term, max_edits, prefix_len, max_expansions)

    def fuzzy_expand_batch_arrays(self, terms, max_edits=2, prefix_len=0, max_expansions=50):
        """(cand offsets, n_within, term offsets, term blob, df, dist, boosts, ms_device) of tfidf_fuzzy_expand_batch."""
        return _fuzzy_expand_arrays(L.load().tfidf_fuzzy_expand_batch, self._h, terms, max_edits, prefix_len,
                                    max_expansions)

    def fuzzy_expand_batch(self, terms, max_edits=2, prefix_len=0, max_expansions=50):
        """[fuzzy_expand(t, ...) for t in terms] in one call."""
        return _fuzzy_expand_lists(self.fuzzy_expand_batch_arrays(terms, max_edits, prefix_len, max_expansions))

    def search_fuzzy_arrays(self, term: bytes, max_edits=2, prefix_len=0, max_expansions=50):
        """(docs uint32[], scores float32[], n_expanded) of tfidf_search_fuzzy."""
        return _fuzzy_search_single(L.load().tfidf_search_fuzzy, self._h, term, max_edits, prefix_len, max_expansions)

    def search_fuzzy(self, term: bytes, max_edits=2, prefix_len=0, max_expansions=50):
        """[(doc, score)]: every document holding a term of fuzzy_expand(term,
        ...), scored as the disjunction of the expansion's terms, each weighted
        boost * idf(largest df of the expansion); (score desc, doc asc)."""
        d, s, _ = self.search_fuzzy_arrays(term, max_edits, prefix_len, max_expansions)
        return list(zip(d.tolist(), s.tolist()))

    def search_fuzzy_batch_arrays(self, terms, max_edits=2, prefix_len=0, max_expansions=50, cap=None):
        """(docs uint32[], scores float32[], hit offsets uint64[n + 1], n_expanded uint32[n], ms_device) of
        tfidf_search_fuzzy_batch; term i's hits are [offsets[i], offsets[i + 1])."""
        return _fuzzy_search_arrays(L.load().tfidf_search_fuzzy_batch, self._h, terms, max_edits, prefix_len,
                                    max_expansions, cap)

    def search_fuzzy_batch(self, terms, max_edits=2, prefix_len=0, max_expansions=50):
        """[search_fuzzy(t, ...) for t in terms] in one pass."""
        return _fuzzy_search_lists(self.search_fuzzy_batch_arrays(terms, max_edits, prefix_len, max_expansions))

    def wildcard_terms(self, pattern: bytes, max_out=10):
        """([(term bytes, df)], n_matched): the vocabulary terms matching the
        wildcard pattern (``*`` any run of code points, ``?`` one code point,
        ``\\x`` the literal x), df descending then bytes; at most max_out
        (1..1024) of the n_matched there are (tfidf_wildcard_terms)."""
        return _wildcard_terms_single(L.load().tfidf_wildcard_terms, self._h, pattern, max_out)

    def wildcard_terms_batch(self, patterns, max_out=10):
        """[wildcard_terms(p, max_out) for p in patterns] from one pass over
        the dictionary per chunk of patterns (tfidf_wildcard_terms_batch)."""
        return _wildcard_term_lists(_wildcard_terms_arrays(L.load().tfidf_wildcard_terms_batch, self._h, patterns,
                                                           max_out))

    def search_wildcard(self, pattern: bytes):
        """(ascending doc ids, n_matched): the live documents holding a term
        that matches the pattern; every hit scores 1.0, and no clause limit
        applies (tfidf_search_wildcard)."""
        return _wildcard_docs_single(L.load().tfidf_search_wildcard, self._h, pattern)

    def search_wildcard_batch_arrays(self, patterns, cap=None):
        """(doc ids uint32[], hit offsets uint64[n + 1], n_matched uint64[n], ms_device) of tfidf_search_wildcard_batch."""
        return _wildcard_docs_arrays(L.load().tfidf_search_wildcard_batch, self._h, patterns, cap)

    def search_wildcard_batch(self, patterns):
        """[search_wildcard(p) for p in patterns] (tfidf_search_wildcard_batch)."""
        return _wildcard_doc_lists(self.search_wildcard_batch_arrays(patterns))

    def last_wildcard_stats(self):
        """(dictionary scans, (pattern, term) matches, union chunks) of the
        last wildcard call on this index or one of its readers
        (tfidf_last_wildcard_stats)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_last_wildcard_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def regex_terms(self, pattern: bytes, max_out=10):
        """([(term bytes, df)], n_matched): the vocabulary terms that belong to
        the regular expression's language (Lucene's RegExp syntax, matched over
        code points, the pattern not lower-cased), df descending then bytes;
        at most max_out (1..1024) of the n_matched there are.  A syntax error
        raises E_QUERY_SYNTAX, ``<`` or a too complex pattern
        E_UNSUPPORTED_QUERY (tfidf_regex_terms)."""
        return _wildcard_terms_single(L.load().tfidf_regex_terms, self._h, pattern, max_out)

    def regex_terms_batch(self, patterns, max_out=10):
        """[regex_terms(p, max_out) for p in patterns] from one pass over the
        dictionary per chunk of patterns' tables (tfidf_regex_terms_batch)."""
        return _wildcard_term_lists(_wildcard_terms_arrays(L.load().tfidf_regex_terms_batch, self._h, patterns,
                                                           max_out))

    def search_regex(self, pattern: bytes):
        """(ascending doc ids, n_matched): the live documents holding a term of
        the pattern's language; every hit scores 1.0, and no clause limit
        applies (tfidf_search_regex)."""
        return _wildcard_docs_single(L.load().tfidf_search_regex, self._h, pattern)

    def search_regex_batch_arrays(self, patterns, cap=None):
        """(doc ids uint32[], hit offsets uint64[n + 1], n_matched uint64[n], ms_device) of tfidf_search_regex_batch."""
        return _wildcard_docs_arrays(L.load().tfidf_search_regex_batch, self._h, patterns, cap)

    def search_regex_batch(self, patterns):
        """[search_regex(p) for p in patterns] (tfidf_search_regex_batch)."""
        return _wildcard_doc_lists(self.search_regex_batch_arrays(patterns))

    def last_regex_stats(self):
        """(dictionary scans, (pattern, term) matches, union chunks, bytes of
        staged DFA tables) of the last regex call on this index or one of its
        readers (tfidf_last_regex_stats)."""
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_last_regex_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def last_fuzzy_chunks(self):
        """(dictionary scans, candidate chunks) of the last fuzzy lookup on
        this index or one of its readers (tfidf_last_fuzzy_chunks)."""
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_last_fuzzy_chunks(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def search_phrase(self, phrase: bytes):
        """[(doc, score, freq)] of the documents that hold the analysed terms
        of ``phrase`` next to each other in order (tfidf_search_phrase): freq
        counts every start position, score is BM25 over freq with the summed
        idf of the positions; (score desc, doc asc).  The bytes are text, not
        a query: operators and quotes are analysed away."""
        return _phrase_single(L.load().tfidf_search_phrase, self._h, phrase)

    def search_phrase_batch_arrays(self, phrases, cap=None):
        """(docs uint32[], scores float32[], freqs uint32[], offsets uint64[n_p + 1])
        of tfidf_search_phrase_batch; phrase i's hits are [offsets[i], offsets[i + 1])."""
        return _phrase_batch_arrays(L.load().tfidf_search_phrase_batch, self._h, phrases, cap)

    def search_phrase_batch(self, phrases):
        """[search_phrase(p) for p in phrases] in one pass; a phrase that is
        not UTF-8 has no hits."""
        return _phrase_lists(*self.search_phrase_batch_arrays(phrases))

    def search_phrase_slop(self, phrase: bytes, slop: int):
        """search_phrase with Lucene's slop (tfidf_search_phrase_slop): [(doc,
        score, freq)] with the float frequency of SloppyPhraseMatcher, the sum
        of 1 / (1 + matchLength) over the matches within ``slop``; slop 0 is
        search_phrase with freq as a float.  With slop > 0 a phrase that
        repeats a term or has more than 64 terms is E_UNSUPPORTED_QUERY."""
        return _phrase_single(L.load().tfidf_search_phrase_slop, self._h, phrase, int(slop))

    def search_phrase_slop_batch_arrays(self, phrases, slops, cap=None):
        """(docs uint32[], scores float32[], freqs float32[], offsets uint64[])
        of tfidf_search_phrase_slop_batch: phrase i is searched with slops[i]."""
        return _phrase_batch_arrays(L.load().tfidf_search_phrase_slop_batch, self._h, phrases, cap, slops=slops)

    def search_phrase_slop_batch(self, phrases, slops):
        """[search_phrase_slop(p, s) for p, s in zip(phrases, slops)] in one pass."""
        return _phrase_lists(*self.search_phrase_slop_batch_arrays(phrases, slops))

    def last_phrase_stats(self):
        """(candidate rows scanned, row chunks) of the last phrase search on
        this index or one of its readers (tfidf_last_phrase_stats)."""
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_last_phrase_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def search_compound_batch_arrays(self, queries, cap=None):
        """(docs uint32[], scores float32[], hit offsets uint64[n + 1], ms_device)
        of tfidf_search_compound_batch.  A query is a list of clauses (occur,
        kind, payload, params...): see must / should / must_not / filter_ and
        text / phrase / wildcard / regex / fuzzy of this module."""
        return _compound_arrays(L.load().tfidf_search_compound_batch, self._h, queries, cap)

    def search_compound_batch(self, queries):
        """Per query every hit [(doc, score)] of the Boolean combination of its
        clauses (Lucene's flat BooleanQuery), score descending, doc ascending."""
        return _compound_lists(self.search_compound_batch_arrays(queries))

    def search_compound(self, clauses):
        """search_compound_batch([clauses])[0]."""
        return self.search_compound_batch([clauses])[0]

    def search_nested_batch_arrays(self, queries, cap=None):
        """(docs uint32[], scores float32[], hit offsets uint64[n_q + 1], ms_device)
        of tfidf_search_nested_batch.  A query is a group(children,
        min_should_match) whose children are occurred clauses or occurred groups
        (at most 64 nodes, groups nested at most 4 deep), or a plain list of
        occurred clauses, which is a root group with min_should_match 0."""
        return _compound_arrays(L.load().tfidf_search_nested_batch, self._h, queries, cap, arrays=_qnode_arrays)

    def search_nested_batch(self, queries):
        """Per query [(doc, score)]: every hit of the clause tree, a group
        combining its children by the flat rule with its min_should_match, score
        descending, doc ascending."""
        return _compound_lists(self.search_nested_batch_arrays(queries))

    def search_nested(self, query):
        """search_nested_batch([query])[0]."""
        return self.search_nested_batch([query])[0]

    def last_compound_stats(self):
        """(clause-row entries, chunks, (query, block) pairs, combine pass ms) of
        the last compound call on this index or one of its readers
        (tfidf_last_compound_stats, tfidf_last_compound_ms)."""
        a, b, c, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        L.check(L.load().tfidf_last_compound_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        L.check(L.load().tfidf_last_compound_ms(self._h, C.byref(ms)))
        return a.value, b.value, c.value, ms.value

    def more_like_this(self, doc, k=10, exclude_seed=True, **params):
        """[(doc, score)]: the top ``k`` of the disjunction of document
        ``doc``'s interesting terms (Lucene's MoreLikeThis on the index's own
        row of the seed; tfidf_more_like_this), scored as ``search`` scores
        it; without the seed itself unless ``exclude_seed`` is False.
        ``params``: min_tf, min_df, max_df, max_terms (mlt_params)."""
        return _mlt_single(L.load().tfidf_more_like_this, self._h, doc, k, exclude_seed, mlt_params(**params))

    def more_like_this_batch_arrays(self, docs, k=10, exclude_seed=True, **params):
        """(docs uint32[n, k], scores float32[n, k], counts uint32[n]) of tfidf_more_like_this_batch."""
        return _mlt_batch_arrays(L.load().tfidf_more_like_this_batch, self._h, docs, k, exclude_seed,
                                 mlt_params(**params))

    def more_like_this_batch(self, docs, k=10, exclude_seed=True, **params):
        """[more_like_this(d, ...) for d in docs] from one device pass over the seeds' rows and one scoring batch."""
        return _topk_lists(*self.more_like_this_batch_arrays(docs, k, exclude_seed, **params))

    def mlt_terms_batch_arrays(self, docs, term_cap=None, bytes_cap=None, **params):
        """(term offsets uint64[n + 1], n_candidates uint64[n], blob offsets
        uint64[m + 1], term blob, tf uint32[m], df uint32[m], score float32[m])
        of tfidf_mlt_terms_batch; seed i's terms are [offsets[i], offsets[i + 1])."""
        return _mlt_terms_arrays(L.load().tfidf_mlt_terms_batch, self._h, docs, mlt_params(**params), term_cap,
                                 bytes_cap)

    def mlt_terms_batch(self, docs, **params):
        """Per seed ([(term bytes, tf, df, score)], n_candidates): its
        interesting terms in selection order (score descending, then bytes)
        and the candidates there were before the cut to max_terms."""
        return _mlt_terms_lists(self.mlt_terms_batch_arrays(docs, **params))

    def mlt_terms_arrays(self, doc, **params):
        return self.mlt_terms_batch_arrays([doc], **params)

    def mlt_terms(self, doc, **params):
        """mlt_terms_batch([doc])[0]."""
        return self.mlt_terms_batch([doc], **params)[0]

    def last_mlt_stats(self):
        """(forward-row entries scanned, candidate chunks) of the last
        more-like-this call on this index or one of its readers (tfidf_last_mlt_stats)."""
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_last_mlt_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_hash_attempt(self, attempt):
        """Seed attempt (0..3) the following commits start from (tfidf_set_hash_attempt)."""
        L.check(L.load().tfidf_set_hash_attempt(self._h, attempt))

    def commit_timing(self):
        t = L.CommitTiming()
        L.check(L.load().tfidf_get_commit_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in L.CommitTiming._fields_}

    def commit_tokenized_docs(self):
        """What the last commit tokenized: {"docs": n, "was_full": bool} (tfidf_commit_tokenized_docs)."""
        n, full = C.c_uint64(), C.c_uint32()
        L.check(L.load().tfidf_commit_tokenized_docs(self._h, C.byref(n), C.byref(full)))
        return {"docs": n.value, "was_full": bool(full.value)}

    def commit_inverted_blocks(self):
        """What the last commit's inversion built: blocks [first_block, n_blocks); remapped: the kept
        count rows moved to a wider column layout (tfidf_commit_inverted_blocks)."""
        f, n, r = C.c_uint32(), C.c_uint32(), C.c_uint32()
        L.check(L.load().tfidf_commit_inverted_blocks(self._h, C.byref(f), C.byref(n), C.byref(r)))
        return {"first_block": f.value, "n_blocks": n.value, "remapped": r.value}

    def commit_inversion_shape(self):
        """The launch shape of the last commit's inversion: document slices per (block, range) tile and
        workgroups per block row in the row scan (tfidf_commit_inversion_shape)."""
        s, p = C.c_uint32(), C.c_uint32()
        L.check(L.load().tfidf_commit_inversion_shape(self._h, C.byref(s), C.byref(p)))
        return {"slices": s.value, "scan_parts": p.value}

    def commit_inversion_fused(self):
        """Whether the last commit took its lone inverted block's counts, df, offsets and base in one
        launch (tfidf_commit_inversion_fused)."""
        f = C.c_uint32()
        L.check(L.load().tfidf_commit_inversion_fused(self._h, C.byref(f)))
        return bool(f.value)

    def commit_host_profile(self):
        """The host side of the last commit (tfidf_commit_host_profile): host times in ms since the call
        began, stream synchronisations, and per mirror (dict, df, crank) its form ("none" / "delta" /
        "whole") and the bytes copied device -> host."""
        p = L.HostProfile()
        L.check(L.load().tfidf_commit_host_profile(self._h, C.byref(p)))
        out = {f: getattr(p, f) for f, _ in L.HostProfile._fields_}
        for m in ("mirror_dict", "mirror_df", "mirror_crank"):
            out[m] = L.MIRROR_FORMS[out[m]]
        return out

    def stats(self):
        s = L.IndexStats()
        L.check(L.load().tfidf_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in L.IndexStats._fields_}

    # -- search (Worker.searchIndex) ------------------------------------------
    def search(self, query: bytes, k=0):
        """[(doc, float score)] in (score desc, doc asc); k == 0 -> all hits."""
        if k == 0:                              # sized by the snapshot the search runs on
            with self.reader() as rd:
                return rd.search(query, 0)
        lib = L.load()
        docs = np.zeros(k, np.uint32)
        scores = np.zeros(k, np.float32)
        n = C.c_uint64()
        rc = lib.tfidf_search(self._h, query, len(query), k, L.ptr(docs, C.c_uint32), L.ptr(scores, C.c_float),
                              k, C.byref(n))
        L.check(rc)
        m = n.value
        return list(zip(docs[:m].tolist(), scores[:m].tolist()))

    def reader(self):
        """A Reader on the snapshot published now (tfidf_reader_open)."""
        return Reader(self)

    def search_coalesced(self, query: bytes, k, wait_us=50, cap=None):
        """Thread-safe search that shares one batched scoring launch with the
        searches other threads issue at the same time (tfidf_search_coalesced).
        k == 0: all hits (the reference's request shape, Worker.java:230), in
        ``cap`` result slots (default: the documents committed now)."""
        if cap is None:
            cap = k if k else max(self.stats()["num_docs"], 1)
        docs = np.empty(max(cap, 1), np.uint32)
        scores = np.empty(max(cap, 1), np.float32)
        n = C.c_uint64()
        L.check(L.load().tfidf_search_coalesced(self._h, query, len(query), k, L.ptr(docs, C.c_uint32),
                                                L.ptr(scores, C.c_float), cap, C.byref(n), wait_us))
        m = n.value
        return list(zip(docs[:m].tolist(), scores[:m].tolist()))

    def search_batch_all_arrays(self, queries, cap=None):
        """Every hit of each query in one pass (tfidf_search_batch_all):
        (docs uint32[], scores float32[], offsets uint64[n_q + 1]); query i's
        hits are [offsets[i], offsets[i + 1]), in (score desc, doc asc).  ``cap``:
        result slots of the first attempt; the call is repeated once with the
        size the library reports when they do not suffice."""
        if cap is None:
            cap = min(65536 * max(len(queries), 1), 1 << 24)
        return _batch_all_arrays(L.load().tfidf_search_batch_all, self._h, queries, cap)

    def search_batch_all(self, queries):
        """[search(q, 0) for q in queries] in one pass; a query that does not
        parse has no hits (as in search_batch)."""
        return _hit_lists(*self.search_batch_all_arrays(queries))

    def search_all_arrays(self, query: bytes):
        """All hits as (doc uint32[], score float32[]) in (score desc, doc asc)
        — searcher.search(q, Integer.MAX_VALUE) without per-hit Python objects."""
        with self.reader() as rd:
            return rd.search_arrays(query, 0)

    def search_arrays(self, query: bytes, k):
        lib = L.load()
        docs = np.zeros(max(k, 1), np.uint32)
        scores = np.zeros(max(k, 1), np.float32)
        n = C.c_uint64()
        L.check(lib.tfidf_search(self._h, query, len(query), k, L.ptr(docs, C.c_uint32), L.ptr(scores, C.c_float),
                                 max(k, 1), C.byref(n)))
        return docs[:n.value], scores[:n.value]

    def search_batch(self, queries, k):
        """queries: list of bytes.  Returns (docs[n_q, k], scores[n_q, k], counts[n_q])."""
        nq = len(queries)
        offs = np.zeros(nq + 1, np.uint64)
        offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
        docs = np.zeros((nq, k), np.uint32)
        scores = np.zeros((nq, k), np.float32)
        counts = np.zeros(nq, np.uint32)
        L.check(L.load().tfidf_search_batch(self._h, b"".join(queries), L.ptr(offs, C.c_uint64), nq, k,
                                            L.ptr(docs, C.c_uint32), L.ptr(scores, C.c_float),
                                            L.ptr(counts, C.c_uint32)))
        return docs, scores, counts

    def search_batch_keys_device(self, queries, k, doc_base, d_keys):
        """n_q x k merge keys (score bits << 32 | ~(doc_base + doc)) into device memory d_keys."""
        nq = len(queries)
        offs = np.zeros(nq + 1, np.uint64)
        offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
        L.check(L.load().tfidf_search_batch_keys_device(self._h, b"".join(queries), L.ptr(offs, C.c_uint64), nq, k,
                                                        doc_base, C.c_void_p(d_keys)))

    def search_all_keys_device(self, query: bytes, doc_base, d_keys, cap):
        """Every hit's merge key, ordered, into device memory (cap >= num_docs); -> #hits."""
        n = C.c_uint64()
        L.check(L.load().tfidf_search_all_keys_device(self._h, query, len(query), doc_base, C.c_void_p(d_keys), cap,
                                                      C.byref(n)))
        return n.value

    def set_stream(self, stream):
        """Issue device work on the caller's HIP stream (int handle); None = the index's own stream."""
        L.check(L.load().tfidf_set_stream(self._h, L.OWN_STREAM if stream is None else C.c_void_p(stream)))

    def set_query_timing(self, on: bool):
        """HIP-event device timing of searches (on by default; off for serving)."""
        L.check(L.load().tfidf_set_query_timing(self._h, 1 if on else 0))

    def last_search_ms(self):
        a, b = C.c_float(), C.c_float()
        L.check(L.load().tfidf_last_search_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- inspection -----------------------------------------------------------
    def doc_key(self, doc):
        buf = C.create_string_buffer(4096)
        n = C.c_uint64()
        L.check(L.load().tfidf_doc_key(self._h, doc, buf, 4096, C.byref(n)))
        return buf.raw[:n.value]

    def doc_keys(self):
        """Every committed document's key: (uint8 blob, uint64 offsets[num_docs + 1])."""
        with self.reader() as rd:
            return rd.doc_keys()

    def malformed_docs(self):
        """Committed doc ids whose bytes are not valid UTF-8 (indexed empty)."""
        n = self.stats()["malformed_docs"]
        out = np.zeros(max(n, 1), np.uint64)
        m = C.c_uint64()
        L.check(L.load().tfidf_malformed_docs(self._h, L.ptr(out, C.c_uint64), len(out), C.byref(m)))
        return out[:m.value].tolist()

    def doc_len(self, doc):
        ln, nm = C.c_uint32(), C.c_uint8()
        L.check(L.load().tfidf_doc_len(self._h, doc, C.byref(ln), C.byref(nm)))
        return ln.value, nm.value

    def doc_terms(self, doc):
        ln, _ = self.doc_len(doc)
        cap = ln + 1
        tfs = np.zeros(cap, np.uint32)
        n = C.c_uint64()
        for per in (48, 1024):                   # term strings: up to 255 UTF-16 units (<= 1020 bytes)
            buf = C.create_string_buffer(cap * per + 64)
            rc = L.load().tfidf_doc_terms(self._h, doc, buf, len(buf), L.ptr(tfs, C.c_uint32), cap, C.byref(n))
            if rc != L.E_BUFFER:
                break
        L.check(rc)
        terms = buf.raw.split(b"\0")[:n.value]
        return dict(zip(terms, tfs[:n.value].tolist()))

    def df(self, term: bytes):
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_term_df(self._h, term, len(term), C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- GLOBAL statistics ------------------------------------------------------
    def vocab_size(self):
        n = C.c_uint64()
        L.check(L.load().tfidf_vocab_size(self._h, C.byref(n)))
        return n.value

    def vocab_export(self):
        """(keys uint64 [n, 2] (lo, hi) sorted by (hi, lo), df_local uint32 [n],
        df_effective uint32 [n]): the vocabulary with the statistics in force."""
        n = self.vocab_size()
        keys = np.zeros((max(n, 1), 2), np.uint64)
        dl = np.zeros(max(n, 1), np.uint32)
        de = np.zeros(max(n, 1), np.uint32)
        m = C.c_uint64()
        L.check(L.load().tfidf_vocab_export(self._h, L.ptr(keys, C.c_uint64), L.ptr(dl, C.c_uint32),
                                            L.ptr(de, C.c_uint32), len(dl), C.byref(m)))
        return keys[:m.value], dl[:m.value], de[:m.value]

    def vocab_export_device(self, d_keys, d_df, cap):
        n = C.c_uint64()
        L.check(L.load().tfidf_vocab_export_device(self._h, C.c_void_p(d_keys), C.c_void_p(d_df), cap, C.byref(n)))
        return n.value

    def vocab_canonicalize_device(self, d_all_keys, n_all, d_df_canon, cap):
        n = C.c_uint64()
        L.check(L.load().tfidf_vocab_canonicalize_device(self._h, C.c_void_p(d_all_keys), n_all,
                                                         C.c_void_p(d_df_canon), cap, C.byref(n)))
        return n.value

    def set_global_stats_device(self, d_df_canon, n_canon, doc_count, sum_ttf):
        L.check(L.load().tfidf_set_global_stats_device(self._h, C.c_void_p(d_df_canon), n_canon, doc_count,
                                                       sum_ttf))

    def vocab_partition_device(self, n_ranks, d_records, cap, d_counts):
        """Records (lo, hi, df) grouped by owner rank into d_records, per-owner
        counts (u64) into d_counts -> n records.  Asynchronous on a stream set
        by set_stream (the buffers must then stay live until that stream
        reaches the work: torch tensors of that stream do); on the index's own
        stream it returns with the work done."""
        n = C.c_uint64()
        L.check(L.load().tfidf_vocab_partition_device(self._h, n_ranks, C.c_void_p(d_records), cap,
                                                      C.c_void_p(d_counts), C.byref(n)))
        return n.value

    def vocab_reduce_device(self, d_records, n, d_df_out, d_n_unique=None):
        """Owner side: summed df per received record (asynchronous on a
        set_stream stream, like vocab_partition_device)."""
        L.check(L.load().tfidf_vocab_reduce_device(self._h, C.c_void_p(d_records), n, C.c_void_p(d_df_out),
                                                   C.c_void_p(d_n_unique) if d_n_unique else None))

    def set_global_df_device(self, d_df, n, doc_count, sum_ttf):
        L.check(L.load().tfidf_set_global_df_device(self._h, C.c_void_p(d_df), n, doc_count, sum_ttf))

    def set_global_stats(self, keys_lohi, df, doc_count, sum_ttf):
        keys_lohi = np.ascontiguousarray(keys_lohi, np.uint64).reshape(-1)
        df = np.ascontiguousarray(df, np.uint64)
        L.check(L.load().tfidf_set_global_stats(self._h, L.ptr(keys_lohi, C.c_uint64), L.ptr(df, C.c_uint64),
                                                len(df), doc_count, sum_ttf))

    def clear_global_stats(self):
        L.check(L.load().tfidf_clear_global_stats(self._h))


def sort_names(blob, offsets):
    """Permutation of the names blob[offsets[i]:offsets[i+1]] in String.compareTo order."""
    n = len(offsets) - 1
    blob = np.ascontiguousarray(blob, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    perm = np.zeros(max(n, 1), np.uint64)
    L.check(L.load().tfidf_sort_names(blob.tobytes(), L.ptr(offsets, C.c_uint64), n, L.ptr(perm, C.c_uint64)))
    return perm[:n]


def leader_merge(responses):
    """Leader.start merge via the C ABI: list (worker order) of lists of
    (name bytes, double) -> [(name, sum)] ordered by name."""
    flat = [x for r in responses for x in r]
    n = len(flat)
    if n == 0:
        return []
    names = b"".join(nm for nm, _ in flat)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(nm) for nm, _ in flat], dtype=np.uint64)
    sc = np.array([s for _, s in flat], np.float64)
    first = np.zeros(n, np.uint64)
    sums = np.zeros(n, np.float64)
    m = C.c_uint64()
    L.check(L.load().tfidf_leader_merge(names, L.ptr(offs, C.c_uint64), n, L.ptr(sc, C.c_double),
                                        L.ptr(first, C.c_uint64), L.ptr(sums, C.c_double), C.byref(m)))
    return [(flat[int(first[i])][0], float(sums[i])) for i in range(m.value)]


class Reader:
    """A pinned snapshot (tfidf_reader_*): Worker.java:223 opens a
    DirectoryReader on the last commit per request and reads the hits' stored
    "path" from it (:234-238); searches and doc keys here all see the commit
    published when the reader was opened, whatever commits follow."""

    def __init__(self, index):
        self._h = C.c_void_p()
        L.check(L.load().tfidf_reader_open(index._h, C.byref(self._h)))
        g, n = C.c_uint64(), C.c_uint64()
        L.check(L.load().tfidf_reader_info(self._h, C.byref(g), C.byref(n)))
        self.generation, self.num_docs = g.value, n.value

    def close(self):
        if self._h:
            L.load().tfidf_reader_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_arrays(self, query: bytes, k=0):
        cap = max(k if k else self.num_docs, 1)
        docs = np.empty(cap, np.uint32)
        scores = np.empty(cap, np.float32)
        n = C.c_uint64()
        L.check(L.load().tfidf_reader_search(self._h, query, len(query), k, L.ptr(docs, C.c_uint32),
                                             L.ptr(scores, C.c_float), cap, C.byref(n)))
        return docs[:n.value], scores[:n.value]

    def search(self, query: bytes, k=0):
        d, s = self.search_arrays(query, k)
        return list(zip(d.tolist(), s.tolist()))

    def search_batch_all_arrays(self, queries, cap=None):
        """ShardIndex.search_batch_all_arrays on this reader's snapshot."""
        if cap is None:
            cap = min(65536 * max(len(queries), 1), 1 << 24)
        return _batch_all_arrays(L.load().tfidf_reader_search_batch_all, self._h, queries, cap)

    def search_batch_all(self, queries):
        return _hit_lists(*self.search_batch_all_arrays(queries))

    def doc_key(self, doc):
        buf = C.create_string_buffer(4096)
        n = C.c_uint64()
        L.check(L.load().tfidf_reader_doc_key(self._h, doc, buf, 4096, C.byref(n)))
        return buf.raw[:n.value]

    def doc_text(self, doc):
        """The document's bytes in this reader's snapshot."""
        return _doc_text(L.load().tfidf_reader_doc_text, self._h, doc)

    def matches_arrays(self, query: bytes, docs, cap=None):
        return _matches_arrays(L.load().tfidf_reader_matches, self._h, query, docs, cap)

    def matches(self, query: bytes, docs):
        """ShardIndex.matches on this reader's snapshot."""
        return _match_lists(*self.matches_arrays(query, docs)[:4])

    def snippets_arrays(self, query: bytes, docs, max_bytes=160, m_cap=None):
        return _snippets_arrays(L.load().tfidf_reader_snippets, self._h, query, docs, max_bytes, m_cap)

    def snippets(self, query: bytes, docs, max_bytes=160):
        """ShardIndex.snippets on this reader's snapshot."""
        return _snippet_lists(self.snippets_arrays(query, docs, max_bytes))

    def matches_batch_arrays(self, queries, docs_per_query, cap=None):
        """(starts, lens, ordinals, match offsets[R + 1], doc offsets[n_q + 1], ms_device) of tfidf_reader_matches_batch."""
        return _matches_batch_arrays(L.load().tfidf_reader_matches_batch, self._h, queries, docs_per_query, cap)

    def matches_batch(self, queries, docs_per_query):
        """ShardIndex.matches_batch on this reader's snapshot."""
        a = self.matches_batch_arrays(queries, docs_per_query)
        return _per_query(_match_lists(*a[:4]), a[4])

    def snippets_batch_arrays(self, queries, docs_per_query, max_bytes=160, m_cap=None):
        """snippets_arrays' eight results over all rows, then doc offsets[n_q + 1] (tfidf_reader_snippets_batch)."""
        return _snippets_batch_arrays(L.load().tfidf_reader_snippets_batch, self._h, queries, docs_per_query, max_bytes,
                                      m_cap)

    def snippets_batch(self, queries, docs_per_query, max_bytes=160):
        """ShardIndex.snippets_batch on this reader's snapshot."""
        a = self.snippets_batch_arrays(queries, docs_per_query, max_bytes)
        return _per_query(_snippet_lists(a[:8]), a[8])

    def fuzzy_terms(self, term: bytes, max_edits=2, prefix_len=0, max_out=10):
        """ShardIndex.fuzzy_terms on this reader's snapshot."""
        return _fuzzy_single(L.load().tfidf_reader_fuzzy_terms, self._h, term, max_edits, prefix_len, max_out)

    def wildcard_terms(self, pattern: bytes, max_out=10):
        """ShardIndex.wildcard_terms on this reader's snapshot."""
        return _wildcard_terms_single(L.load().tfidf_reader_wildcard_terms, self._h, pattern, max_out)

    def wildcard_terms_batch(self, patterns, max_out=10):
        """ShardIndex.wildcard_terms_batch on this reader's snapshot."""
        return _wildcard_term_lists(_wildcard_terms_arrays(L.load().tfidf_reader_wildcard_terms_batch, self._h,
                                                           patterns, max_out))

    def search_wildcard(self, pattern: bytes):
        """ShardIndex.search_wildcard on this reader's snapshot."""
        return _wildcard_docs_single(L.load().tfidf_reader_search_wildcard, self._h, pattern)

    def search_wildcard_batch_arrays(self, patterns, cap=None):
        """(doc ids uint32[], hit offsets uint64[n + 1], n_matched uint64[n], ms_device) of tfidf_reader_search_wildcard_batch."""
        return _wildcard_docs_arrays(L.load().tfidf_reader_search_wildcard_batch, self._h, patterns, cap)

    def search_wildcard_batch(self, patterns):
        """ShardIndex.search_wildcard_batch on this reader's snapshot."""
        return _wildcard_doc_lists(self.search_wildcard_batch_arrays(patterns))

    def regex_terms(self, pattern: bytes, max_out=10):
        """ShardIndex.regex_terms on this reader's snapshot."""
        return _wildcard_terms_single(L.load().tfidf_reader_regex_terms, self._h, pattern, max_out)

    def regex_terms_batch(self, patterns, max_out=10):
        """ShardIndex.regex_terms_batch on this reader's snapshot."""
        return _wildcard_term_lists(_wildcard_terms_arrays(L.load().tfidf_reader_regex_terms_batch, self._h,
                                                           patterns, max_out))

    def search_regex(self, pattern: bytes):
        """ShardIndex.search_regex on this reader's snapshot."""
        return _wildcard_docs_single(L.load().tfidf_reader_search_regex, self._h, pattern)

    def search_regex_batch_arrays(self, patterns, cap=None):
        """(doc ids uint32[], hit offsets uint64[n + 1], n_matched uint64[n], ms_device) of tfidf_reader_search_regex_batch."""
        return _wildcard_docs_arrays(L.load().tfidf_reader_search_regex_batch, self._h, patterns, cap)

    def search_regex_batch(self, patterns):
        """ShardIndex.search_regex_batch on this reader's snapshot."""
        return _wildcard_doc_lists(self.search_regex_batch_arrays(patterns))

    def fuzzy_terms_batch_arrays(self, terms, max_edits=2, prefix_len=0, max_out=10):
        """(cand offsets, n_within, term offsets, term blob, df, dist, ms_device) of tfidf_reader_fuzzy_terms_batch."""
        return _fuzzy_batch_arrays(L.load().tfidf_reader_fuzzy_terms_batch, self._h, terms, max_edits, prefix_len,
                                   max_out)

    def fuzzy_terms_batch(self, terms, max_edits=2, prefix_len=0, max_out=10):
        """ShardIndex.fuzzy_terms_batch on this reader's snapshot."""
        return _fuzzy_lists(self.fuzzy_terms_batch_arrays(terms, max_edits, prefix_len, max_out))

    def fuzzy_expand(self, term: bytes, max_edits=2, prefix_len=0, max_expansions=50):
        """ShardIndex.fuzzy_expand on this reader's snapshot."""
        return _fuzzy_expand_single(L.load().tfidf_reader_fuzzy_expand, self._h, term, max_edits, prefix_len,
                                    max_expansions)

    def fuzzy_expand_batch_arrays(self, terms, max_edits=2, prefix_len=0, max_expansions=50):
        """ShardIndex.fuzzy_expand_batch_arrays on this reader's snapshot."""
        return _fuzzy_expand_arrays(L.load().tfidf_reader_fuzzy_expand_batch, self._h, terms, max_edits, prefix_len,
                                    max_expansions)

    def fuzzy_expand_batch(self, terms, max_edits=2, prefix_len=0, max_expansions=50):
        """ShardIndex.fuzzy_expand_batch on this reader's snapshot."""
        return _fuzzy_expand_lists(self.fuzzy_expand_batch_arrays(terms, max_edits, prefix_len, max_expansions))

    def search_fuzzy_arrays(self, term: bytes, max_edits=2, prefix_len=0, max_expansions=50):
        """ShardIndex.search_fuzzy_arrays on this reader's snapshot."""
        return _fuzzy_search_single(L.load().tfidf_reader_search_fuzzy, self._h, term, max_edits, prefix_len,
                                    max_expansions)

    def search_fuzzy(self, term: bytes, max_edits=2, prefix_len=0, max_expansions=50):
        """ShardIndex.search_fuzzy on this reader's snapshot."""
        d, s, _ = self.search_fuzzy_arrays(term, max_edits, prefix_len, max_expansions)
        return list(zip(d.tolist(), s.tolist()))

    def search_fuzzy_batch_arrays(self, terms, max_edits=2, prefix_len=0, max_expansions=50, cap=None):
        """ShardIndex.search_fuzzy_batch_arrays on this reader's snapshot."""
        return _fuzzy_search_arrays(L.load().tfidf_reader_search_fuzzy_batch, self._h, terms, max_edits, prefix_len,
                                    max_expansions, cap)

    def search_fuzzy_batch(self, terms, max_edits=2, prefix_len=0, max_expansions=50):
        """ShardIndex.search_fuzzy_batch on this reader's snapshot."""
        return _fuzzy_search_lists(self.search_fuzzy_batch_arrays(terms, max_edits, prefix_len, max_expansions))

    def search_phrase(self, phrase: bytes):
        """ShardIndex.search_phrase on this reader's snapshot."""
        return _phrase_single(L.load().tfidf_reader_search_phrase, self._h, phrase)

    def search_phrase_batch_arrays(self, phrases, cap=None):
        """ShardIndex.search_phrase_batch_arrays on this reader's snapshot."""
        return _phrase_batch_arrays(L.load().tfidf_reader_search_phrase_batch, self._h, phrases, cap)

    def search_phrase_batch(self, phrases):
        """ShardIndex.search_phrase_batch on this reader's snapshot."""
        return _phrase_lists(*self.search_phrase_batch_arrays(phrases))

    def search_phrase_slop(self, phrase: bytes, slop: int):
        """ShardIndex.search_phrase_slop on this reader's snapshot."""
        return _phrase_single(L.load().tfidf_reader_search_phrase_slop, self._h, phrase, int(slop))

    def search_phrase_slop_batch_arrays(self, phrases, slops, cap=None):
        """ShardIndex.search_phrase_slop_batch_arrays on this reader's snapshot."""
        return _phrase_batch_arrays(L.load().tfidf_reader_search_phrase_slop_batch, self._h, phrases, cap, slops=slops)

    def search_phrase_slop_batch(self, phrases, slops):
        """ShardIndex.search_phrase_slop_batch on this reader's snapshot."""
        return _phrase_lists(*self.search_phrase_slop_batch_arrays(phrases, slops))

    def search_compound_batch_arrays(self, queries, cap=None):
        """ShardIndex.search_compound_batch_arrays on this reader's snapshot."""
        return _compound_arrays(L.load().tfidf_reader_search_compound_batch, self._h, queries, cap)

    def search_compound_batch(self, queries):
        """ShardIndex.search_compound_batch on this reader's snapshot."""
        return _compound_lists(self.search_compound_batch_arrays(queries))

    def search_compound(self, clauses):
        """ShardIndex.search_compound on this reader's snapshot."""
        return self.search_compound_batch([clauses])[0]

    def search_nested_batch_arrays(self, queries, cap=None):
        """ShardIndex.search_nested_batch_arrays on this reader's snapshot."""
        return _compound_arrays(L.load().tfidf_reader_search_nested_batch, self._h, queries, cap, arrays=_qnode_arrays)

    def search_nested_batch(self, queries):
        """ShardIndex.search_nested_batch on this reader's snapshot."""
        return _compound_lists(self.search_nested_batch_arrays(queries))

    def search_nested(self, query):
        """ShardIndex.search_nested on this reader's snapshot."""
        return self.search_nested_batch([query])[0]

    def more_like_this(self, doc, k=10, exclude_seed=True, **params):
        """ShardIndex.more_like_this on this reader's snapshot."""
        return _mlt_single(L.load().tfidf_reader_more_like_this, self._h, doc, k, exclude_seed, mlt_params(**params))

    def more_like_this_batch_arrays(self, docs, k=10, exclude_seed=True, **params):
        """ShardIndex.more_like_this_batch_arrays on this reader's snapshot."""
        return _mlt_batch_arrays(L.load().tfidf_reader_more_like_this_batch, self._h, docs, k, exclude_seed,
                                 mlt_params(**params))

    def more_like_this_batch(self, docs, k=10, exclude_seed=True, **params):
        """ShardIndex.more_like_this_batch on this reader's snapshot."""
        return _topk_lists(*self.more_like_this_batch_arrays(docs, k, exclude_seed, **params))

    def mlt_terms_batch_arrays(self, docs, term_cap=None, bytes_cap=None, **params):
        """ShardIndex.mlt_terms_batch_arrays on this reader's snapshot."""
        return _mlt_terms_arrays(L.load().tfidf_reader_mlt_terms_batch, self._h, docs, mlt_params(**params), term_cap,
                                 bytes_cap)

    def mlt_terms_batch(self, docs, **params):
        """ShardIndex.mlt_terms_batch on this reader's snapshot."""
        return _mlt_terms_lists(self.mlt_terms_batch_arrays(docs, **params))

    def mlt_terms_arrays(self, doc, **params):
        return self.mlt_terms_batch_arrays([doc], **params)

    def mlt_terms(self, doc, **params):
        """ShardIndex.mlt_terms on this reader's snapshot."""
        return self.mlt_terms_batch([doc], **params)[0]

    def doc_keys(self):
        lib = L.load()
        offs = np.zeros(self.num_docs + 1, np.uint64)
        need = C.c_uint64()
        rc = lib.tfidf_reader_doc_keys(self._h, None, 0, L.ptr(offs, C.c_uint64), C.byref(need))
        if rc not in (L.OK, L.E_BUFFER):
            L.check(rc)
        buf = C.create_string_buffer(max(need.value, 1))
        L.check(lib.tfidf_reader_doc_keys(self._h, buf, need.value, L.ptr(offs, C.c_uint64), C.byref(need)))
        return np.frombuffer(buf.raw[:need.value], np.uint8).copy(), offs
