"""Wildcard and prefix search on the device (tfidf_wildcard_terms[_batch],
tfidf_search_wildcard[_batch], the reader forms, Worker.search_prefix and
Worker.suggest_terms) against wildcard_ref.py, compared exactly: the same term
lists, df, n_matched and doc ids as brute force over the oracle's vocabulary
and documents.  The `dense` corpus is fuzzy_ref's (every string over {a, b, c}
of 1..6 letters with df 1..5, exact and hashed keys on both sides of their
limits, non-ASCII, Han, an emoji and a 255-unit term); the `block` corpus has 3
x 8192 - 5 short documents with chosen terms at block and bitmap word edges."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import wildcard_ref as W
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex, _key_arrays
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

INVERSIONS = [L.INVERSION_BLOCK, L.INVERSION_TERM]
HASHED = b"zqxjkvwypmnbghtrd"                       # 17 bytes: a hashed key
PATTERNS = [b"*", b"a*", b"*c", b"a?c*", b"??", b"abcab", HASHED[:12] + b"*", HASHED + b"*", W.LONG255[:40] + b"*",
            W.LONG255[:254] + b"?", b"caf?", b"", b"\xff*", b"?" * 256, b"*nop", b"ZQ*", "àé*".encode(), "*ñ".encode(),
            b"?", b"a*b*c", b"nothing*", b"*lmnop*", b"\\*", b"CAF*", b"x"]


@functools.lru_cache(maxsize=None)
def dense_sets():
    texts = W.dense_texts()
    ix = W.oracle_index(texts)
    sets = W.doc_term_sets(ix, len(texts))
    ix.close()
    return sets


@functools.lru_cache(maxsize=None)
def want_terms_all(p):
    return W.expected_terms(W.dense_vocab(), p, 1 << 30)


def want_terms(p, k):
    lst, n = want_terms_all(p)
    return lst[:k], n


@functools.lru_cache(maxsize=None)
def want_docs(p):
    return W.expected_docs(dense_sets(), W.dense_vocab(), p)


_state = {}


def index(inversion=L.INVERSION_BLOCK):
    """The committed dense index per inversion, shared by the tests (never changed)."""
    if inversion not in _state:
        g = ShardIndex(vocab_capacity_log2=16, inversion=inversion)
        texts = W.dense_texts()
        g.add_documents(texts, [b"d%05d" % i for i in range(len(texts))])
        g.commit()
        assert g.stats()["term_major"] == (1 if inversion == L.INVERSION_TERM else 0)
        _state[inversion] = g
    return _state[inversion]


def block_index(inversion):
    key = ("block", inversion)
    if key not in _state:
        g = ShardIndex(vocab_capacity_log2=12, inversion=inversion)
        g.add_documents(W.block_texts())
        g.commit()
        assert g.stats()["term_major"] == (1 if inversion == L.INVERSION_TERM else 0)
        _state[key] = g
    return _state[key]


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_term_lists_equal_the_reference(inversion):
    g = index(inversion)
    for k in (1, 5, 1024):
        got = g.wildcard_terms_batch(PATTERNS, k)
        assert len(got) == len(PATTERNS)
        for p, gt in zip(PATTERNS, got):
            assert gt == want_terms(p, k), (p[:40], k)
    # the fixture reaches its cases
    assert want_terms(b"*", 5)[1] == len(W.dense_vocab()) > 1024           # more terms than the scorer takes clauses
    assert [t for t, _ in want_terms(b"caf?", 5)[0]] == [b"cafe", "café".encode()]
    assert want_terms(HASHED + b"*", 5)[1] == 2 and want_terms(HASHED[:12] + b"*", 5)[1] == 3
    assert want_terms(W.LONG255[:40] + b"*", 5) == ([(W.LONG255, 2)], 1) == want_terms(W.LONG255[:254] + b"?", 5)
    assert want_terms(b"", 5) == want_terms(b"\xff*", 5) == want_terms(b"?" * 256, 5) == ([], 0)
    assert {W.HAN, W.EMOJI} <= {t for t, _ in want_terms(b"?", 1024)[0]}


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_document_sets_equal_the_reference(inversion):
    g = index(inversion)
    got = g.search_wildcard_batch(PATTERNS)
    assert len(got) == len(PATTERNS)
    for p, gd in zip(PATTERNS, got):
        assert gd == want_docs(p), p[:40]
    n = len(W.dense_texts())
    assert want_docs(b"*") == (list(range(n)), len(W.dense_vocab()))       # every document has a token
    assert 0 < len(want_docs(b"a?c*")[0]) < n and want_docs(b"nothing*") == ([], 0)


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_block_and_word_edges(inversion):
    g = block_index(inversion)
    got = g.search_wildcard_batch(W.BLOCK_PATTERNS)
    for p, gd in zip(W.BLOCK_PATTERNS, got):
        (docs, n), vocab = W.block_expected(p)
        assert gd == (docs, n), p
        assert g.wildcard_terms(p, 1024) == W.expected_terms(vocab, p, 1024)
    assert g.search_wildcard(b"edgeterm")[0] == W.EDGE_DOCS == [0, 31, 32, 63, 64, 8191, 8192, 16383, 3 * 8192 - 6]
    assert len(g.search_wildcard(b"*")[0]) == W.N_BLOCKS_DOCS


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_a_literal_pattern_is_the_term(inversion):
    g = index(inversion)
    for t in (b"abcab", b"a", W.CAFES[0], HASHED, W.LONG255, b"zzzz"):
        docs, n = g.search_wildcard(t)
        assert docs == sorted(d for d, _ in g.search(t, k=0))
        terms, m = g.wildcard_terms(t, 5)
        assert (terms, m) == ([(x, df) for x, df, _ in g.fuzzy_terms(t, 0)[0]], n)
        assert n == (1 if t != b"zzzz" else 0)


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_single_and_reader_forms_equal_the_batch_of_one(inversion):
    g = index(inversion)
    some = [b"a*", b"*", b"caf?", HASHED + b"*", b"", b"\xff*", b"nothing*", W.EMOJI]
    with g.reader() as rd:
        for p in some:
            wt, wd = want_terms(p, 5), want_docs(p)
            assert g.wildcard_terms(p, 5) == wt == rd.wildcard_terms(p, 5)
            assert g.wildcard_terms_batch([p], 5) == [wt] == rd.wildcard_terms_batch([p], 5)
            assert g.search_wildcard(p) == wd == rd.search_wildcard(p)
            assert g.search_wildcard_batch([p]) == [wd] == rd.search_wildcard_batch([p])
    assert g.wildcard_terms_batch([]) == [] == g.search_wildcard_batch([])  # n_p = 0 is legal
    assert g.last_wildcard_stats() == (0, 0, 0)


@pytest.mark.parametrize("inversion", INVERSIONS)
@pytest.mark.parametrize("knob,budget", [("TFIDF_WILDCARD_MATCH_BUDGET", "1"), ("TFIDF_WILDCARD_MATCH_BUDGET", "100"),
                                         ("TFIDF_WILDCARD_HIT_BUDGET", "1"), ("TFIDF_WILDCARD_HIT_BUDGET", "20000")])
def test_any_budget_gives_the_same_output(inversion, knob, budget, monkeypatch):
    g = index(inversion)
    whole_d = g.search_wildcard_batch_arrays(PATTERNS)
    scans, matches, unions = g.last_wildcard_stats()
    assert scans == 1 and unions == 1 and matches == sum(want_terms(p, 1)[1] for p in PATTERNS)
    whole_t = g.wildcard_terms_batch(PATTERNS, 5)
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    monkeypatch.setenv(knob, budget)
    split_d = g.search_wildcard_batch_arrays(PATTERNS)
    for a, b in zip(split_d[:3], whole_d[:3]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    s2, m2, u2 = g.last_wildcard_stats()
    assert (s2, m2) == (scans, matches) and u2 > unions
    if budget == "1":                                                       # every pattern with a term alone
        assert u2 == sum(1 for p in PATTERNS if want_terms(p, 1)[1])
    assert g.wildcard_terms_batch(PATTERNS, 5) == whole_t


def test_more_patterns_than_one_scan_stages():
    g = index()
    many = [b"%s*" % s[:3] for s in W.ABC[:300]] + [W.LONG255[:200] + b"*"] * 12
    got_t, got_d = g.wildcard_terms_batch(many, 3), g.search_wildcard_batch(many)
    assert g.last_wildcard_stats()[0] >= 3                                  # 128 patterns, 2048 elements per scan
    for p, t, d in zip(many, got_t, got_d):
        assert t == want_terms(p, 3) and d == want_docs(p), p[:40]


def _raw_docs(g, patterns, cap, payload=True):
    blob, p_offs = _key_arrays(patterns)
    n = len(patterns)
    h_offs = np.full(n + 1, 77, np.uint64)
    matched = np.full(max(n, 1), 77, np.uint64)
    total = C.c_uint64(77)
    docs = np.zeros(max(cap, 1), np.uint32)
    rc = L.load().tfidf_search_wildcard_batch(g._h, blob, L.ptr(p_offs, C.c_uint64), n,
                                              L.ptr(docs, C.c_uint32) if payload else None, cap,
                                              L.ptr(h_offs, C.c_uint64), L.ptr(matched, C.c_uint64), C.byref(total), None)
    return rc, h_offs.tolist(), matched[:n].tolist(), total.value


def _raw_terms(g, patterns, max_out, cand_cap, terms_cap, payload=True):
    blob, p_offs = _key_arrays(patterns)
    n = len(patterns)
    c_offs = np.full(n + 1, 77, np.uint64)
    matched = np.full(max(n, 1), 77, np.uint64)
    nc, nb = C.c_uint64(77), C.c_uint64(77)
    t_out = np.zeros(cand_cap + 1, np.uint64)
    text = np.zeros(max(terms_cap, 1), np.uint8)
    df = np.zeros(max(cand_cap, 1), np.uint32)
    rc = L.load().tfidf_wildcard_terms_batch(
        g._h, blob, L.ptr(p_offs, C.c_uint64), n, max_out, L.ptr(c_offs, C.c_uint64), L.ptr(matched, C.c_uint64),
        L.ptr(t_out, C.c_uint64) if payload else None, text.ctypes.data_as(C.c_void_p) if payload else None, terms_cap,
        L.ptr(df, C.c_uint32) if payload else None, cand_cap, C.byref(nc), C.byref(nb), None)
    return rc, c_offs.tolist(), matched[:n].tolist(), nc.value, nb.value


def test_buffer_protocol_and_argument_errors():
    g = index()
    pats = [b"a?c*", b"caf?", b"", W.LONG255[:40] + b"*", b"nothing*"]
    full_d = [want_docs(p) for p in pats]
    offs = [0]
    for d, _ in full_d:
        offs.append(offs[-1] + len(d))
    matched = [m for _, m in full_d]
    H = offs[-1]
    assert H > 10
    assert _raw_docs(g, pats, 0, payload=False) == (L.E_BUFFER, offs, matched, H)      # the size query
    assert _raw_docs(g, pats, H - 1) == (L.E_BUFFER, offs, matched, H)                 # one slot short: counts in full
    assert _raw_docs(g, pats, H) == (L.OK, offs, matched, H)
    assert _raw_docs(g, [b"nothing*", b""], 0, payload=False) == (L.OK, [0, 0, 0], [0, 0], 0)
    assert _raw_docs(g, [], 0, payload=False)[0] == L.OK
    full_t = [want_terms(p, 5) for p in pats]
    n_c = sum(len(c) for c, _ in full_t)
    n_b = sum(len(t) for c, _ in full_t for t, _ in c)
    c_offs = [0]
    for c, _ in full_t:
        c_offs.append(c_offs[-1] + len(c))
    assert n_c > 5 and n_b > 255
    assert _raw_terms(g, pats, 5, 0, 0, payload=False) == (L.E_BUFFER, c_offs, matched, n_c, n_b)
    assert _raw_terms(g, pats, 5, n_c - 1, n_b) == (L.E_BUFFER, c_offs, matched, n_c, n_b)
    assert _raw_terms(g, pats, 5, n_c, n_b - 1) == (L.E_BUFFER, c_offs, matched, n_c, n_b)
    assert _raw_terms(g, pats, 5, n_c, n_b) == (L.OK, c_offs, matched, n_c, n_b)
    # argument errors: nothing written
    for k in (0, 1025):
        rc, o, w, a, b = _raw_terms(g, pats, k, n_c, n_b)
        assert rc == L.E_INVALID_ARG and o == [77] * (len(pats) + 1) and w == [77] * len(pats) and (a, b) == (77, 77)
    many = [b"a"] * 65537
    assert _raw_terms(g, many, 1, 0, 0, payload=False)[0] == L.E_INVALID_ARG
    assert _raw_docs(g, many, 0, payload=False) == (L.E_INVALID_ARG, [77] * 65538, [77] * 65537, 77)
    # before the first commit
    fresh = ShardIndex(vocab_capacity_log2=12)
    fresh.add_documents([b"abc"])
    for call in (lambda: fresh.wildcard_terms_batch([b"a*"]), lambda: fresh.wildcard_terms(b"a*"),
                 lambda: fresh.search_wildcard_batch([b"a*"]), lambda: fresh.search_wildcard(b"a*")):
        with pytest.raises(L.TfidfError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    fresh.close()


def test_delete_commit_and_an_older_reader():
    texts = W.dense_texts()
    keys = [b"d%05d" % i for i in range(len(texts))]
    g = ShardIndex(vocab_capacity_log2=16)
    g.add_documents(texts, keys)
    g.commit()
    probes = [b"caf*", b"a", b"a*", b"*", HASHED + b"*", b"?"]
    before = {p: (want_terms(p, 1024), want_docs(p)) for p in probes}
    old = g.reader()
    assert {p: (old.wildcard_terms(p, 1024), old.search_wildcard(p)) for p in probes} == before
    # the only documents holding "cafe", and the first document of the corpus (the only "a": every later id moves)
    gone = [i for i, t in enumerate(texts) if t in (W.CAFES[1], b"X CAFE .")] + [0]
    assert len(gone) == 3 and g.delete_documents([keys[i] for i in gone]) == 3
    g.commit()
    left = [t for i, t in enumerate(texts) if i not in gone]
    ix = W.oracle_index(left)
    vocab, sets = ix.vocab(), W.doc_term_sets(ix, len(left))
    ix.close()
    assert W.CAFES[1] not in vocab and b"a" not in vocab
    after = {p: (W.expected_terms(vocab, p, 1024), W.expected_docs(sets, vocab, p)) for p in probes}
    assert {p: (g.wildcard_terms(p, 1024), g.search_wildcard(p)) for p in probes} == after
    assert after[b"a"] == (([], 0), ([], 0)) and after[b"*"][1][0] == list(range(len(left)))
    assert W.CAFES[1] not in [t for t, _ in after[b"caf*"][0][0]] and after[b"caf*"][0][1] == before[b"caf*"][0][1] - 1
    assert {p: (old.wildcard_terms(p, 1024), old.search_wildcard(p)) for p in probes} == before   # the old snapshot
    old.close()
    g.close()


def test_calls_beside_add_docs_and_commit():
    texts = W.dense_texts()
    added = [b"abcabq", b"abcabr abcabq", b"abcqbq"]
    probes = [b"abcab?", b"abc*q", b"*"]
    states = []
    for i in range(len(added) + 1):
        ix = W.oracle_index(texts + added[:i])
        vocab, sets = ix.vocab(), W.doc_term_sets(ix, len(texts) + i)
        ix.close()
        states.append([(W.expected_terms(vocab, p, 5), W.expected_docs(sets, vocab, p)) for p in probes])
    assert len({repr(s) for s in states}) == len(states)                    # every commit changes an answer
    g = ShardIndex(vocab_capacity_log2=16)
    g.add_documents(texts)
    g.commit()
    rd = g.reader()
    errs, stop = [], threading.Event()

    def both(h):
        return list(zip(h.wildcard_terms_batch(probes, 5), h.search_wildcard_batch(probes)))

    def look():
        try:
            while not stop.is_set():
                assert both(rd) == states[0]                                # the reader: its own snapshot
                assert g.search_wildcard_batch(probes) in [[d for _, d in s] for s in states]   # one whole snapshot
                assert g.wildcard_terms(probes[0], 5) in [s[0][0] for s in states]
        except BaseException as e:                                          # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=look) for _ in range(4)]
    for t in th:
        t.start()
    for d in added:
        g.add_documents([d])
        g.commit()
    stop.set()
    for t in th:
        t.join()
    assert errs == []
    assert both(g) == states[-1] and both(rd) == states[0]
    rd.close()
    g.close()


def test_df_stays_local_under_global_statistics():
    g = ShardIndex(vocab_capacity_log2=16, stats_mode=L.STATS_GLOBAL)
    g.add_documents(W.dense_texts())
    g.commit()
    keys, dl, _ = g.vocab_export()
    st = g.stats()
    g.set_global_stats(keys, dl.astype(np.uint64) * 3, st["doc_count"] * 3, st["sum_ttf"] * 3)
    for p in (b"a*", b"caf?"):
        assert g.wildcard_terms(p, 1024) == want_terms(p, 1024) and g.search_wildcard(p) == want_docs(p)
    g.close()


def test_worker_prefix_search_and_suggestions(lucene_fixture):
    w = Worker()
    texts = [d["text"].encode() for d in lucene_fixture["docs"]]
    names = [d["name"] for d in lucene_fixture["docs"]]
    w.index.add_documents(texts, [n.encode() for n in names])
    w.commit()
    ix = W.oracle_index(texts)
    vocab, sets = ix.vocab(), W.doc_term_sets(ix, len(texts))
    ix.close()
    stem = sorted(vocab, key=lambda t: (-vocab[t], t))[0][:2]
    docs, n = W.expected_docs(sets, vocab, stem + b"*")
    hits = w.search_prefix(stem.decode().upper())
    assert [h["document"]["name"] for h in hits] == [names[d] for d in docs] and len(docs) >= 1
    assert all(h["score"] == 1.0 for h in hits)
    sug = w.suggest_terms(stem.decode(), 3)
    assert sug == [(t.decode(), df) for t, df in W.expected_terms(vocab, stem + b"*", 3)[0]] and 1 <= len(sug) <= 3
    assert w.search_prefix("a*") == [] == w.suggest_terms("?")              # the text's own wildcards are literals
    assert w.search_prefix("zzzzqqqq") == []
    w.close()
