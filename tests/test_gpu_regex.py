"""Regular-expression search on the device (tfidf_regex_terms[_batch],
tfidf_search_regex[_batch], the reader forms, Worker.search_regex) against
regex_ref.py, compared exactly: the same term lists, df, n_matched and doc ids
as brute force over the oracle's vocabulary and documents, and the same arrays
as the wildcard calls for every wildcard pattern written as a regular
expression.  The corpora and the committed indexes are those of
test_gpu_wildcard.py (never changed)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import regex_ref as R
import test_gpu_wildcard as TW
import wildcard_ref as W
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex, _key_arrays
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

INVERSIONS = TW.INVERSIONS
HASHED = TW.HASHED
HARD7 = b"(a|b)*a(a|b){7}"                          # 2^8 live states
HARD10 = b"(a|b)*a(a|b){10}"                        # 2^11 live states, a 12 KiB table
HARD_OR = HARD10 + b"|[a-c]{1,3}"                   # as large, and short terms belong to it
PATTERNS = [b".*", b"a.*", b".*c", b"a.c.*", b"..", b"abcab", HASHED[:12] + b".*", HASHED + b".*", W.LONG255[:40] + b".*",
            W.LONG255[:254] + b".", b"caf.", b"", b"\xff.*", b".{256}", b".*nop", b"ZQ.*", "àé.*".encode(), ".*ñ".encode(),
            b".", b"a.*b.*c", b"nothing.*", b".*lmnop.*", b"@", b"#", b"[ab]{2,3}", b"(ab|ba)+c?", b"[^a-c]+",
            "caf[é-ë]s?".encode(), "[^\x00-\x7f]+".encode(), b"~(a.*)&[a-c]{1,2}", HARD7, b"[a-c]*[^c]", b".{17}",
            b"\\w{17,}", b"(lmnop){51}", b"[a-c]{6}&.*cc.*&~(.*aa.*)", b'"caf"(e|' + "é".encode() + b")", b"()", b"x", b"(a|b)*a(a|b){3}"]
assert len(PATTERNS) < 128


def index(inversion=L.INVERSION_BLOCK):
    return TW.index(inversion)


@functools.lru_cache(maxsize=None)
def want_terms_all(p):
    return R.expected_terms(W.dense_vocab(), p, 1 << 30)


def want_terms(p, k):
    lst, n = want_terms_all(p)
    return lst[:k], n


@functools.lru_cache(maxsize=None)
def want_docs(p):
    return R.expected_docs(TW.dense_sets(), W.dense_vocab(), p)


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_term_lists_equal_the_reference(inversion):
    g = index(inversion)
    for k in (1, 5, 1024):
        got = g.regex_terms_batch(PATTERNS, k)
        assert len(got) == len(PATTERNS)
        for p, gt in zip(PATTERNS, got):
            assert gt == want_terms(p, k), (p[:40], k)
    # the fixture reaches its cases
    assert want_terms(b".*", 5)[1] == want_terms(b"@", 5)[1] == len(W.dense_vocab()) > 1024
    assert [t for t, _ in want_terms(b"caf.", 5)[0]] == [b"cafe", "café".encode()]
    assert want_terms(HASHED + b".*", 5)[1] == 2 and want_terms(HASHED[:12] + b".*", 5)[1] == 3
    assert want_terms(W.LONG255[:40] + b".*", 5) == ([(W.LONG255, 2)], 1) == want_terms(b"(lmnop){51}", 5)
    assert want_terms(b"", 5) == want_terms(b"\xff.*", 5) == want_terms(b".{256}", 5) == want_terms(b"#", 5) == ([], 0)
    assert want_terms(b"ZQ.*", 5) == want_terms(b"()", 5) == ([], 0) and want_terms(b"zq.*", 5)[1] > 0
    assert {W.HAN, W.EMOJI} <= {t for t, _ in want_terms(b".", 1024)[0]}
    assert want_terms(HARD7, 5) == ([], 0)                                  # walked to the end of many terms, accepted by none
    assert 0 < want_terms(b"(a|b)*a(a|b){3}", 5)[1] < want_terms(b"[a-c]*[^c]", 5)[1]
    assert want_terms(b"\\w{17,}", 5)[1] >= 2 and want_terms("[^\x00-\x7f]+".encode(), 5)[1] >= 2


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_document_sets_equal_the_reference(inversion):
    g = index(inversion)
    got = g.search_regex_batch(PATTERNS)
    assert len(got) == len(PATTERNS)
    for p, gd in zip(PATTERNS, got):
        assert gd == want_docs(p), p[:40]
    n = len(W.dense_texts())
    assert want_docs(b".*") == (list(range(n)), len(W.dense_vocab()))      # every document has a token
    assert 0 < len(want_docs(b"a.c.*")[0]) < n and want_docs(b"nothing.*") == ([], 0)


def twin(p):
    """the regular expression of a wildcard pattern (one that is not UTF-8 stays: it matches nothing either way)"""
    rx = R.from_wildcard(p)
    return p if rx is None else rx


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_wildcard_twins_give_the_wildcard_calls_arrays(inversion):
    assert twin(b"a?c*") == b"a.c.*" and twin(b"\\*") == b"\\*" and twin(b"ZQ*") == b"zq.*" and twin(b"\xff*") == b"\xff*"
    for g, pats in ((index(inversion), TW.PATTERNS), (TW.block_index(inversion), W.BLOCK_PATTERNS)):
        rx = [twin(p) for p in pats]
        wd, rd = g.search_wildcard_batch_arrays(pats), g.search_regex_batch_arrays(rx)
        for a, b in zip(wd[:3], rd[:3]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        for k in (1, 5, 1024):
            assert g.regex_terms_batch(rx, k) == g.wildcard_terms_batch(pats, k)
    g = TW.block_index(inversion)                                          # the block and word edges of the union
    assert g.search_regex(b"edgeterm")[0] == W.EDGE_DOCS == g.search_regex(b"edge[a-z]+")[0]
    assert g.search_regex(b"edge\\d")[0] == W.EDGE_DOCS and g.search_regex(b"edge\\d")[1] == len(W.EDGE_DOCS)
    assert g.search_regex(b"solo|edge8") == ([8191, W.N_BLOCKS_DOCS - 1], 2)
    assert len(g.search_regex(b"[wv]\\d")[0]) == W.N_BLOCKS_DOCS


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_a_literal_pattern_is_the_term(inversion):
    g = index(inversion)
    for t in (b"abcab", b"a", W.CAFES[0], HASHED, W.LONG255, b"zzzz"):
        docs, n = g.search_regex(t)
        assert docs == sorted(d for d, _ in g.search(t, k=0))
        terms, m = g.regex_terms(t, 5)
        assert (terms, m) == ([(x, df) for x, df, _ in g.fuzzy_terms(t, 0)[0]], n)
        assert n == (1 if t != b"zzzz" else 0)


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_single_and_reader_forms_equal_the_batch_of_one(inversion):
    g = index(inversion)
    some = [b"a.*", b".*", b"caf.", HASHED + b".*", b"", b"\xff.*", b"nothing.*", W.EMOJI, b"[ab]{2,3}", b"#"]
    with g.reader() as rd:
        for p in some:
            wt, wd = want_terms(p, 5), want_docs(p)
            assert g.regex_terms(p, 5) == wt == rd.regex_terms(p, 5)
            assert g.regex_terms_batch([p], 5) == [wt] == rd.regex_terms_batch([p], 5)
            assert g.search_regex(p) == wd == rd.search_regex(p)
            assert g.search_regex_batch([p]) == [wd] == rd.search_regex_batch([p])
    assert g.regex_terms_batch([]) == [] == g.search_regex_batch([])        # n_p = 0 is legal
    assert g.last_regex_stats() == (0, 0, 0, 0)


@pytest.mark.parametrize("inversion", INVERSIONS)
@pytest.mark.parametrize("knob,budget", [("TFIDF_REGEX_MATCH_BUDGET", "1"), ("TFIDF_REGEX_MATCH_BUDGET", "100"),
                                         ("TFIDF_REGEX_HIT_BUDGET", "1"), ("TFIDF_REGEX_HIT_BUDGET", "20000"),
                                         ("TFIDF_REGEX_TABLE_BUDGET", "1"), ("TFIDF_REGEX_TABLE_BUDGET", "3000")])
def test_any_budget_gives_the_same_output(inversion, knob, budget, monkeypatch):
    g = index(inversion)
    staged = sum(1 for p in PATTERNS if p not in (b"", b"\xff.*", b"#", b"()"))   # the others have a table to walk
    whole_d = g.search_regex_batch_arrays(PATTERNS)
    scans, matches, unions, tab_bytes = g.last_regex_stats()
    assert scans == 1 and unions == 1 and matches == sum(want_terms(p, 1)[1] for p in PATTERNS)
    assert 160 * staged < tab_bytes <= 32768                                # a header and the ASCII map each at least
    whole_t = g.regex_terms_batch(PATTERNS, 5)
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    monkeypatch.setenv(knob, budget)
    split_d = g.search_regex_batch_arrays(PATTERNS)
    for a, b in zip(split_d[:3], whole_d[:3]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    s2, m2, u2, t2 = g.last_regex_stats()
    assert (m2, t2) == (matches, tab_bytes)
    if knob == "TFIDF_REGEX_TABLE_BUDGET":
        assert s2 > scans and u2 >= unions
        if budget == "1":
            assert s2 == staged                                             # one table in each scan
    else:
        assert s2 == scans and u2 > unions
        if budget == "1":                                                   # every pattern with a term alone
            assert u2 == sum(1 for p in PATTERNS if want_terms(p, 1)[1])
    assert g.regex_terms_batch(PATTERNS, 5) == whole_t


def test_more_patterns_than_one_scan_stages():
    g = index()
    many = [s[:2] + b"[a-c]*" + s[-1:] for s in W.ABC[600:880]]
    many[50:50] = [HARD10, b"nothing[0-9]+", HARD7]
    many[200:200] = [HARD_OR, b"#", b"(a|b)*b(a|b){10}", b"zzz.*"]
    many += [b"(a|b|c)*c(a|b|c){6}", W.LONG255[:200] + b".*", b"\xff", HARD7 + b"|" + HASHED]
    many += [b"[a-c]{%d}" % (i % 7) for i in range(300 - len(many))]
    assert len(many) == 300
    got_t, got_d = g.regex_terms_batch(many, 3), g.search_regex_batch(many)
    scans, _, _, tab_bytes = g.last_regex_stats()
    assert scans >= 4 and tab_bytes > 3 * 12288 + 32768                     # 128 patterns, 32 KiB of tables per scan
    for p, t, d in zip(many, got_t, got_d):
        assert t == want_terms(p, 3) and d == want_docs(p), p[:40]
    assert want_terms(HARD_OR, 3)[1] == 3 + 9 + 27 and want_terms(b"zzz.*", 3) == ([], 0) == want_terms(HARD10, 3)


def _raw_docs(g, patterns, cap, payload=True):
    blob, p_offs = _key_arrays(patterns)
    n = len(patterns)
    h_offs = np.full(n + 1, 77, np.uint64)
    matched = np.full(max(n, 1), 77, np.uint64)
    total = C.c_uint64(77)
    docs = np.zeros(max(cap, 1), np.uint32)
    ms = C.c_float(77.0)
    rc = L.load().tfidf_search_regex_batch(g._h, blob, L.ptr(p_offs, C.c_uint64), n,
                                           L.ptr(docs, C.c_uint32) if payload else None, cap,
                                           L.ptr(h_offs, C.c_uint64), L.ptr(matched, C.c_uint64), C.byref(total),
                                           C.byref(ms))
    return rc, h_offs.tolist(), matched[:n].tolist(), total.value, ms.value == 77.0


def _raw_terms(g, patterns, max_out, cand_cap, terms_cap, payload=True):
    blob, p_offs = _key_arrays(patterns)
    n = len(patterns)
    c_offs = np.full(n + 1, 77, np.uint64)
    matched = np.full(max(n, 1), 77, np.uint64)
    nc, nb = C.c_uint64(77), C.c_uint64(77)
    t_out = np.zeros(cand_cap + 1, np.uint64)
    text = np.zeros(max(terms_cap, 1), np.uint8)
    df = np.zeros(max(cand_cap, 1), np.uint32)
    ms = C.c_float(77.0)
    rc = L.load().tfidf_regex_terms_batch(
        g._h, blob, L.ptr(p_offs, C.c_uint64), n, max_out, L.ptr(c_offs, C.c_uint64), L.ptr(matched, C.c_uint64),
        L.ptr(t_out, C.c_uint64) if payload else None, text.ctypes.data_as(C.c_void_p) if payload else None, terms_cap,
        L.ptr(df, C.c_uint32) if payload else None, cand_cap, C.byref(nc), C.byref(nb), C.byref(ms))
    return rc, c_offs.tolist(), matched[:n].tolist(), nc.value, nb.value, ms.value == 77.0


def test_buffer_protocol_and_argument_errors():
    g = index()
    pats = [b"a.c.*", b"caf.", b"", W.LONG255[:40] + b".*", b"nothing.*"]
    full_d = [want_docs(p) for p in pats]
    offs = [0]
    for d, _ in full_d:
        offs.append(offs[-1] + len(d))
    matched = [m for _, m in full_d]
    H = offs[-1]
    assert H > 10
    assert _raw_docs(g, pats, 0, payload=False)[:4] == (L.E_BUFFER, offs, matched, H)  # the size query
    assert _raw_docs(g, pats, H - 1)[:4] == (L.E_BUFFER, offs, matched, H)             # one slot short: counts in full
    assert _raw_docs(g, pats, H)[:4] == (L.OK, offs, matched, H)
    assert _raw_docs(g, [b"nothing.*", b""], 0, payload=False)[:4] == (L.OK, [0, 0, 0], [0, 0], 0)
    assert _raw_docs(g, [], 0, payload=False)[0] == L.OK
    full_t = [want_terms(p, 5) for p in pats]
    n_c = sum(len(c) for c, _ in full_t)
    n_b = sum(len(t) for c, _ in full_t for t, _ in c)
    c_offs = [0]
    for c, _ in full_t:
        c_offs.append(c_offs[-1] + len(c))
    assert n_c > 5 and n_b > 255
    assert _raw_terms(g, pats, 5, 0, 0, payload=False)[:5] == (L.E_BUFFER, c_offs, matched, n_c, n_b)
    assert _raw_terms(g, pats, 5, n_c - 1, n_b)[:5] == (L.E_BUFFER, c_offs, matched, n_c, n_b)
    assert _raw_terms(g, pats, 5, n_c, n_b - 1)[:5] == (L.E_BUFFER, c_offs, matched, n_c, n_b)
    assert _raw_terms(g, pats, 5, n_c, n_b)[:5] == (L.OK, c_offs, matched, n_c, n_b)
    # argument errors: nothing written
    for k in (0, 1025):
        rc, o, w, a, b, ms = _raw_terms(g, pats, k, n_c, n_b)
        assert rc == L.E_INVALID_ARG and o == [77] * (len(pats) + 1) and w == [77] * len(pats) and (a, b, ms) == (77, 77, True)
    many = [b"a"] * 65537
    assert _raw_terms(g, many, 1, 0, 0, payload=False)[0] == L.E_INVALID_ARG
    assert _raw_docs(g, many, 0, payload=False) == (L.E_INVALID_ARG, [77] * 65538, [77] * 65537, 77, True)
    # a pattern in error at the front, in the middle or at the end: its status, and nothing written
    good = [b"a.*", b"caf.", b".*c"]
    for bad, code in ((b"a|", L.E_QUERY_SYNTAX), (b"(ab", L.E_QUERY_SYNTAX), (b"[b-a]", L.E_QUERY_SYNTAX),
                      (b"a<1-5>", L.E_UNSUPPORTED_QUERY), (b"(a|b)*a(a|b){16}", L.E_UNSUPPORTED_QUERY),
                      (b"(a{1000}){1000}", L.E_UNSUPPORTED_QUERY)):
        for at in (0, 1, 3):
            ps = good[:at] + [bad] + good[at:]
            assert _raw_docs(g, ps, 1 << 16) == (code, [77] * 5, [77] * 4, 77, True), (bad, at)
            assert _raw_terms(g, ps, 5, 64, 4096) == (code, [77] * 5, [77] * 4, 77, 77, True), (bad, at)
            msg = L.load().tfidf_last_error().decode()
            assert "pattern %d" % at in msg and "byte" in msg, msg
        for call in (lambda: g.regex_terms(bad), lambda: g.search_regex(bad), lambda: g.regex_terms_batch([bad]),
                     lambda: g.search_regex_batch(good + [bad])):
            with pytest.raises(L.TfidfError) as ei:
                call()
            assert ei.value.code == code
    with g.reader() as rd:
        with pytest.raises(L.TfidfError) as ei:
            rd.search_regex_batch([b"a", b"*"])
        assert ei.value.code == L.E_QUERY_SYNTAX
    # before the first commit
    fresh = ShardIndex(vocab_capacity_log2=12)
    fresh.add_documents([b"abc"])
    for call in (lambda: fresh.regex_terms_batch([b"a.*"]), lambda: fresh.regex_terms(b"a.*"),
                 lambda: fresh.search_regex_batch([b"a.*"]), lambda: fresh.search_regex(b"a.*")):
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
    probes = [b"caf.*", b"a", b"a.*", b".*", HASHED + b".*", b".", b"[a-c]{1,2}"]
    before = {p: (want_terms(p, 1024), want_docs(p)) for p in probes}
    old = g.reader()
    assert {p: (old.regex_terms(p, 1024), old.search_regex(p)) for p in probes} == before
    # the only documents holding "cafe", and the first document of the corpus (the only "a": every later id moves)
    gone = [i for i, t in enumerate(texts) if t in (W.CAFES[1], b"X CAFE .")] + [0]
    assert len(gone) == 3 and g.delete_documents([keys[i] for i in gone]) == 3
    g.commit()
    left = [t for i, t in enumerate(texts) if i not in gone]
    ix = W.oracle_index(left)
    vocab, sets = ix.vocab(), W.doc_term_sets(ix, len(left))
    ix.close()
    assert W.CAFES[1] not in vocab and b"a" not in vocab
    after = {p: (R.expected_terms(vocab, p, 1024), R.expected_docs(sets, vocab, p)) for p in probes}
    assert {p: (g.regex_terms(p, 1024), g.search_regex(p)) for p in probes} == after
    assert after[b"a"] == (([], 0), ([], 0)) and after[b".*"][1][0] == list(range(len(left)))
    assert W.CAFES[1] not in [t for t, _ in after[b"caf.*"][0][0]] and after[b"caf.*"][0][1] == before[b"caf.*"][0][1] - 1
    assert {p: (old.regex_terms(p, 1024), old.search_regex(p)) for p in probes} == before   # the old snapshot
    old.close()
    g.close()


def test_calls_beside_add_docs_and_commit():
    texts = W.dense_texts()
    added = [b"abcabq", b"abcabr abcabq", b"abcqbq"]
    probes = [b"abcab.", b"abc.*q", b".*", b"abc[a-z]b[qr]"]
    states = []
    for i in range(len(added) + 1):
        ix = W.oracle_index(texts + added[:i])
        vocab, sets = ix.vocab(), W.doc_term_sets(ix, len(texts) + i)
        ix.close()
        states.append([(R.expected_terms(vocab, p, 5), R.expected_docs(sets, vocab, p)) for p in probes])
    assert len({repr(s) for s in states}) == len(states)                    # every commit changes an answer
    g = ShardIndex(vocab_capacity_log2=16)
    g.add_documents(texts)
    g.commit()
    rd = g.reader()
    errs, stop = [], threading.Event()

    def both(h):
        return list(zip(h.regex_terms_batch(probes, 5), h.search_regex_batch(probes)))

    def look():
        try:
            while not stop.is_set():
                assert both(rd) == states[0]                                # the reader: its own snapshot
                assert g.search_regex_batch(probes) in [[d for _, d in s] for s in states]   # one whole snapshot
                assert g.regex_terms(probes[0], 5) in [s[0][0] for s in states]
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


def test_worker_search_regex(lucene_fixture):
    w = Worker()
    texts = [d["text"].encode() for d in lucene_fixture["docs"]]
    names = [d["name"] for d in lucene_fixture["docs"]]
    w.index.add_documents(texts, [n.encode() for n in names])
    w.commit()
    ix = W.oracle_index(texts)
    vocab, sets = ix.vocab(), W.doc_term_sets(ix, len(texts))
    ix.close()
    stem = sorted(vocab, key=lambda t: (-vocab[t], t))[0][:2].decode()
    for rx in (stem + ".*", "[a-m].*(s|ing)", ".{1,3}", "zzzzqqqq", stem.upper() + ".*"):
        docs, _ = R.expected_docs(sets, vocab, rx.encode())
        hits = w.search_regex(rx)
        assert [h["document"]["name"] for h in hits] == [names[d] for d in docs], rx
        assert all(h["score"] == 1.0 for h in hits)
    assert w.search_regex(stem + ".*") == w.search_prefix(stem) != [] and w.search_regex(stem.upper() + ".*") == []
    with pytest.raises(L.TfidfError) as ei:
        w.search_regex(stem + "(")
    assert ei.value.code == L.E_QUERY_SYNTAX
    w.close()
