"""Hit highlighting on the device (tfidf_matches / tfidf_snippets and their
reader forms) against the restatement built from the oracle alone
(highlight_ref.py), compared exactly: edge lengths around every slice, chunk
and wave boundary, documents without a split byte, Unicode folding, hashed
keys (with and without forced collisions), operator queries, a malformed
document, snippet ranges / packed bytes / in-snippet matches at several
widths, row chunks (the budget knobs, and one call over the default item
budget), the buffer protocol and the order of its errors, snapshot pinning
beside commits, and Worker.search_snippets."""
import ctypes as C
import threading

import numpy as np
import pytest

import highlight_ref as H
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex, query_positive_terms
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

_index = {}


def index_of(name):
    """One committed index per corpus, shared by the tests (never changed)."""
    name = {"nosplit220": "nosplit255"}.get(name, name)             # the same documents, another query
    if name not in _index:
        texts, _, _ = H.corpus(name)
        g = ShardIndex()
        g.add_documents(list(texts), [b"%s/%04d" % (name.encode(), i) for i in range(len(texts))])
        g.commit()
        _index[name] = g
    return _index[name]


def check_matches(name, docs=None, reader=False):
    texts, q, terms = H.corpus(name)
    g = index_of(name)
    docs = list(range(len(texts))) if docs is None else docs
    assert query_positive_terms(q) == terms
    if reader:
        with g.reader() as rd:
            got = rd.matches(q, docs)
    else:
        got = g.matches(q, docs)
    want = H.expected_matches(name)
    assert len(got) == len(docs)
    for d, m in zip(docs, got):
        assert m == want[d], (name, d, len(texts[d]))
    return got


def check_snippets(name, W, docs=None):
    texts, q, _ = H.corpus(name)
    g = index_of(name)
    docs = list(range(len(texts))) if docs is None else docs
    got = g.snippets(q, docs, W)
    want = H.expected_snippets(name, W)
    assert len(got) == len(docs)
    for d, (a, text, ms) in zip(docs, got):
        wa, wb, wm = want[d]
        assert (a, a + len(text)) == (wa, wb), (name, W, d)
        assert text == texts[d][wa:wb], (name, W, d)                # the packed bytes
        assert ms == wm, (name, W, d)
        assert len(text) <= W
        if H.doc_tokens(texts[d]) is not None:
            text.decode("utf-8")
    return got


# 1. edge lengths
def test_edge_lengths_all_documents_in_one_call():
    got = check_matches("edge")
    assert sum(len(m) for m in got) > 20000
    check_matches("edge", reader=True)


def test_edge_lengths_one_document_per_call():
    n = len(H.LENGTHS)
    for d in (0, 1, n - 4, n - 3, n - 2, n - 1):                    # 0, 1, 16384, 16385, 20000, 70000 bytes
        check_matches("edge", [d])


def reversed_with_repeats():
    docs = list(range(H.N_EDGE))[::-1]
    docs[5], docs[200] = docs[6], docs[3]
    return docs


def test_edge_lengths_reversed_with_repeats():
    docs = reversed_with_repeats()
    check_matches("edge", docs)
    check_snippets("edge", 160, docs[:40])


@pytest.mark.parametrize("knobs", [{"TFIDF_HL_CHUNK_ITEMS": "1"}, {"TFIDF_HL_CHUNK_ITEMS": "3"},
                                   {"TFIDF_HL_CHUNK_MATCHES": "1"}, {"TFIDF_HL_CHUNK_MATCHES": "7"},
                                   {"TFIDF_HL_CHUNK_ITEMS": "3", "TFIDF_HL_CHUNK_MATCHES": "7"}],
                         ids=["items1", "items3", "matches1", "matches7", "items3-matches7"])
def test_single_forms_under_any_chunking(knobs, monkeypatch):
    """A single-query call is a batch of one query, so the budget knobs cut its
    rows too (read at call time: the shared index serves).  Items 1: every row
    with work is a chunk; items 3: a 70 000-byte document (5 items) is a chunk
    of its own beside chunks of several rows; matches 1 / 7: rows above the
    budget alone, rows of 0 matches ride along."""
    index_of("edge")
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    check_matches("edge")
    check_matches("edge", reader=True)
    check_snippets("edge", 160, reversed_with_repeats())


def test_single_call_over_the_default_item_budget():
    """2^16 + 1 rows of one short document: one item each, one more than a row
    chunk's default item budget, so the call runs in two chunks (no knob set)."""
    n = (1 << 16) + 1
    d = H.LENGTHS.index(257)
    texts, q, _ = H.corpus("edge")
    m = H.expected_matches("edge")[d]
    a, b, sm = H.expected_snippets("edge", 160)[d]
    assert len(texts[d]) == 257 and len(m) > len(sm) > 0
    docs = np.full(n, d, np.uint32)

    def tiled(ms, col, dtype):
        return np.tile(np.array([x[col] for x in ms], dtype), n)

    def rows(k):
        return np.arange(n + 1, dtype=np.uint64) * np.uint64(k)
    with index_of("edge").reader() as rd:
        st, ln, od, offs, _ = rd.matches_arrays(q, docs)
        text, t_offs, d_starts, sst, sln, sod, m_offs, _ = rd.snippets_arrays(q, docs, 160)
    assert len(st) == n * len(m) and len(sst) == n * len(sm)
    assert (offs == rows(len(m))).all()
    assert (st == tiled(m, 0, np.uint64)).all() and (ln == tiled(m, 1, np.uint32)).all()
    assert (od == tiled(m, 2, np.uint32)).all()
    assert text == texts[d][a:b] * n and (t_offs == rows(b - a)).all() and (d_starts == a).all()
    assert (m_offs == rows(len(sm))).all()
    assert (sst == tiled(sm, 0, np.uint64)).all() and (sln == tiled(sm, 1, np.uint32)).all()
    assert (sod == tiled(sm, 2, np.uint32)).all()


# 2. no split byte
@pytest.mark.parametrize("name", ["nosplit255", "nosplit220", "han"])
def test_documents_without_a_split_byte(name):
    got = check_matches(name)
    if name == "nosplit255":
        assert got[0] == [(0, 255, 0), (255, 255, 0)] and len(got[1]) == 156
    if name == "nosplit220":
        assert got[0] == [] and got[1] == [(39780, 220, 0)]
    if name == "han":
        assert len(got[0]) == 2 * 1366


# 3. Unicode folding
def test_unicode_folding():
    got = check_matches("unicode")
    assert [m[1] for m in got[1]] == [9, 8, 8, 9]                   # İstanbul: raw 9 bytes, term 8
    assert all(got)


def test_tokens_of_every_kind_across_the_lookahead_window():
    got = check_matches("window")
    assert {o for m in got for _, _, o in m} == set(range(15))
    for W in (16, 160, 1024):
        check_snippets("window", W)


def test_tokens_over_255_units_across_the_lookahead_window():
    """`window` with runs of 300 a and 1 100 Z between its pieces: the scan
    cuts them at 255 units (a x 255 + a x 45; z x 255 four times + z x 80), and
    the corpus commits under the first hash seed (test_gpu_token_cut.py: two
    over-long runs in one unit's window once failed k_tokenize_uchunk)."""
    got = check_matches("windowcut")
    s = index_of("windowcut").stats()
    assert (s["hash_rebuilds"], s["hash_seed"]) == (0, 0)
    assert {o for m in got for _, _, o in m} == set(range(18))
    assert {l for m in got for _, l, o in m if o >= 15} == {255, 80, 45}
    for W in (16, 160, 1024):
        check_snippets("windowcut", W)


# 4. hashed keys
@pytest.mark.parametrize("weak", [False, True])
def test_hashed_keys_never_match_the_unqueried_twin(weak, monkeypatch):
    texts, q, terms = H.corpus("twins")
    if weak:
        monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    g = ShardIndex()
    g.add_documents(list(texts))
    g.commit()
    assert g.stats()["hash_rebuilds"] == (1 if weak else 0)
    got = g.matches(q, [0, 1, 2])
    assert got == H.expected_matches("twins")
    assert got[1] == [] and [o for _, _, o in got[0]] == [0, 1]
    for W in (16, 64):
        for d, ((a, text, ms), (wa, wb, wm)) in enumerate(zip(g.snippets(q, [0, 1, 2], W),
                                                              H.expected_snippets("twins", W))):
            assert (a, text, ms) == (wa, texts[d][wa:wb], wm)
    g.close()


# 5. operators
@pytest.mark.parametrize("name", ["ops", "dup", "dotted", "seventy"])
def test_operator_queries(name):
    got = check_matches(name)
    if name == "ops":
        assert got[2] == [] and got[3] == [(0, 4, 1)]               # gamma is never a match; non-hits are legal
    if name == "dup":
        assert {o for _, _, o in got[0]} == {0}
    if name == "dotted":
        assert [o for _, _, o in got[0]] == [0, 1, 1, 0, 0]
    if name == "seventy":
        assert max(o for _, _, o in got[2]) == 69
    for W in (16, 64, 160):
        check_snippets(name, W)


# 6. malformed document
def test_malformed_document_has_no_matches_and_a_head_snippet():
    got = check_matches("malformed")
    assert got[1] == [] and got[2] == [] and got[4] == [] and got[0] and got[3]
    s = check_snippets("malformed", 16)
    assert (s[4][0], len(s[4][1])) == (0, 15)                       # snapped back to a character boundary
    check_snippets("malformed", 64)


# 7. snippets
@pytest.mark.parametrize("W", [16, 64, 160, 1024])
@pytest.mark.parametrize("name", ["edge", "unicode", "ops"])
def test_snippets(name, W):
    check_snippets(name, W)


def test_snippets_of_a_document_with_thousands_of_matches():
    for W in (16, 160, 1024):
        got = check_snippets("dense", W)
        assert got[0][2]
    assert len(H.expected_matches("dense")[0]) >= 5000


@pytest.mark.parametrize("W", [15, 65537, 0])
def test_snippet_width_out_of_range(W):
    g = index_of("ops")
    with pytest.raises(L.TfidfError) as e:
        g.snippets(b"alpha", [0], W)
    assert e.value.code == L.E_INVALID_ARG


def test_widest_snippet():
    check_snippets("han", 65536)


# 8. buffer protocol
def test_buffer_protocol():
    lib = L.load()
    texts, q, _ = H.corpus("edge")
    g = index_of("edge")
    docs = np.arange(40, 72, dtype=np.uint32)
    n = len(docs)
    with g.reader() as rd:
        st, ln, od, offs, ms = rd.matches_arrays(q, docs)
        total = len(st)
        assert total == int(offs[n]) > 100 and ms > 0
        # sizes: cap 0, NULL payload
        o2 = np.full(n + 1, 7, np.uint64)
        nn = C.c_uint64()
        rc = lib.tfidf_reader_matches(rd._h, q, len(q), L.ptr(docs, C.c_uint32), n, None, None, None, 0,
                                      L.ptr(o2, C.c_uint64), C.byref(nn), None)
        assert rc == L.E_BUFFER and nn.value == total and (o2 == offs).all()
        # one below the total
        cap = total - 1
        s2, l2, d2 = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        o2[:] = 7
        rc = lib.tfidf_reader_matches(rd._h, q, len(q), L.ptr(docs, C.c_uint32), n, L.ptr(s2, C.c_uint64),
                                      L.ptr(l2, C.c_uint32), L.ptr(d2, C.c_uint32), cap, L.ptr(o2, C.c_uint64),
                                      C.byref(nn), None)
        assert rc == L.E_BUFFER and nn.value == total and (o2 == offs).all()
        # snippets: text_cap and m_cap one below, and the sizes alone
        full = rd.snippets_arrays(q, docs, 160)
        text, t_offs, d_starts, sst, _, _, m_offs, _ = full
        nt, nm = len(text), len(sst)
        assert nt == int(t_offs[n]) and nm == int(m_offs[n]) > 0

        def call(t_cap, m_cap, null=False):
            tb = np.zeros(max(t_cap, 1), np.uint8)
            a = [np.zeros(max(m_cap, 1), t) for t in (np.uint64, np.uint32, np.uint32)]
            to, mo, ds = np.full(n + 1, 7, np.uint64), np.full(n + 1, 7, np.uint64), np.zeros(n, np.uint64)
            ct, cm = C.c_uint64(), C.c_uint64()
            rc = lib.tfidf_reader_snippets(rd._h, q, len(q), L.ptr(docs, C.c_uint32), n, 160,
                                           None if null else tb.ctypes.data_as(C.c_void_p), t_cap,
                                           L.ptr(to, C.c_uint64), L.ptr(ds, C.c_uint64),
                                           None if null else L.ptr(a[0], C.c_uint64),
                                           None if null else L.ptr(a[1], C.c_uint32),
                                           None if null else L.ptr(a[2], C.c_uint32), m_cap, L.ptr(mo, C.c_uint64),
                                           C.byref(ct), C.byref(cm), None)
            assert (ct.value, cm.value) == (nt, nm)
            assert (to == t_offs).all() and (mo == m_offs).all() and (ds == d_starts).all()
            return rc
        assert call(nt - 1, nm) == L.E_BUFFER
        assert call(nt, nm - 1) == L.E_BUFFER
        assert call(0, 0, null=True) == L.E_BUFFER
        assert call(nt, nm) == L.OK
        # documents: out of range writes nothing; none is fine
        bad = np.array([0, H.N_EDGE], np.uint32)
        o3 = np.full(3, 7, np.uint64)
        nn.value = 99
        rc = lib.tfidf_reader_matches(rd._h, q, len(q), L.ptr(bad, C.c_uint32), 2, None, None, None, 0,
                                      L.ptr(o3, C.c_uint64), C.byref(nn), None)
        assert rc == L.E_INVALID_ARG and (o3 == 7).all() and nn.value == 99
        assert rd.matches(q, []) == [] and rd.snippets(q, []) == []
        # query errors as in tfidf_search; a query without a present term: nothing, head snippets
        for bq, code in ((b"AND x", L.E_QUERY_SYNTAX), (b"x \xff", L.E_UNSUPPORTED_QUERY)):
            with pytest.raises(L.TfidfError) as e:
                rd.matches(bq, [0])
            assert e.value.code == code
            # ... and before any document check: the query's error wins, nothing is written
            pay = [np.full(4, 7, t) for t in (np.uint64, np.uint32, np.uint32)]
            pp = [L.ptr(a, t) for a, t in zip(pay, (C.c_uint64, C.c_uint32, C.c_uint32))]
            tb, to, ds = np.full(320, 7, np.uint8), np.full(3, 7, np.uint64), np.full(2, 7, np.uint64)
            ct = C.c_uint64(99)
            o3[:] = 7
            nn.value = 99
            assert lib.tfidf_reader_matches(rd._h, bq, len(bq), L.ptr(bad, C.c_uint32), 2, *pp, 4,
                                            L.ptr(o3, C.c_uint64), C.byref(nn), None) == code
            assert lib.tfidf_reader_snippets(rd._h, bq, len(bq), L.ptr(bad, C.c_uint32), 2, 160,
                                             tb.ctypes.data_as(C.c_void_p), 320, L.ptr(to, C.c_uint64),
                                             L.ptr(ds, C.c_uint64), *pp, 4, L.ptr(o3, C.c_uint64), C.byref(ct),
                                             C.byref(nn), None) == code
            assert all((a == 7).all() for a in pay + [tb, to, ds, o3]) and (ct.value, nn.value) == (99, 99)
        assert rd.matches(b"nosuchword NOT alpha", [60, 61]) == [[], []]
        assert rd.snippets(b"nosuchword", [62], 64) == [(0, texts[62][:64], [])]


# 9. snapshot
def test_reader_keeps_its_snapshot_and_calls_run_beside_commits():
    old, new = b"alpha one beta. " * 30 + b"gamma", b"delta gamma two. " * 30 + b"alpha alpha"
    q, terms = b"alpha gamma", [b"alpha", b"gamma"]
    exp = {t: (H.matches(t, terms), H.snippet(t, H.matches(t, terms), 64)) for t in (old, new)}
    filler = [H.edge_doc(i, 300) for i in range(20)]
    g = ShardIndex()
    g.add_documents([old] + filler, [b"k"] + [b"f%d" % i for i in range(20)])
    g.commit()
    rd = g.reader()
    g.add_documents([new], [b"k"])                                  # replaces "k": the new text is the last document
    g.commit()
    g.compact()
    g.commit()

    def observe(h, d):
        (m,), ((a, text, ms),) = h.matches(q, [d]), h.snippets(q, [d], 64)
        return m, (a, a + len(text), ms)
    assert observe(rd, 0) == exp[old]
    assert rd.snippets(q, [0], 64)[0][1] == old[exp[old][1][0]:exp[old][1][1]]
    nd = g.stats()["num_docs"] - 1
    assert g.doc_text(nd) == new and observe(g, nd) == exp[new]
    assert observe(rd, 0) == exp[old]
    rd.close()
    # one thread commits while another asks for snippets of the replaced document
    seen, loose, errs = [], [], []

    def writer():
        try:
            for i in range(5):
                g.add_documents([old if i % 2 == 0 else new], [b"k"])
                g.commit()
        except Exception as e:                                      # pragma: no cover
            errs.append(e)

    def asker():
        try:
            for _ in range(12):
                with g.reader() as r:
                    seen.append((r.doc_text(r.num_docs - 1), observe(r, r.num_docs - 1)))
                loose.append(observe(g, g.stats()["num_docs"] - 1))   # two calls: maybe two snapshots
        except Exception as e:                                      # pragma: no cover
            errs.append(e)
    ts = [threading.Thread(target=writer), threading.Thread(target=asker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errs == []
    assert len(seen) == len(loose) == 12
    for text, ob in seen:
        assert text in (old, new) and ob == exp[text]
    for m, sn in loose:
        assert m in (exp[old][0], exp[new][0]) and sn in (exp[old][1], exp[new][1])
    g.close()


# 10. Worker.search_snippets
def test_worker_search_snippets(lucene_fixture):
    w = Worker()
    texts = [d["text"].encode() for d in lucene_fixture["docs"]]
    names = [d["name"] for d in lucene_fixture["docs"]]
    w.index.add_documents(texts, [n.encode() for n in names])
    w.commit()
    for query in ("fast food", "best wireless earbuds", "kheder"):
        q = query.encode()
        terms = H.plain_terms(q)
        top = w.index.search(q, 5)
        out = w.search_snippets(query, k=5, max_bytes=48)
        assert len(out) == len(top) > 0
        for info, (d, score) in zip(out, top):
            assert info["document"]["name"] == names[d]
            assert np.float32(info["score"]).view(np.int32) == np.float32(score).view(np.int32)
            a, b, ms = H.snippet(texts[d], H.matches(texts[d], terms), 48)
            assert info["snippet"] == texts[d][a:b].decode()
            assert info["matches"] == [[s, l] for s, l, _ in ms] and info["matches"]
        assert [i["document"]["name"] for i in w.search_index(query)][:len(top)] == [i["document"]["name"] for i in out]
    assert w.search_snippets("zzzznothing") == []
    w.close()
