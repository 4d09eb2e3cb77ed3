"""Exact phrase search on the device (tfidf_search_phrase_batch, its single,
reader and Worker forms) against phrase_ref.py, compared exactly: ids, order,
freq and float32 score bits over every phrase of the case.  One committed
index holds the corpora of phrase_ref side by side; the expected value of every
phrase comes from phrase_ref (the oracle) alone."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import highlight_ref as H
import phrase_ref as P
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

_state = {}


def index():
    """The committed index over all corpora, shared by the tests (never changed)."""
    if "g" not in _state:
        g = ShardIndex()
        g.add_documents(list(P.TEXTS), [b"d/%05d" % i for i in range(len(P.TEXTS))])
        g.commit()
        _state["g"] = g
        _state["ref"] = P.PhraseRef(P.TEXTS)
    return _state["g"]


def ref():
    index()
    return _state["ref"]


@functools.lru_cache(maxsize=None)
def want(phrase):
    return P.exact(ref().search(phrase))


def batch():
    """The mixed batch: every phrase of the case, duplicates of two, phrases
    without work at the front, in the middle and at the end."""
    ph = list(P.PHRASES)
    return ([P.NO_WORK[0], P.NO_WORK[2]] + ph[:9] + [P.NO_WORK[1], ph[0], P.NO_WORK[3], P.NO_WORK[2]] + ph[9:] +
            [ph[12], P.NO_WORK[1], P.NO_WORK[0]])


def exact_lists(lists):
    return [P.exact(h) for h in lists]


def whole():
    """The mixed batch's arrays from one unchunked call (shared: the Han and
    the 40 000-letter documents are one lane's work each, seconds per call)."""
    if "whole" not in _state:
        g = index()
        b = batch()
        _state["whole"] = g.search_phrase_batch_arrays(b)
        assert g.last_phrase_stats() == (sum(len(ref().candidates(p)) for p in b), 1)
    return _state["whole"]


# 1. the mixed batch
def test_the_mixed_batch():
    g = index()
    b = batch()
    got = exact_lists(E_lists(whole()))
    assert len(got) == len(b)
    for p, h in zip(b, got):
        assert h == want(p), p[:24]
    # the fixture reaches its cases
    by = dict(zip(b, got))
    for p, stated in P.STATED:
        f = {d: fr for d, _, fr in by[p]}
        for d, n in stated.items():
            assert f.get(d, 0) == n, (p[:16], d)
    assert all(by[p] == [] for p in P.NO_WORK)
    assert [d for d, _, _ in by[P.SEVENTY]] == [P.doc("seventy", 2)]
    assert [(d, f) for d, _, f in by[P.TWINS]] == [(P.doc("twins", 0), 1)]
    assert [(d, f) for d, _, f in by[P.ISTANBUL]] == [(P.doc("unicode", 1), 1)]
    assert [(d, f) for d, _, f in by[P.PHRASE_1024]] == [(P.doc("long"), 2)]
    assert len(by[b"alpha beta"]) >= 5 and len(ref().candidates(b"alpha beta")) > len(by[b"alpha beta"])
    quick = [p for p in b if p != b"a" * 510 and P.doc("han") not in {d for d, _, _ in by[p]}]   # one lane's seconds
    with g.reader() as rd:
        assert exact_lists(rd.search_phrase_batch(quick)) == [by[p] for p in quick] and len(quick) > 20
    assert g.search_phrase_batch([]) == []                           # n_p = 0


# 2. one term: the term search, bit for bit
@pytest.mark.parametrize("term", P.SINGLE)
def test_one_term_phrase_is_the_term_search(term):
    g = index()
    got = g.search_phrase(term)
    hits = g.search(term, 0)
    assert [(d, P.bits(s)) for d, s, _ in got] == [(d, P.bits(s)) for d, s in hits] and hits
    assert P.exact(got) == want(term)
    tf = {d: dict(g.doc_terms(d))[P.terms_of(term)[0]] for d, _, _ in got}
    assert all(f == tf[d] for d, _, f in got)


# 3. the single forms are the batch of one
def test_single_forms_equal_the_batch_of_one():
    g = index()
    with g.reader() as rd:
        for p in (b"alpha gamma", b"a" * 600, P.NO_WORK[3], b"", P.PHRASE_1024, b"kappa"):
            one = P.exact(g.search_phrase(p))
            assert one == want(p)
            assert one == P.exact(rd.search_phrase(p)) == P.exact(g.search_phrase_batch([p])[0])


# 4. row chunks
def equal_arrays(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and (x.view(np.uint32 if x.dtype == np.float32 else x.dtype) ==
                                                              y.view(np.uint32 if y.dtype == np.float32 else y.dtype)).all()


@pytest.mark.parametrize("knob, value", [("TFIDF_HL_CHUNK_ITEMS", "1"), ("TFIDF_HL_CHUNK_ITEMS", "2"),
                                         ("TFIDF_HL_CHUNK_ITEMS", "7"), ("TFIDF_HL_CHUNK_MATCHES", "1"),
                                         ("TFIDF_HL_CHUNK_MATCHES", "2"), ("TFIDF_HL_CHUNK_MATCHES", "101"),
                                         ("TFIDF_ALLHITS_CHUNK", "1"), ("TFIDF_ALLHITS_CHUNK", "3"), ("all", "3/3/7")])
def test_any_chunking_gives_the_unchunked_output(knob, value, monkeypatch):
    g = index()
    b = batch()
    cand = sum(len(ref().candidates(p)) for p in b)
    unchunked = whole()
    with g.reader() as rd:
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        if knob == "all":
            for k, v in zip(("TFIDF_ALLHITS_CHUNK", "TFIDF_HL_CHUNK_ITEMS", "TFIDF_HL_CHUNK_MATCHES"), value.split("/")):
                monkeypatch.setenv(k, v)
        else:
            monkeypatch.setenv(knob, value)
        equal_arrays(rd.search_phrase_batch_arrays(b), unchunked)
        n_cand, n_chunks = g.last_phrase_stats()
        assert n_cand == cand and 1 < n_chunks <= cand


def E_lists(arrays):
    from tfidf_amd import engine as E
    return E._phrase_lists(*arrays)


# 5. buffer protocol
def raw(h, phrases, cap, null=False, fill=7, reader=True, offs=None):
    lib = L.load()
    n_p = len(phrases)
    p_offs = np.zeros(n_p + 1, np.uint64)
    p_offs[1:] = np.cumsum([len(p) for p in phrases], dtype=np.uint64)
    if offs is not None:
        p_offs = np.asarray(offs, np.uint64)
    o = {"d": np.full(max(cap, 1), fill, np.uint32), "s": np.full(max(cap, 1), fill, np.float32),
         "f": np.full(max(cap, 1), fill, np.uint32), "o": np.full(n_p + 1, fill, np.uint64)}
    n = C.c_uint64(fill)
    fn = lib.tfidf_reader_search_phrase_batch if reader else lib.tfidf_search_phrase_batch
    rc = fn(h._h, b"".join(phrases), L.ptr(p_offs, C.c_uint64), n_p, None if null else L.ptr(o["d"], C.c_uint32),
            None if null else L.ptr(o["s"], C.c_float), None if null else L.ptr(o["f"], C.c_uint32), cap,
            L.ptr(o["o"], C.c_uint64), C.byref(n))
    return rc, o, n.value


def untouched(o, n):
    return all((a == 7).all() for a in o.values()) and n == 7


@pytest.mark.parametrize("chunk", [None, "2"])
def test_buffer_protocol(chunk, monkeypatch):
    """Sizes alone, one slot short, an exact fit: the offsets and the total are
    those of the successful call, also with the hits spread over row chunks."""
    if chunk:
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        monkeypatch.setenv("TFIDF_HL_CHUNK_ITEMS", chunk)
    g = index()
    b = [b"alpha beta", P.NO_WORK[3], b"beta gamma", b"alpha", b""]
    with g.reader() as rd:
        docs, scores, freqs, offs = rd.search_phrase_batch_arrays(b)
        total = len(docs)
        assert total == int(offs[-1]) > 15 and [int(offs[i + 1] - offs[i]) for i in range(5)] == [len(want(p)) for p in b]
        for cap, null in ((0, True), (total - 1, False), (1, False)):
            rc, o, n = raw(rd, b, cap, null)
            assert rc == L.E_BUFFER and n == total and (o["o"] == offs).all()
        rc, o, n = raw(rd, b, total)
        assert rc == L.OK and n == total and (o["o"] == offs).all()
        assert (o["d"] == docs).all() and (o["s"].view(np.uint32) == scores.view(np.uint32)).all() and (o["f"] == freqs).all()
        if chunk:
            assert g.last_phrase_stats()[1] > 3
        rc, o, n = raw(rd, [P.NO_WORK[2], b""], 0, null=True)       # no hits: nothing to fit
        assert rc == L.OK and n == 0 and (o["o"] == 0).all()


# 6. argument errors: nothing written
def test_argument_errors_write_nothing():
    g = index()
    with g.reader() as rd:
        for reader, h in ((True, rd), (False, g)):
            rc, o, n = raw(h, [b"alpha", P.PHRASE_1025, b"beta"], 64, reader=reader)
            assert rc == L.E_INVALID_ARG and untouched(o, n)
            rc, o, n = raw(h, [b"alpha", b"beta"], 64, reader=reader, offs=[0, 5, 4])
            assert rc == L.E_INVALID_ARG and untouched(o, n)
            rc, o, n = raw(h, [b"alpha", b"beta"], 64, reader=reader, offs=[1, 5, 9])
            assert rc == L.E_INVALID_ARG and untouched(o, n)
        rc, o, n = raw(rd, [b"alpha", P.PHRASE_1024], 64)
        assert rc == L.OK and not untouched(o, n)
    with pytest.raises(L.TfidfError) as e:
        g.search_phrase(P.PHRASE_1025)
    assert e.value.code == L.E_INVALID_ARG
    fresh = ShardIndex()
    for call in (lambda: fresh.search_phrase(b"alpha"), lambda: fresh.search_phrase_batch([b"alpha", b"beta"])):
        with pytest.raises(L.TfidfError) as e:
            call()
        assert e.value.code == L.E_STATE
    fresh.close()


# 7. hashed keys under forced collisions
@pytest.mark.parametrize("how", ["weak", "attempt"])
def test_twin_phrases_under_other_hash_seeds(how, monkeypatch):
    texts = list(H.corpus("twins")[0]) + [H.TWIN_A[1] + b" " + H.TWIN_A[0] + b" " + H.TWIN_A[1]]
    g = ShardIndex()
    if how == "weak":
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    else:
        g.set_hash_attempt(2)
    g.add_documents(texts)
    g.commit()
    if how == "weak":
        assert g.stats()["hash_rebuilds"] == 1
    else:
        assert g.stats()["hash_seed"] != 0
    r = P.PhraseRef(texts)
    phrases = [P.TWINS, H.TWIN_A[1] + b" " + H.TWIN_A[0], H.TWIN_A[1] + b" " + H.TWIN_A[1], H.TWIN_A[0],
               H.TWIN_U[0] + b" " + H.TWIN_U[1], H.TWIN_A[1] + b" " + H.TWIN_U[1]]
    got = exact_lists(g.search_phrase_batch(phrases))
    assert got == [P.exact(r.search(p)) for p in phrases]
    assert sorted(d for d, _, _ in got[0]) == [0, 3] and [d for d, _, _ in got[1]] == [3] and got[2] == []
    assert [d for d, _, _ in got[5]] == [1] and len(got[3]) == 3
    r.close()
    g.close()


# 8. deletes, replacements, compaction
def test_deleted_and_replaced_documents():
    texts = [b"alpha beta one", b"beta alpha two", b"x alpha beta alpha beta", b"alpha, beta", b"gamma alpha beta"]
    g = ShardIndex()
    g.add_documents(texts, [b"k%d" % i for i in range(5)])
    g.commit()
    assert g.delete_documents([b"k0"]) == 1
    g.add_documents([b"no phrase here: beta alpha"], [b"k2"])         # replaces k2
    g.add_documents([b"alpha beta alpha beta alpha beta"], [b"k5"])
    g.commit()
    live = [g.doc_text(d) for d in range(g.stats()["num_docs"])]
    assert len(live) == 5 and texts[0] not in live and texts[2] not in live
    r = P.PhraseRef(live)
    phrases = [b"alpha beta", b"beta alpha", b"alpha", b"two"]
    before = exact_lists(g.search_phrase_batch(phrases))
    assert before == [P.exact(r.search(p)) for p in phrases]
    assert [f for _, _, f in before[0]] == [3, 1, 1] and before[1] and before[3]
    g.compact()
    g.commit()
    assert [g.doc_text(d) for d in range(g.stats()["num_docs"])] == live
    assert exact_lists(g.search_phrase_batch(phrases)) == before
    r.close()
    g.close()


# 9. snapshots
def test_reader_keeps_its_snapshot_beside_commits():
    old, new = b"alpha beta. " * 30 + b"gamma", b"beta alpha " * 20 + b"alpha beta"
    filler = [H.edge_doc(i, 300) for i in range(20)]
    g = ShardIndex()
    g.add_documents([old] + filler, [b"k"] + [b"f%d" % i for i in range(20)])
    g.commit()
    r_old = P.PhraseRef([old] + filler)
    r_new = P.PhraseRef(filler + [new])
    phrases = [b"alpha beta", b"beta alpha", b"beta gamma"]
    exp = {0: [P.exact(r_old.search(p)) for p in phrases], 1: [P.exact(r_new.search(p)) for p in phrases]}
    assert exp[0] != exp[1]
    rd = g.reader()
    g.add_documents([new], [b"k"])
    g.commit()
    assert exact_lists(rd.search_phrase_batch(phrases)) == exp[0]
    assert exact_lists(g.search_phrase_batch(phrases)) == exp[1]
    errs, seen = [], []

    def writer():
        try:
            for i in range(4):
                g.add_documents([H.edge_doc(100 + i, 200)], [b"w%d" % i])
                g.commit()
        except Exception as e:                                      # pragma: no cover
            errs.append(e)

    def asker():
        try:
            for _ in range(8):
                seen.append(exact_lists(rd.search_phrase_batch(phrases)))
        except Exception as e:                                      # pragma: no cover
            errs.append(e)
    ts = [threading.Thread(target=writer), threading.Thread(target=asker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errs == [] and len(seen) == 8 and all(s == exp[0] for s in seen)
    rd.close()
    for r in (r_old, r_new):
        r.close()
    g.close()


# 10. k1 / b other than the defaults (two pairs of test_gpu_bm25_params.py's set)
@pytest.mark.parametrize("k1, b", [(2.0, 1.0), (1.2, 0.0)])
def test_other_bm25_parameters(k1, b):
    texts = P.TEXTS[P.doc("ops"):P.doc("unicode")] + list(H.corpus("dup")[0]) + [b"a a a"]
    g = ShardIndex(k1=k1, b=b)
    g.add_documents(list(texts))
    g.commit()
    r = P.PhraseRef(texts, k1, b)
    phrases = [b"alpha beta", b"beta gamma", b"lambda alpha", b"alpha", b"a a", b"beta beta"]
    got = exact_lists(g.search_phrase_batch(phrases))
    assert got == [P.exact(r.search(p)) for p in phrases] and all(got)
    d = P.PhraseRef(texts)
    assert got[0] != P.exact(d.search(phrases[0]))                  # the parameters reach the score
    hits = g.search(b"alpha", 0)
    assert [(x, P.bits(s)) for x, s, _ in g.search_phrase(b"alpha")] == [(x, P.bits(s)) for x, s in hits]
    for x in (r, d):
        x.close()
    g.close()


# 11. Worker.search_phrase
def test_worker_search_phrase(lucene_fixture):
    w = Worker()
    texts = [d["text"].encode() for d in lucene_fixture["docs"]]
    names = [d["name"] for d in lucene_fixture["docs"]]
    w.index.add_documents(texts, [n.encode() for n in names])
    w.commit()
    r = P.PhraseRef(texts)
    toks = [t for t in P.terms_of(texts[0])]
    two = (toks[0] + b" " + toks[1]).decode()
    for q in (two, "fast food", "zzzznothing at all", ""):
        exp = r.search(q.encode())
        assert w.search_phrase(q) == [{"document": {"name": names[d]}, "score": float(s), "freq": f} for d, s, f in exp], q
    one = toks[0].decode()
    assert [dict(h, freq=None) for h in w.search_phrase(one)] == [dict(h, freq=None) for h in w.search_index(one)]
    assert w.search_phrase(two)
    w.close()
    r.close()
