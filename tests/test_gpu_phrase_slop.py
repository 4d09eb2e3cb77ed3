"""Sloppy phrase search on the device (tfidf_search_phrase_slop_batch, its
single, reader and Worker forms) against phrase_slop_ref.py, compared exactly:
ids, order, float32 frequency bits and float32 score bits.  One committed index
holds phrase_slop_ref's documents; the expected value of every (phrase, slop)
comes from phrase_slop_ref (the oracle) alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import highlight_ref as H
import phrase_ref as P
import phrase_slop_ref as S
from tfidf_amd import _lib as L
from tfidf_amd import engine as E
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

_state = {}


def index():
    """The committed index over all corpora, shared by the tests (never changed)."""
    if "g" not in _state:
        g = ShardIndex()
        g.add_documents(list(S.TEXTS), [b"d/%05d" % i for i in range(len(S.TEXTS))])
        g.commit()
        _state["g"] = g
        _state["ref"] = P.PhraseRef(S.TEXTS)
    return _state["g"]


def ref():
    index()
    return _state["ref"]


@functools.lru_cache(maxsize=None)
def want(phrase, slop):
    return S.exact(S.search(ref(), phrase, slop))


def batch():
    """The mixed batch of (phrase, slop): the stated rows, every stated phrase
    at further slops, one phrase twice running with two slops, phrases without
    work at the front, in the middle and at the end, 64 terms at slop 5,
    repeats and long phrases at slop 0, one-term phrases."""
    stated = [(p, s) for _, p, s, _, _ in S.STATED]
    more = [(p, s) for p in sorted({p for p, _ in stated}) for s in (0, 7, 2 ** 31 - 1, 2 ** 32 - 1)]
    b = [(S.NO_WORK[0], 3), (S.NO_WORK[2], 0)] + stated + [(b"a b", 1), (b"a b", 2), (b"b x a", 2), (b"b x a", 3),
                                                           (b"b x a", 7), (S.NO_WORK[1], 1), (S.NO_WORK[3], 2)]
    b += more + [(S.M64, 5), (S.M64, 0), (S.M65, 0), (b"beta beta", 0), (b"a a", 0), (P.PHRASE_1024, 0), (P.SEVENTY, 0)]
    b += [(p, s) for p in (b"alpha gamma", b"gamma alpha", b"alpha beta", b"beta alpha", b"lambda alpha", P.TWINS,
                           P.ISTANBUL, b"gamma alpha beta", b"a x b", b"beta.gamma beta") for s in (2, 1)]
    b += [(t, 9) for t in (b"alpha", b"kappa", b"beta.gamma")] + [(b"alpha", 0)]
    return b + [(S.NO_WORK[2], 4), (S.NO_WORK[0], 0)]


def split(b):
    return [p for p, _ in b], [s for _, s in b]


def exact_lists(lists):
    return [S.exact(h) for h in lists]


def whole():
    """The mixed batch's arrays from one unchunked call."""
    if "whole" not in _state:
        g = index()
        b = batch()
        _state["whole"] = g.search_phrase_slop_batch_arrays(*split(b))
        assert g.last_phrase_stats() == (sum(len(ref().candidates(p)) for p, _ in b), 1)
    return _state["whole"]


# 1. the mixed batch
def test_the_mixed_batch():
    g = index()
    b = batch()
    arrays = whole()
    assert arrays[2].dtype == np.float32
    got = exact_lists(E._phrase_lists(*arrays))
    assert len(got) == len(b)
    for (p, s), h in zip(b, got):
        assert h == want(p, s), (p[:24], s)
    by = dict(zip(b, got))
    # the fixture reaches its cases: the stated table, on the documents it names
    for d, p, s, f, _ in S.STATED:
        fr = {x: y for x, _, y in by[(p, s)]}
        if f:
            assert fr[S.doc("near", d)] == S.bits(np.float32(f)), (d, p, s)
        else:
            assert S.doc("near", d) not in fr, (d, p, s)
    assert by[(b"a b", 1)] != by[(b"a b", 2)]
    rep = {x: y for x, _, y in by[(b"b x a", 3)]}[S.doc("rep")]
    assert rep == S.bits(S.sloppy_matches(P.terms_of(S.REP[0]), P.terms_of(b"b x a"), 3)[0])
    assert {x: y for x, _, y in by[(b"a b", 1)]}[S.doc("rep")] == S.bits(np.float32(3000.0))
    assert [(d, f) for d, _, f in by[(S.M64, 5)]] == [(S.doc("long"), S.bits(np.float32(16.0)))]
    assert [(d, f) for d, _, f in by[(P.PHRASE_1024, 0)]] == [(S.doc("long"), S.bits(np.float32(2.0)))]
    assert by[(b"a a", 0)] and by[(b"beta beta", 0)] and by[(P.SEVENTY, 0)]
    assert all(by[(p, s)] == [] for p, s in b if p in S.NO_WORK)
    assert by[(b"beta alpha", 2)] and by[(b"beta alpha", 2)] != by[(b"beta alpha", 1)]
    assert g.search_phrase_slop_batch([], []) == []                  # n_p = 0


# 2. every slop 0: the exact call
def test_all_slops_zero_is_the_exact_batch():
    g = index()
    phrases = S.PHRASES + S.NO_WORK
    docs, scores, freqs, offs = g.search_phrase_slop_batch_arrays(phrases, [0] * len(phrases))
    e_docs, e_scores, e_freqs, e_offs = g.search_phrase_batch_arrays(phrases)
    assert (offs == e_offs).all() and (docs == e_docs).all() and len(docs) > 40
    assert (scores.view(np.uint32) == e_scores.view(np.uint32)).all()
    assert freqs.dtype == np.float32 and (freqs.view(np.uint32) == e_freqs.astype(np.float32).view(np.uint32)).all()


# 3. one term at any slop: the term search, bit for bit
@pytest.mark.parametrize("term", [b"alpha", b"kappa", b"beta.gamma"])
def test_one_term_phrase_is_the_term_search(term):
    g = index()
    got = g.search_phrase_slop(term, 9)
    hits = g.search(term, 0)
    assert [(d, S.bits(s)) for d, s, _ in got] == [(d, S.bits(s)) for d, s in hits] and hits
    assert S.exact(got) == want(term, 9)
    tf = {d: dict(g.doc_terms(d))[P.terms_of(term)[0]] for d, _, _ in got}
    assert all(f == float(tf[d]) for d, _, f in got)


# 4. the single forms are the batch of one
def test_single_forms_equal_the_batch_of_one():
    g = index()
    with g.reader() as rd:
        for p, s in ((b"a b", 2), (b"b x a", 3), (S.NO_WORK[3], 1), (b"", 2), (S.M64, 5), (b"kappa", 1),
                     (b"alpha gamma", 0), (b"c a", 2 ** 32 - 1)):
            one = S.exact(g.search_phrase_slop(p, s))
            assert one == want(p, s)
            assert one == S.exact(rd.search_phrase_slop(p, s)) == S.exact(g.search_phrase_slop_batch([p], [s])[0])
            assert one == S.exact(rd.search_phrase_slop_batch([p], [s])[0])


# 5. row chunks
def equal_arrays(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("knob, value", [("TFIDF_HL_CHUNK_ITEMS", "1"), ("TFIDF_HL_CHUNK_ITEMS", "2"),
                                         ("TFIDF_HL_CHUNK_ITEMS", "7"), ("TFIDF_HL_CHUNK_MATCHES", "1"),
                                         ("TFIDF_HL_CHUNK_MATCHES", "2"), ("TFIDF_HL_CHUNK_MATCHES", "101"),
                                         ("TFIDF_ALLHITS_CHUNK", "1"), ("TFIDF_ALLHITS_CHUNK", "3"), ("all", "3/3/7")])
def test_any_chunking_gives_the_unchunked_output(knob, value, monkeypatch):
    g = index()
    b = batch()
    cand = sum(len(ref().candidates(p)) for p, _ in b)
    unchunked = whole()
    with g.reader() as rd:
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        if knob == "all":
            for k, v in zip(("TFIDF_ALLHITS_CHUNK", "TFIDF_HL_CHUNK_ITEMS", "TFIDF_HL_CHUNK_MATCHES"), value.split("/")):
                monkeypatch.setenv(k, v)
        else:
            monkeypatch.setenv(knob, value)
        equal_arrays(rd.search_phrase_slop_batch_arrays(*split(b)), unchunked)
        n_cand, n_chunks = g.last_phrase_stats()
        assert n_cand == cand and 1 < n_chunks <= cand


# 6. buffer protocol
def raw(h, phrases, slops, cap, null=False, fill=7, reader=True, offs=None, null_slops=False):
    lib = L.load()
    n_p = len(phrases)
    p_offs = np.zeros(n_p + 1, np.uint64)
    p_offs[1:] = np.cumsum([len(p) for p in phrases], dtype=np.uint64)
    if offs is not None:
        p_offs = np.asarray(offs, np.uint64)
    sl = np.asarray(slops, np.uint32)
    o = {"d": np.full(max(cap, 1), fill, np.uint32), "s": np.full(max(cap, 1), fill, np.float32),
         "f": np.full(max(cap, 1), fill, np.float32), "o": np.full(n_p + 1, fill, np.uint64)}
    n = C.c_uint64(fill)
    fn = lib.tfidf_reader_search_phrase_slop_batch if reader else lib.tfidf_search_phrase_slop_batch
    rc = fn(h._h, b"".join(phrases), L.ptr(p_offs, C.c_uint64), None if null_slops else L.ptr(sl, C.c_uint32), n_p,
            None if null else L.ptr(o["d"], C.c_uint32), None if null else L.ptr(o["s"], C.c_float),
            None if null else L.ptr(o["f"], C.c_float), cap, L.ptr(o["o"], C.c_uint64), C.byref(n))
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
    b, sl = [b"alpha beta", S.NO_WORK[3], b"a b", b"alpha", b"", b"beta alpha"], [2, 1, 2, 5, 1, 0]
    with g.reader() as rd:
        docs, scores, freqs, offs = rd.search_phrase_slop_batch_arrays(b, sl)
        total = len(docs)
        assert total == int(offs[-1]) > 15
        assert [int(offs[i + 1] - offs[i]) for i in range(len(b))] == [len(want(p, s)) for p, s in zip(b, sl)]
        for cap, null in ((0, True), (total - 1, False), (1, False)):
            rc, o, n = raw(rd, b, sl, cap, null)
            assert rc == L.E_BUFFER and n == total and (o["o"] == offs).all()
        rc, o, n = raw(rd, b, sl, total)
        assert rc == L.OK and n == total and (o["o"] == offs).all()
        assert (o["d"] == docs).all() and o["s"].tobytes() == scores.tobytes() and o["f"].tobytes() == freqs.tobytes()
        if chunk:
            assert g.last_phrase_stats()[1] > 3
        rc, o, n = raw(rd, [S.NO_WORK[2], b""], [1, 2], 0, null=True)     # no hits: nothing to fit
        assert rc == L.OK and n == 0 and (o["o"] == 0).all()


# 7. argument errors: nothing written
def test_argument_errors_write_nothing():
    g = index()
    with g.reader() as rd:
        for reader, h in ((True, rd), (False, g)):
            rc, o, n = raw(h, [b"alpha", b"beta alpha beta", b"beta"], [1, 1, 1], 64, reader=reader)   # a repeat
            assert rc == L.E_UNSUPPORTED_QUERY and untouched(o, n)
            rc, o, n = raw(h, [b"alpha beta", S.M65], [0, 1], 64, reader=reader)                        # 65 terms
            assert rc == L.E_UNSUPPORTED_QUERY and untouched(o, n)
            rc, o, n = raw(h, [b"alpha", P.PHRASE_1025, b"beta"], [0, 0, 0], 64, reader=reader)
            assert rc == L.E_INVALID_ARG and untouched(o, n)
            rc, o, n = raw(h, [b"alpha", b"beta"], [1, 1], 64, reader=reader, null_slops=True)
            assert rc == L.E_INVALID_ARG and untouched(o, n)
            rc, o, n = raw(h, [b"alpha", b"beta"], [1, 1], 64, reader=reader, offs=[0, 5, 4])
            assert rc == L.E_INVALID_ARG and untouched(o, n)
            rc, o, n = raw(h, [b"alpha", b"beta"], [1, 1], 64, reader=reader, offs=[1, 5, 9])
            assert rc == L.E_INVALID_ARG and untouched(o, n)
        rc, o, n = raw(rd, [b"beta alpha beta", S.M65, S.M64], [0, 0, 64], 64)      # served: slop 0, and 64 terms
        assert rc == L.OK and not untouched(o, n)
    for call in (lambda: g.search_phrase_slop(b"a a", 1), lambda: g.search_phrase_slop(S.M65, 2)):
        with pytest.raises(L.UnsupportedQuery) as e:
            call()
        assert e.value.code == L.E_UNSUPPORTED_QUERY
    with pytest.raises(ValueError):
        g.search_phrase_slop_batch([b"alpha"], [1, 2])
    fresh = ShardIndex()
    for call in (lambda: fresh.search_phrase_slop(b"alpha", 1),
                 lambda: fresh.search_phrase_slop_batch([b"alpha", b"beta"], [1, 0])):
        with pytest.raises(L.TfidfError) as e:
            call()
        assert e.value.code == L.E_STATE
    fresh.close()


# 8. deletes, replacements, compaction
def test_deleted_and_replaced_documents():
    texts = [b"alpha beta one", b"beta alpha two", b"x alpha beta alpha beta", b"alpha, beta", b"gamma alpha x beta"]
    g = ShardIndex()
    g.add_documents(texts, [b"k%d" % i for i in range(5)])
    g.commit()
    assert g.delete_documents([b"k0"]) == 1
    g.add_documents([b"no phrase here: beta x alpha"], [b"k2"])       # replaces k2
    g.add_documents([b"alpha beta alpha y beta alpha beta"], [b"k5"])
    g.commit()
    live = [g.doc_text(d) for d in range(g.stats()["num_docs"])]
    assert len(live) == 5 and texts[0] not in live and texts[2] not in live
    r = P.PhraseRef(live)
    phrases, slops = [b"alpha beta", b"beta alpha", b"alpha", b"alpha beta", b"two"], [1, 3, 2, 0, 1]
    before = exact_lists(g.search_phrase_slop_batch(phrases, slops))
    assert before == [S.exact(S.search(r, p, s)) for p, s in zip(phrases, slops)]
    assert len(before[0]) > len(before[3]) > 0 and before[1] and before[4]
    g.compact()
    g.commit()
    assert [g.doc_text(d) for d in range(g.stats()["num_docs"])] == live
    assert exact_lists(g.search_phrase_slop_batch(phrases, slops)) == before
    r.close()
    g.close()


# 9. snapshots
def test_reader_keeps_its_snapshot_across_a_commit():
    old, new = b"alpha x beta. " * 30 + b"gamma", b"beta alpha " * 20 + b"alpha y y beta"
    filler = [H.edge_doc(i, 300) for i in range(20)]
    g = ShardIndex()
    g.add_documents([old] + filler, [b"k"] + [b"f%d" % i for i in range(20)])
    g.commit()
    r_old = P.PhraseRef([old] + filler)
    r_new = P.PhraseRef(filler + [new])
    phrases, slops = [b"alpha beta", b"beta alpha", b"beta gamma"], [1, 2, 3]
    exp = {0: [S.exact(S.search(r_old, p, s)) for p, s in zip(phrases, slops)],
           1: [S.exact(S.search(r_new, p, s)) for p, s in zip(phrases, slops)]}
    assert exp[0] != exp[1]
    rd = g.reader()
    g.add_documents([new], [b"k"])
    g.commit()
    assert exact_lists(rd.search_phrase_slop_batch(phrases, slops)) == exp[0]
    assert exact_lists(g.search_phrase_slop_batch(phrases, slops)) == exp[1]
    rd.close()
    for r in (r_old, r_new):
        r.close()
    g.close()


# 10. k1 / b other than the defaults
def test_other_bm25_parameters():
    k1, b = 2.0, 1.0
    texts = S.TEXTS[S.doc("ops"):S.doc("unicode")] + list(S.NEAR)
    g = ShardIndex(k1=k1, b=b)
    g.add_documents(list(texts))
    g.commit()
    r = P.PhraseRef(texts, k1, b)
    phrases, slops = [b"alpha beta", b"beta alpha", b"lambda alpha", b"alpha", b"a b", b"c a"], [2, 2, 1, 3, 2, 4]
    got = exact_lists(g.search_phrase_slop_batch(phrases, slops))
    assert got == [S.exact(S.search(r, p, s)) for p, s in zip(phrases, slops)] and all(got)
    d = P.PhraseRef(texts)
    assert got[0] != S.exact(S.search(d, phrases[0], slops[0]))      # the parameters reach the score
    for x in (r, d):
        x.close()
    g.close()


# 11. Worker.search_near
def test_worker_search_near(lucene_fixture):
    w = Worker()
    texts = [d["text"].encode() for d in lucene_fixture["docs"]]
    names = [d["name"] for d in lucene_fixture["docs"]]
    w.index.add_documents(texts, [n.encode() for n in names])
    w.commit()
    r = P.PhraseRef(texts)
    toks = list(dict.fromkeys(P.terms_of(texts[0])))
    two, swapped = (toks[0] + b" " + toks[1]).decode(), (toks[1] + b" " + toks[0]).decode()
    for q, slop in ((two, 0), (two, 2), (swapped, 2), ("fast food", 3), ("zzzznothing at all", 1), ("", 2)):
        exp = S.search(r, q.encode(), slop)
        got = w.search_near(q, slop)
        assert got == [{"document": {"name": names[d]}, "score": float(s), "freq": float(f)} for d, s, f in exp], q
        assert all(isinstance(h["freq"], float) for h in got)
    assert w.search_near(swapped, 2) and w.search_near(two, 0) == [dict(h, freq=float(h["freq"]))
                                                                  for h in w.search_phrase(two)]
    for q in ("fast fast", " ".join("w%d" % i for i in range(65))):
        with pytest.raises(ValueError):
            w.search_near(q, 1)
    w.close()
    r.close()
