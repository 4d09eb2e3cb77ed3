"""Fuzzy term lookup on the device (tfidf_fuzzy_terms[_batch], the reader
forms, Worker.search_did_you_mean) against fuzzy_ref.py, compared exactly: the
same candidate lists, df, dist and n_within as brute force over the oracle's
vocabulary.  The `dense` corpus holds every string over {a, b, c} of 1..6
letters with df 1..5 (many ties) and the special terms: exact and hashed keys
on both sides of their limits, non-ASCII, Han, an emoji and a 255-unit term,
each also spelt in upper case."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import fuzzy_ref as F
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

TERMS = F.dense_terms()
EDITS, PREFIXES, OUTS = (0, 1, 2), (0, 1, 3), (1, 5, 1024)
INVERSIONS = [L.INVERSION_BLOCK, L.INVERSION_TERM]


@functools.lru_cache(maxsize=None)
def _all(term, e, p):
    return F.expected(F.dense_vocab(), term, e, p, 1 << 30)


def want(term, e, p, k):
    lst, n = _all(term, e, p)
    return lst[:k], n


_state = {}


def index(inversion=L.INVERSION_BLOCK):
    """The committed dense index per inversion, shared by the tests (never changed)."""
    if inversion not in _state:
        g = ShardIndex(vocab_capacity_log2=16, inversion=inversion)
        texts = F.dense_texts()
        g.add_documents(texts, [b"d%05d" % i for i in range(len(texts))])
        g.commit()
        assert g.stats()["term_major"] == (1 if inversion == L.INVERSION_TERM else 0)
        _state[inversion] = g
    return _state[inversion]


# 1, 3. the whole batch, every parameter, both inversions
@pytest.mark.parametrize("inversion", INVERSIONS)
@pytest.mark.parametrize("max_edits", EDITS)
def test_batch_equals_the_reference(inversion, max_edits):
    g = index(inversion)
    for p in PREFIXES:
        for k in OUTS:
            got = g.fuzzy_terms_batch(TERMS, max_edits, p, k)
            assert len(got) == len(TERMS)
            for t, gt in zip(TERMS, got):
                assert gt == want(t, max_edits, p, k), (t[:40], max_edits, p, k)
    assert g.last_fuzzy_chunks()[0] >= 2                    # the batch does not fit one staging of the scan
    # the fixture reaches its cases
    a = want(b"a", 2, 0, 5)
    assert a[1] > 30 and len(a[0]) == 5
    assert want(b"", 2, 0, 5) == want(b"\xff\xfe", 2, 0, 5) == want(b"l" * 256, 2, 0, 5) == ([], 0)
    assert all(want(s, 0, 0, 5) == ([(s, 2, 0)], 1) for s in F.SPECIALS)
    assert want(b"zzzzzzzzzzzz", 2, 0, 5) == ([], 0)


# 2, 3. the single calls are the batch of one
@pytest.mark.parametrize("inversion", INVERSIONS)
def test_single_calls_equal_the_batch_of_one(inversion):
    g = index(inversion)
    some = [b"a", b"ABCA", F.CAFES[0], F.LONG255[1:], F.ASCII_SPECIALS[3][:-1], F.UNI_SPECIALS[1], F.EMOJI, b"",
            b"\xff\xfe", b"xyz"]
    with g.reader() as rd:
        for t in some:
            for e, p, k in ((2, 0, 5), (1, 1, 1024), (0, 3, 1)):
                w = want(t, e, p, k)
                assert g.fuzzy_terms(t, e, p, k) == w, (t[:40], e, p, k)
                assert rd.fuzzy_terms(t, e, p, k) == w
                assert g.fuzzy_terms_batch([t], e, p, k) == [w] == rd.fuzzy_terms_batch([t], e, p, k)
    assert g.fuzzy_terms_batch([]) == []                    # n_terms = 0 is legal


# 4. candidate budgets: any split gives the same output
@pytest.mark.parametrize("budget", ["1", "7", "100"])
def test_any_candidate_budget_gives_the_same_output(budget, monkeypatch):
    g = index()
    with g.reader() as rd:
        whole = rd.fuzzy_terms_batch_arrays(TERMS, 2, 0, 5)
        scans, fills = g.last_fuzzy_chunks()
        assert fills == scans                               # everything fitted: one candidate chunk per scan
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        monkeypatch.setenv("TFIDF_FUZZY_CAND_BUDGET", budget)
        split = rd.fuzzy_terms_batch_arrays(TERMS, 2, 0, 5)
        for a, b in zip(split[:6], whole[:6]):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        s2, f2 = g.last_fuzzy_chunks()
        assert s2 == scans and f2 > fills and f2 > 1
        if budget == "1":                                   # one term per chunk: every term with candidates alone
            assert f2 == sum(1 for t in TERMS if want(t, 2, 0, 5)[1])


# 5. buffer protocol and argument errors
def _raw(g, terms, max_edits, prefix_len, max_out, cand_cap, terms_cap, payload=True):
    from tfidf_amd.engine import _key_arrays
    blob, t_offs = _key_arrays(terms)
    n = len(terms)
    c_offs = np.full(n + 1, 77, np.uint64)
    within = np.full(max(n, 1), 77, np.uint64)
    nc, nb = C.c_uint64(77), C.c_uint64(77)
    t_out = np.zeros(cand_cap + 1, np.uint64)
    text = np.zeros(max(terms_cap, 1), np.uint8)
    df = np.zeros(max(cand_cap, 1), np.uint32)
    dist = np.zeros(max(cand_cap, 1), np.uint8)
    rc = L.load().tfidf_fuzzy_terms_batch(
        g._h, blob, L.ptr(t_offs, C.c_uint64), n, max_edits, prefix_len, max_out, L.ptr(c_offs, C.c_uint64),
        L.ptr(within, C.c_uint64), L.ptr(t_out, C.c_uint64) if payload else None,
        text.ctypes.data_as(C.c_void_p) if payload else None, terms_cap, L.ptr(df, C.c_uint32) if payload else None,
        L.ptr(dist, C.c_uint8) if payload else None, cand_cap, C.byref(nc), C.byref(nb), None)
    return rc, c_offs.tolist(), within[:n].tolist(), nc.value, nb.value


def test_buffer_protocol_and_argument_errors():
    g = index()
    terms = [b"a", F.CAFES[1], b"", F.LONG255[:-1], b"xyz"]
    full = g.fuzzy_terms_batch(terms, 2, 0, 5)
    n_c = sum(len(c) for c, _ in full)
    n_b = sum(len(t) for c, _ in full for t, _, _ in c)
    offs = [0]
    for c, _ in full:
        offs.append(offs[-1] + len(c))
    within = [w for _, w in full]
    assert n_c > 5 and n_b > 255
    # the size query: caps 0, NULL payload pointers
    assert _raw(g, terms, 2, 0, 5, 0, 0, payload=False) == (L.E_BUFFER, offs, within, n_c, n_b)
    # one candidate slot short, one term byte short: offsets, n_within and totals still in full
    assert _raw(g, terms, 2, 0, 5, n_c - 1, n_b) == (L.E_BUFFER, offs, within, n_c, n_b)
    assert _raw(g, terms, 2, 0, 5, n_c, n_b - 1) == (L.E_BUFFER, offs, within, n_c, n_b)
    assert _raw(g, terms, 2, 0, 5, n_c, n_b) == (L.OK, offs, within, n_c, n_b)
    # nothing to return: OK with the caps at 0
    assert _raw(g, [b"zzzzzzzzzzzz", b""], 2, 0, 5, 0, 0, payload=False) == (L.OK, [0, 0, 0], [0, 0], 0, 0)
    assert _raw(g, [], 2, 0, 5, 0, 0, payload=False)[0] == L.OK
    # argument errors: nothing written
    untouched = [77] * (len(terms) + 1)
    for e, k in ((3, 5), (2, 0), (2, 1025)):
        rc, o, w, a, b = _raw(g, terms, e, 0, k, n_c, n_b)
        assert rc == L.E_INVALID_ARG and o == untouched and w == [77] * len(terms) and (a, b) == (77, 77)
    many = [b"a"] * 65537
    assert _raw(g, many, 2, 0, 1, 0, 0, payload=False)[0] == L.E_INVALID_ARG
    with pytest.raises(L.TfidfError) as ei:
        g.fuzzy_terms(b"a", 3)
    assert ei.value.code == L.E_INVALID_ARG
    # before the first commit
    fresh = ShardIndex(vocab_capacity_log2=12)
    fresh.add_documents([b"abc"])
    with pytest.raises(L.TfidfError) as ei:
        fresh.fuzzy_terms_batch([b"abc"])
    assert ei.value.code == L.E_STATE
    with pytest.raises(L.TfidfError) as ei:
        fresh.fuzzy_terms(b"abc")
    assert ei.value.code == L.E_STATE
    fresh.close()


# 6. hashed keys under forced collisions
def test_long_terms_under_a_weak_hash(monkeypatch):
    twins = [F.ASCII_SPECIALS[3][:-1] + b"k", "àéîõüçñy".encode()]           # same length, same first 8 bytes
    texts = F.dense_texts() + twins + [b"Q " + t.decode().upper().encode() for t in twins]
    vocab = F.oracle_vocab(texts)
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    g = ShardIndex(vocab_capacity_log2=16)
    g.add_documents(texts)
    g.commit()
    assert g.stats()["hash_rebuilds"] >= 1
    long_terms = F.ASCII_SPECIALS[2:] + F.UNI_SPECIALS + [F.LONG255] + twins
    terms = []
    for s in long_terms:
        terms += [s, s[1:], s.decode()[:-1].encode(), s.decode()[:3].encode() + b"q" + s.decode()[3:].encode()]
    for e in (0, 1, 2):
        got = g.fuzzy_terms_batch(terms, e, 0, 5)
        for t, gt in zip(terms, got):
            assert gt == F.expected(vocab, t, e, 0, 5), (t[:40], e)
    both = g.fuzzy_terms(twins[0], 1, 0, 5)[0]                              # the colliding pair, told apart
    assert [(t, d) for t, _, d in both] == [(twins[0], 0), (F.ASCII_SPECIALS[2], 1), (F.ASCII_SPECIALS[3], 1)]
    g.close()


# 7. lifecycle: delete, compact, a reader opened before
def test_delete_compact_and_an_older_reader():
    texts = F.dense_texts()
    keys = [b"d%05d" % i for i in range(len(texts))]
    g = ShardIndex(vocab_capacity_log2=16)
    g.add_documents(texts, keys)
    g.commit()
    cafe, cafe_acc = F.CAFES[1], F.CAFES[0]
    probes = [cafe, cafe_acc, b"a"] + F.ASCII_SPECIALS[2:] + F.UNI_SPECIALS + [F.LONG255, F.LONG255[1:]]
    before = {t: want(t, 1, 0, 1024) for t in probes}
    old = g.reader()
    assert {t: old.fuzzy_terms(t, 1, 0, 1024) for t in probes} == before
    # the only documents holding "cafe", and the first document of the corpus (so every later byte moves)
    gone = [i for i, t in enumerate(texts) if t in (cafe, b"X CAFE .")] + [0]
    assert len(gone) == 3
    assert g.delete_documents([keys[i] for i in gone]) == 3
    g.commit()
    left = [t for i, t in enumerate(texts) if i not in gone]
    vocab = F.oracle_vocab(left)
    assert cafe not in vocab and b"a" not in vocab and F.dense_vocab()[b"a"] == 1      # document 0 was the only "a"
    after = {t: F.expected(vocab, t, 1, 0, 1024) for t in probes}
    assert {t: g.fuzzy_terms(t, 1, 0, 1024) for t in probes} == after
    assert after[cafe][1] == before[cafe][1] - 1 and after[cafe_acc][1] == before[cafe_acc][1] - 1
    assert cafe not in [t for t, _, _ in after[cafe_acc][0]] and cafe in [t for t, _, _ in before[cafe_acc][0]]
    assert g.compact()["bytes_reclaimed"] > 0
    g.commit()
    assert {t: g.fuzzy_terms(t, 1, 0, 1024) for t in probes} == after      # the long terms byte for byte
    assert {t: old.fuzzy_terms(t, 1, 0, 1024) for t in probes} == before   # the older reader: the old vocabulary
    old.close()
    g.close()


# threading: lookups on several threads beside add_docs and commit
def test_lookups_beside_add_docs_and_commit():
    texts = F.dense_texts()
    added = [b"abcabq", b"abcabr abcabq", b"abcqbq"]
    vocabs = [F.oracle_vocab(texts + added[:i]) for i in range(len(added) + 1)]
    probes = [b"abcabq", b"a", F.LONG255[1:], F.UNI_SPECIALS[1]]
    states = [[F.expected(v, t, 1, 0, 5) for t in probes] for v in vocabs]
    assert len({repr(s) for s in states}) == len(states)                    # every commit changes an answer
    g = ShardIndex(vocab_capacity_log2=16)
    g.add_documents(texts)
    g.commit()
    rd = g.reader()
    errs, stop = [], threading.Event()

    def look():
        try:
            while not stop.is_set():
                assert rd.fuzzy_terms_batch(probes, 1, 0, 5) == states[0]   # the reader: its own snapshot
                assert g.fuzzy_terms_batch(probes, 1, 0, 5) in states       # the index: one whole snapshot
                assert g.fuzzy_terms(probes[0], 1, 0, 5) in [s[0] for s in states]
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
    assert g.fuzzy_terms_batch(probes, 1, 0, 5) == states[-1] and rd.fuzzy_terms_batch(probes, 1, 0, 5) == states[0]
    rd.close()
    g.close()


# 8. GLOBAL statistics do not change the returned df
def test_df_stays_local_under_global_statistics():
    g = ShardIndex(vocab_capacity_log2=16, stats_mode=L.STATS_GLOBAL)
    g.add_documents(F.dense_texts())
    g.commit()
    keys, dl, _ = g.vocab_export()
    st = g.stats()
    g.set_global_stats(keys, dl.astype(np.uint64) * 3, st["doc_count"] * 3, st["sum_ttf"] * 3)
    local, effective = g.df(b"a")
    assert effective == 3 * local == 3 * F.dense_vocab()[b"a"]
    for t in (b"a", b"abca", F.CAFES[0], F.LONG255):
        assert g.fuzzy_terms(t, 2, 0, 1024) == want(t, 2, 0, 1024)
    g.close()


# 9. Worker.search_did_you_mean
def test_worker_did_you_mean(lucene_fixture):
    w = Worker()
    texts = [d["text"].encode() for d in lucene_fixture["docs"]]
    w.index.add_documents(texts, [d["name"].encode() for d in lucene_fixture["docs"]])
    w.commit()
    vocab = F.oracle_vocab(texts)
    fixed = [F.expected(vocab, t, 2, 0, 1)[0][0][0].decode() for t in (b"wirless", b"earbusd")]
    assert fixed == ["wireless", "earbuds"]
    corrected, hits = w.search_did_you_mean("wirless earbusd")
    assert corrected == " ".join(fixed)
    assert hits == w.search_index(corrected) and len(hits) >= 3
    assert w.search_index("wirless earbusd") == []
    assert w.search_did_you_mean("wireless earbuds") == (None, w.search_index("wireless earbuds"))
    corrected, hits = w.search_did_you_mean("Wirless AND earbuds")          # operators stay where they are
    assert corrected == "wireless AND earbuds" and hits == w.search_index("wireless AND earbuds")
    assert w.search_did_you_mean("zzzzqqqqzzzz") == (None, [])              # nothing near: the query as it is
    w.close()
