"""Fuzzy search on the device (tfidf_fuzzy_expand*, tfidf_search_fuzzy*, the
reader forms, Worker.search_fuzzy) against fuzzy_search_ref.py, compared
exactly: the same expansions (terms, order, boost bits, df, dist, n_within) and
the same hits, order and float32 score bits.  The corpus is
fuzzy_ref.dense_texts() plus the four families of fuzzy_search_ref.py: two
times 81 hashed terms within 2 edits of one another (ASCII and non-ASCII, some
only spelt in upper case), a pair whose UTF-8 and UTF-16 orders differ, and a
frequent word with three rare misspellings."""
import ctypes as C
import functools

import numpy as np
import pytest

import fuzzy_ref as F
import fuzzy_search_ref as R
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex, _key_arrays
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

TERMS = R.terms()
EDITS, PREFIXES, EXPANSIONS = (0, 1, 2), (0, 1, 3), (1, 5, 50, 64)
INVERSIONS = [L.INVERSION_BLOCK, L.INVERSION_TERM]


@functools.lru_cache(maxsize=None)
def _cands(term, e, p):
    return R.candidates(R.fixture().vocab, term, e, p)


def want_expand(term, e, p, k):
    c = _cands(term, e, p)
    return [(t, df, d, float(b)) for t, df, d, b in c[:k]], len(c)


def want_hits(term, e, p, k):
    return R.bits(R.hits(R.clause_scores(R.fixture(), _cands(term, e, p)[:k])))


_state = {}


def index(inversion=L.INVERSION_BLOCK):
    """The committed fixture index per inversion, shared by the tests (never changed)."""
    if inversion not in _state:
        g = ShardIndex(vocab_capacity_log2=16, inversion=inversion)
        texts = R.texts()
        g.add_documents(texts, [b"d%05d" % i for i in range(len(texts))])
        g.commit()
        assert g.stats()["term_major"] == (1 if inversion == L.INVERSION_TERM else 0)
        _state[inversion] = g
    return _state[inversion]


def test_the_fixture_reaches_its_cases():
    """Checked against the reference alone."""
    big = only_hashed = ends_at_e = fewer = 0
    fam = set(R.FAMILY_A)
    for t in TERMS:
        c = _cands(t, 2, 0)
        for k in EXPANSIONS:
            s = R.straddle(c, k)
            fewer += 0 < len(c) < k
            if s is None:
                continue
            big += s[1] - s[0] > 64 and s[1] > k
            only_hashed += s[1] > k and all(x[0] in fam for x in c[s[0]:s[1]])
            ends_at_e += s[1] == k
    assert big and only_hashed and ends_at_e and fewer
    # m > ed drops candidates, and a one-letter term at 2 edits keeps itself alone
    assert want_expand(b"a", 2, 0, 50) == ([(b"a", 1, 0, 1.0)], 1)
    assert len(F.expected(R.fixture().vocab, b"a", 2, 0, 1 << 30)[0]) > 30
    assert any(len(_cands(t, 2, 0)) < F.expected(R.fixture().vocab, t, 2, 0, 1)[1] for t in TERMS if len(t) > 1)
    # pair (c) at equal boost, in byte order: the reverse of their UTF-16 order
    b = float(np.float32(1) - np.float32(1) / np.float32(5))
    assert [(t, x) for t, _, _, x in want_expand(b"qqxqq", 1, 0, 50)[0]] == [(R.PAIR_C[1], b), (R.PAIR_C[0], b)]
    assert want_expand(b"", 2, 0, 5) == want_expand(b"\xff\xfe", 2, 0, 5) == want_expand(b"l" * 256, 2, 0, 5) == ([], 0)


# 1. the expansions: every parameter, both inversions
@pytest.mark.parametrize("inversion", INVERSIONS)
@pytest.mark.parametrize("max_edits", EDITS)
def test_expansions_equal_the_reference(inversion, max_edits):
    g = index(inversion)
    for p in PREFIXES:
        for k in EXPANSIONS:
            got = g.fuzzy_expand_batch(TERMS, max_edits, p, k)
            assert len(got) == len(TERMS)
            for t, gt in zip(TERMS, got):
                assert gt == want_expand(t, max_edits, p, k), (t[:40], max_edits, p, k)
    assert g.last_fuzzy_chunks()[0] >= 2                    # the batch does not fit one staging of the scan


# 2. the hits
@pytest.mark.parametrize("inversion", INVERSIONS)
@pytest.mark.parametrize("params", [(2, 0, 50), (1, 0, 64), (2, 1, 5), (0, 3, 1), (2, 3, 64)])
def test_hits_equal_the_reference(inversion, params):
    e, p, k = params
    g = index(inversion)
    docs, scores, offs, n_exp, _ = g.search_fuzzy_batch_arrays(TERMS, e, p, k)
    o = offs.tolist()
    some = 0
    for i, t in enumerate(TERMS):
        exp = _cands(t, e, p)[:k]
        assert n_exp[i] == len(exp), t[:40]
        per_doc = R.clause_scores(R.fixture(), exp)
        assert R.sums_are_order_independent(per_doc), t[:40]    # so the scorer's clause order cannot be what differs
        got = list(zip(docs[o[i]:o[i + 1]].tolist(), scores[o[i]:o[i + 1]].view(np.int32).tolist()))
        assert got == R.bits(R.hits(per_doc)), (t[:40], params)
        some += bool(got)
    assert some > 20


def test_misspellings_score_with_the_frequent_words_idf():
    g = index()
    fx = R.fixture()
    got = g.search_fuzzy_arrays(R.WORD_D, 2, 0, 50)
    exp = _cands(R.WORD_D, 2, 0)[:50]
    assert {t for t, _, _, _ in exp} == {R.WORD_D, *R.MISSPELT_D} and got[2] == 4
    assert max(df for _, df, _, _ in exp) == R.DF_D and sorted(df for _, df, _, _ in exp) == [1, 1, 1, R.DF_D]
    by_doc = dict(zip(got[0].tolist(), got[1].view(np.int32).tolist()))
    want = dict(want_hits(R.WORD_D, 2, 0, 50))
    assert by_doc == want and len(want) == R.DF_D + 3
    for m in R.MISSPELT_D:
        (doc, _), = fx.postings[m]
        d, s = g.search_all_arrays(m)
        assert d.tolist() == [doc]
        assert by_doc[doc] == want[doc] and by_doc[doc] != int(s.view(np.int32)[0])   # not the rare term's own idf
        assert np.int32(by_doc[doc]).view(np.float32) < s[0]                         # blended: the frequent word's idf, boosted down
    # the word itself outranks its misspellings
    top = got[0][:R.DF_D].tolist()
    assert all(fx.rows[d].get(R.WORD_D) for d in top)


@pytest.mark.parametrize("inversion", INVERSIONS)
def test_an_expansion_of_the_term_alone_is_the_plain_search(inversion):
    g = index(inversion)
    for t in [b"abc", R.WORD_D, R.FAMILY_A[4], R.FAMILY_B[3], F.EMOJI, F.LONG255, R.PAIR_C[0], b"x"]:
        assert [c[0] for c in want_expand(t, 0, 0, 50)[0]] == [t]
        d, s, n = g.search_fuzzy_arrays(t, 0, 0, 50)
        wd, ws = g.search_all_arrays(t)
        assert n == 1 and len(wd) >= 1
        assert d.tolist() == wd.tolist() and s.view(np.int32).tolist() == ws.view(np.int32).tolist(), t[:40]


# 3. the single calls and the reader forms are the batch of one
@pytest.mark.parametrize("inversion", INVERSIONS)
def test_single_calls_and_readers_equal_the_batch_of_one(inversion):
    g = index(inversion)
    some = [b"a", b"ABCA", R.FAMILY_A[0], R.FAMILY_B[0].decode().upper().encode(), b"qqxqq", R.MISSPELT_D[1], F.EMOJI,
            b"", b"\xff\xfe", b"zzzzzzzzzzzz"]
    with g.reader() as rd:
        for t in some:
            for e, p, k in ((2, 0, 50), (1, 1, 64), (2, 3, 1)):
                w = want_expand(t, e, p, k)
                assert g.fuzzy_expand(t, e, p, k) == w, (t[:40], e, p, k)
                assert rd.fuzzy_expand(t, e, p, k) == w
                assert g.fuzzy_expand_batch([t], e, p, k) == [w] == rd.fuzzy_expand_batch([t], e, p, k)
                h = want_hits(t, e, p, k)
                for d, s, n in (g.search_fuzzy_arrays(t, e, p, k), rd.search_fuzzy_arrays(t, e, p, k)):
                    assert list(zip(d.tolist(), s.view(np.int32).tolist())) == h and n == len(w[0])
                assert R.bits(g.search_fuzzy(t, e, p, k)) == h == R.bits(rd.search_fuzzy(t, e, p, k))
                assert [R.bits(x) for x in g.search_fuzzy_batch([t], e, p, k)] == [h]
                assert [R.bits(x) for x in rd.search_fuzzy_batch([t], e, p, k)] == [h]
    assert g.fuzzy_expand_batch([]) == [] == g.search_fuzzy_batch([])      # n_terms = 0 is legal


def test_a_reader_opened_before_a_commit_sees_its_own_expansion():
    docs = [R.WORD_D + b" zzpad"] * 3 + [R.MISSPELT_D[1] + b" zzpad"]
    g = ShardIndex(vocab_capacity_log2=12)
    g.add_documents(docs)
    g.commit()
    old = g.reader()
    before = R.Shard(docs)
    g.add_documents([R.MISSPELT_D[0] + b" zzpad", R.FAMILY_A[7] + b" " + R.WORD_D])
    g.commit()
    after = R.Shard(docs + [R.MISSPELT_D[0] + b" zzpad", R.FAMILY_A[7] + b" " + R.WORD_D])
    for t in (R.WORD_D, R.MISSPELT_D[2], R.FAMILY_A[8]):
        for sh, who in ((before, old), (after, g)):
            exp, n = R.expansion(sh.vocab, t, 2, 0, 50)
            assert who.fuzzy_expand(t, 2, 0, 50) == ([(a, b, c, float(d)) for a, b, c, d in exp], n)
            assert R.bits(who.search_fuzzy(t, 2, 0, 50)) == R.bits(R.hits(R.clause_scores(sh, exp)))
    assert len(old.fuzzy_expand(R.WORD_D)[0]) == 2 and len(g.fuzzy_expand(R.WORD_D)[0]) == 3
    old.close()
    g.close()


# 4. candidate budgets: any split gives the same output
@pytest.mark.parametrize("budget", ["1", "7", "100"])
def test_any_candidate_budget_gives_the_same_output(budget, monkeypatch):
    g = index()
    with g.reader() as rd:
        whole = rd.fuzzy_expand_batch_arrays(TERMS, 2, 0, 50)
        hits = rd.search_fuzzy_batch_arrays(TERMS, 2, 0, 50)
        scans, fills = g.last_fuzzy_chunks()
        assert fills == scans and scans >= 2                # everything fitted: one candidate chunk per scan
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        monkeypatch.setenv("TFIDF_FUZZY_CAND_BUDGET", budget)
        split = rd.fuzzy_expand_batch_arrays(TERMS, 2, 0, 50)
        s2, f2 = g.last_fuzzy_chunks()
        assert s2 == scans and f2 > fills
        hits2 = rd.search_fuzzy_batch_arrays(TERMS, 2, 0, 50)
        assert g.last_fuzzy_chunks() == (s2, f2)
        for a, b in zip(split[:7] + hits2[:4], whole[:7] + hits[:4]):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


# 5. buffer protocol and argument errors
def _raw_expand(g, terms, e, p, k, cand_cap, terms_cap, payload=True):
    blob, t_offs = _key_arrays(terms)
    n = len(terms)
    c_offs = np.full(n + 1, 77, np.uint64)
    within = np.full(max(n, 1), 77, np.uint64)
    nc, nb = C.c_uint64(77), C.c_uint64(77)
    t_out = np.zeros(cand_cap + 1, np.uint64)
    text = np.zeros(max(terms_cap, 1), np.uint8)
    df = np.zeros(max(cand_cap, 1), np.uint32)
    dist = np.zeros(max(cand_cap, 1), np.uint8)
    boosts = np.zeros(max(cand_cap, 1), np.float32)
    rc = L.load().tfidf_fuzzy_expand_batch(
        g._h, blob, L.ptr(t_offs, C.c_uint64), n, e, p, k, L.ptr(c_offs, C.c_uint64), L.ptr(within, C.c_uint64),
        L.ptr(t_out, C.c_uint64) if payload else None, text.ctypes.data_as(C.c_void_p) if payload else None, terms_cap,
        L.ptr(df, C.c_uint32) if payload else None, L.ptr(dist, C.c_uint8) if payload else None,
        L.ptr(boosts, C.c_float) if payload else None, cand_cap, C.byref(nc), C.byref(nb), None)
    return rc, c_offs.tolist(), within[:n].tolist(), nc.value, nb.value


def _raw_search(g, terms, e, p, k, cap, payload=True):
    blob, t_offs = _key_arrays(terms)
    n = len(terms)
    offs = np.full(n + 1, 77, np.uint64)
    n_exp = np.full(max(n, 1), 77, np.uint32)
    docs = np.zeros(max(cap, 1), np.uint32)
    scores = np.zeros(max(cap, 1), np.float32)
    total = C.c_uint64(77)
    rc = L.load().tfidf_search_fuzzy_batch(
        g._h, blob, L.ptr(t_offs, C.c_uint64), n, e, p, k, L.ptr(docs, C.c_uint32) if payload else None,
        L.ptr(scores, C.c_float) if payload else None, cap, L.ptr(offs, C.c_uint64), L.ptr(n_exp, C.c_uint32),
        C.byref(total), None)
    return rc, offs.tolist(), n_exp[:n].tolist(), total.value


def test_buffer_protocol_and_argument_errors():
    g = index()
    terms = [b"abc", R.WORD_D, b"", R.FAMILY_A[0], b"zzzzzzzzzzzz"]
    full = [want_expand(t, 2, 0, 5) for t in terms]
    n_c = sum(len(c) for c, _ in full)
    n_b = sum(len(t) for c, _ in full for t, _, _, _ in c)
    offs = [0]
    for c, _ in full:
        offs.append(offs[-1] + len(c))
    within = [w for _, w in full]
    assert n_c == 14 and within[0] > 64
    # the size query: caps 0, NULL payload pointers
    assert _raw_expand(g, terms, 2, 0, 5, 0, 0, payload=False) == (L.E_BUFFER, offs, within, n_c, n_b)
    # one candidate slot short, one term byte short: offsets, n_within and totals still in full
    assert _raw_expand(g, terms, 2, 0, 5, n_c - 1, n_b) == (L.E_BUFFER, offs, within, n_c, n_b)
    assert _raw_expand(g, terms, 2, 0, 5, n_c, n_b - 1) == (L.E_BUFFER, offs, within, n_c, n_b)
    assert _raw_expand(g, terms, 2, 0, 5, n_c, n_b) == (L.OK, offs, within, n_c, n_b)
    assert _raw_expand(g, [b"zzzzzzzzzzzz", b""], 2, 0, 5, 0, 0, payload=False) == (L.OK, [0, 0, 0], [0, 0], 0, 0)
    assert _raw_expand(g, [], 2, 0, 5, 0, 0, payload=False)[0] == L.OK
    # the hits: the same protocol
    hits = [want_hits(t, 2, 0, 5) for t in terms]
    h_offs = [0]
    for h in hits:
        h_offs.append(h_offs[-1] + len(h))
    n_exp = [len(c) for c, _ in full]
    assert h_offs[-1] > 10
    assert _raw_search(g, terms, 2, 0, 5, 0, payload=False) == (L.E_BUFFER, h_offs, n_exp, h_offs[-1])
    assert _raw_search(g, terms, 2, 0, 5, h_offs[-1] - 1) == (L.E_BUFFER, h_offs, n_exp, h_offs[-1])
    assert _raw_search(g, terms, 2, 0, 5, h_offs[-1]) == (L.OK, h_offs, n_exp, h_offs[-1])
    assert _raw_search(g, [], 2, 0, 5, 0, payload=False)[0] == L.OK
    # argument errors: nothing written
    untouched = [77] * (len(terms) + 1)
    for e, k in ((3, 5), (2, 0), (2, 65)):
        rc, o, w, a, b = _raw_expand(g, terms, e, 0, k, n_c, n_b)
        assert rc == L.E_INVALID_ARG and o == untouched and w == [77] * len(terms) and (a, b) == (77, 77)
        rc, o, x, tot = _raw_search(g, terms, e, 0, k, 100)
        assert rc == L.E_INVALID_ARG and o == untouched and x == [77] * len(terms) and tot == 77
    assert _raw_expand(g, [b"a"] * 65537, 2, 0, 1, 0, 0, payload=False)[0] == L.E_INVALID_ARG
    with pytest.raises(L.TfidfError) as ei:
        g.search_fuzzy(b"a", 2, 0, 65)
    assert ei.value.code == L.E_INVALID_ARG
    # before the first commit
    fresh = ShardIndex(vocab_capacity_log2=12)
    fresh.add_documents([b"abc"])
    for call in (lambda: fresh.fuzzy_expand_batch([b"abc"]), lambda: fresh.fuzzy_expand(b"abc"),
                 lambda: fresh.search_fuzzy_batch([b"abc"]), lambda: fresh.search_fuzzy(b"abc")):
        with pytest.raises(L.TfidfError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    fresh.close()


# 6. Worker.search_fuzzy
def test_worker_search_fuzzy(tmp_path):
    docs = tmp_path / "docs"
    docs.mkdir()
    (docs / "a.txt").write_text("wireless earbuds for the gym")
    (docs / "b.txt").write_text("a kangaroo in the garden")
    (docs / "c.txt").write_text("wired headphones")
    w = Worker(str(docs), str(tmp_path / "ix"))
    w.init()
    assert w.search_index("wirless") == []
    hits = w.search_fuzzy("Wirless")
    assert [h["document"]["name"] for h in hits] == ["a.txt"] and hits[0]["score"] > 0
    assert [h["document"]["name"] for h in w.search_fuzzy("kangaru")] == ["b.txt"]
    assert w.search_fuzzy("zzzzqqqqzzzz") == []
    assert w.search_fuzzy("wirless", max_edits=0) == []
    for bad in ("wirless earbuds", "", " . "):
        with pytest.raises(ValueError):
            w.search_fuzzy(bad)
    w.close()
