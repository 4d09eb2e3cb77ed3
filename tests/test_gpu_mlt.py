"""More-like-this on the device (tfidf_mlt_terms_batch, tfidf_more_like_this_batch,
their single, reader and Worker forms) against mlt_ref.py, compared exactly:
terms, order, tf, df and float32 score bits of the interesting terms; ids, order
and float32 score bits of the hits.  One committed index per inversion holds the
corpora of mlt_ref side by side; every expected value comes from mlt_ref (the
oracle) alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import mlt_ref as M
from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import engine as E
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

_state = {}
INVERSIONS = [L.INVERSION_BLOCK, L.INVERSION_TERM]
KEYS = [b"d/%05d" % i for i in range(len(M.TEXTS))]
LOOSE = dict(min_tf=1, min_df=1)


def index(inv=L.INVERSION_BLOCK):
    """The committed index over all corpora, shared by the tests (never changed)."""
    if ("g", inv) not in _state:
        g = ShardIndex(inversion=inv)
        g.add_documents(list(M.TEXTS), KEYS)
        g.commit()
        assert g.stats()["term_major"] == (inv == L.INVERSION_TERM)
        _state["g", inv] = g
    return _state["g", inv]


def ref():
    if "ref" not in _state:
        _state["ref"] = M.MltRef(M.TEXTS)
    return _state["ref"]


@functools.lru_cache(maxsize=None)
def want_terms(d, items):
    sel, n = ref().terms(d, **{**M.DEFAULTS, **dict(items)})
    return M.exact_terms(sel), n


def check_terms(got, seeds, params):
    assert len(got) == len(seeds)
    for (lst, n_cand), d in zip(got, seeds):
        assert (M.exact_terms(lst), n_cand) == want_terms(d, tuple(sorted(params.items()))), d


def check_hits(got, seeds, k, exclude, params, r=None):
    r = r or ref()
    assert len(got) == len(seeds)
    for h, d in zip(got, seeds):
        assert M.exact_hits(h) == M.exact_hits(r.more_like_this(d, k, exclude, **params)), d


def all_seeds():
    return list(range(len(M.TEXTS)))


# 1. every document as a seed, default and loose parameters, both inversions
@pytest.mark.parametrize("inv", INVERSIONS)
@pytest.mark.parametrize("params", [{}, LOOSE], ids=["defaults", "min1"])
def test_every_seed_terms_and_hits_are_the_reference(inv, params):
    g = index(inv)
    seeds = [d for d in all_seeds() if d != M.doc("big") or not params]   # the big row under min1: test 3
    got = g.mlt_terms_batch(seeds, **params)
    check_terms(got, seeds, params)
    check_hits(g.more_like_this_batch(seeds, 10, True, **params), seeds, 10, True, params)
    n_entries, chunks = g.last_mlt_stats()
    assert n_entries == sum(len(ref().rows[d]) for d in seeds) and chunks == 1
    if not params:
        sk = [len(got[seeds.index(M.doc("skewed", i))][0]) for i in range(len(M.SKEWED))]
        assert sum(1 for n in sk if n) >= len(sk) // 2, "the defaults select something on the skewed corpus"
    # a tf the CSR field cannot hold, and one it can
    esc = dict((t, tf) for t, tf, _, _ in got[seeds.index(M.doc("esc", 0))][0])
    assert esc[b"zzescape"] == 65535
    assert dict((t, tf) for t, tf, _, _ in got[seeds.index(M.doc("esc", 1))][0])[b"zzsixhundred"] == 600
    for name in ("empty_front", "empty_mid"):
        for i in (0, 1):
            assert got[seeds.index(M.doc(name, i))] == ([], 0)


def test_hits_equal_the_oracle_search_of_the_joined_terms():
    g = index()
    r = ref()
    plain = 0
    for d in all_seeds():
        sel, _ = r.terms(d, **M.DEFAULTS)
        terms = [t for t, _, _, _ in sel]
        if not terms:
            continue
        try:                                              # the joined terms parse back to the same clauses
            if [t for t, _ in O.query_terms(b" ".join(terms))] != terms:
                continue
        except ValueError:
            continue
        plain += 1
        want = [h for h in r.o.search(b" ".join(terms), 0)][:10]
        assert M.exact_hits(g.more_like_this(d, 10, False)) == M.exact_hits(want), d
        assert M.exact_hits(r.more_like_this(d, 10, False)) == M.exact_hits(want), d
    assert plain >= 10


# 2. a boundary tie group larger than max_terms, hashed keys among it
@pytest.mark.parametrize("inv", INVERSIONS)
@pytest.mark.parametrize("max_terms", [25, 45])
def test_tie_group_across_the_cut_is_broken_by_bytes(inv, max_terms):
    g = index(inv)
    d = M.doc("tie")
    params = dict(min_tf=2, min_df=1, max_terms=max_terms)
    got = g.mlt_terms_batch([d], **params)
    check_terms(got, [d], params)
    lst, n_cand = got[0]
    assert n_cand == 51 and len(lst) == max_terms and [t for t, _, _, _ in lst[:3]] == M.TIE_TOP
    tied = lst[3:]
    assert len({(tf, df, M.bits(s)) for _, tf, df, s in tied}) == 1 and len(tied) < 48
    names = [t for t, _, _, _ in tied]
    assert names == sorted(M.TIE_SHORT + M.TIE_ASCII + M.TIE_UNI)[:max_terms - 3]
    assert any(len(t) > 16 for t in names) and (max_terms == 25 or any(t[0] >= 0x80 and len(t) > 14 for t in names))
    check_hits(g.more_like_this_batch([d], 5, False, **params), [d], 5, False, params)


# 3. a row of more than 4 096 distinct terms, max_terms at its limit; terms from more than one dictionary range
def _home_range(term, cap_log2=18, range_bits=16):
    lo, hi = E.term_key(term)
    x = (lo ^ (((lo >> 32) << 16 | (lo >> 48)) & 0xFFFFFFFF) ^ hi ^ (((hi >> 32) << 8 | (hi >> 56)) & 0xFFFFFFFF)) & 0xFFFFFFFF
    home = ((x * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - cap_log2)
    return home >> range_bits, home & ((1 << range_bits) - 1)


@pytest.mark.parametrize("inv", INVERSIONS)
def test_big_row_with_1024_terms(inv):
    g = index(inv)
    d = M.doc("big")
    params = dict(min_tf=1, min_df=1, max_terms=1024)
    got = g.mlt_terms_batch([d], **params)
    check_terms(got, [d], params)
    assert got[0][1] == 4200 and len(got[0][0]) == 1024
    check_hits(g.more_like_this_batch([d], 3, False, **params), [d], 3, False, params)
    if inv == L.INVERSION_BLOCK:
        # the selected terms' home slots (dict_hash / dict_home of tfidf_common.h) lie in several of the four 2^16-slot
        # ranges of a 2^18-slot dictionary; linear probing moves a term a few slots at this load, so homes within 256
        # slots of a range's end are not counted
        ranges = {r for r, at in (_home_range(t) for t, _, _, _ in got[0][0]) if at < (1 << 16) - 256}
        assert len(ranges) >= 2, ranges
    with pytest.raises(L.TfidfError) as e:
        g.mlt_terms_batch([d], max_terms=1025)
    assert e.value.code == L.E_INVALID_ARG
    with pytest.raises(L.TfidfError) as e:
        g.more_like_this(d, 10, max_terms=0)
    assert e.value.code == L.E_INVALID_ARG


# 4. after delete + commit (live_map not the identity) and again after compact
def test_after_delete_and_after_compact():
    g = ShardIndex()
    g.add_documents(list(M.TEXTS), KEYS)
    g.commit()
    dead = {M.doc("skewed", i) for i in range(0, 60, 3)} | {M.doc("empty_front", 0), M.doc("esc", 2)}
    assert g.delete_documents([KEYS[d] for d in sorted(dead)]) == len(dead)
    g.commit()
    live = [d for d in range(len(M.TEXTS)) if d not in dead]
    r = M.MltRef([M.TEXTS[d] for d in live])
    seeds = list(range(len(live)))
    try:
        for step in ("deleted", "compacted"):
            assert g.stats()["num_docs"] == len(live)
            got = g.mlt_terms_batch(seeds)
            for (lst, n), d in zip(got, seeds):
                sel, nc = r.terms(d, **M.DEFAULTS)
                assert (M.exact_terms(lst), n) == (M.exact_terms(sel), nc), (step, d)
            check_hits(g.more_like_this_batch(seeds, 7), seeds, 7, True, {}, r)
            if step == "deleted":
                g.compact()
                g.commit()
    finally:
        r.close()
        g.close()


# 5. GLOBAL statistics: the selection is the shard's own, the scores follow the global numbers
def test_global_statistics_change_the_scores_not_the_selection():
    g = ShardIndex()
    g.add_documents(list(M.SKEWED))
    g.commit()
    r = M.MltRef(M.SKEWED)
    try:
        seeds = list(range(len(M.SKEWED)))
        before_terms = g.mlt_terms_batch(seeds)
        before_hits = g.more_like_this_batch(seeds, 10)
        keys, dl, _ = g.vocab_export()
        st = g.stats()
        g.set_global_stats(keys, dl.astype(np.uint64) * 3 + 1, st["doc_count"] * 4, st["sum_ttf"] * 5)
        r.set_global_stats(st["doc_count"] * 4, st["sum_ttf"] * 5, {t: 3 * len(p) + 1 for t, p in r.post.items()})
        assert g.mlt_terms_batch(seeds) == before_terms
        for (lst, n), d in zip(before_terms, seeds):
            sel, nc = r.terms(d, **M.DEFAULTS)
            assert (M.exact_terms(lst), n) == (M.exact_terms(sel), nc)
        after = g.more_like_this_batch(seeds, 10)
        check_hits(after, seeds, 10, True, {}, r)
        assert [M.exact_hits(h) for h in after] != [M.exact_hits(h) for h in before_hits]
    finally:
        r.close()
        g.close()


# 6. non-default k1 / b
def test_other_k1_and_b():
    g = ShardIndex(k1=0.9, b=0.4)
    g.add_documents(list(M.SKEWED))
    g.commit()
    r = M.MltRef(M.SKEWED, k1=0.9, b=0.4)
    try:
        seeds = list(range(len(M.SKEWED)))
        check_hits(g.more_like_this_batch(seeds, 10), seeds, 10, True, {}, r)
        check_hits(g.more_like_this_batch(seeds, 10, **LOOSE), seeds, 10, True, LOOSE, r)
    finally:
        r.close()
        g.close()


# 7. exclusion, k = 1, k = 1024
def test_exclusion_and_the_limits_of_k():
    g = index()
    seeds = [M.doc("skewed", i) for i in range(0, 60, 7)] + [M.doc("esc", 3)]
    for k, excl in ((1, True), (1, False), (10, False), (1023, True), (1024, False)):
        got = g.more_like_this_batch(seeds, k, excl, **LOOSE)
        check_hits(got, seeds, k, excl, LOOSE)
        if excl:
            assert all(d not in [x for x, _ in h] for h, d in zip(got, seeds))
    on = g.more_like_this_batch(seeds, 10, False, **LOOSE)
    assert sum(1 for h, d in zip(on, seeds) if d in [x for x, _ in h]) >= len(seeds) // 2   # the fixture has seeds to drop
    for k, excl in ((0, False), (1025, False), (1024, True)):
        with pytest.raises(L.TfidfError) as e:
            g.more_like_this_batch(seeds, k, excl)
        assert e.value.code == L.E_INVALID_ARG


# 8. seeds: repeated, unordered, empty and malformed ones anywhere, none, out of range
def test_seed_lists():
    g = index()
    e0, m0, m1, e1, e2 = (M.doc("empty_front", 0), M.doc("empty_front", 1), M.doc("empty_mid", 0), M.doc("empty_mid", 1),
                          M.doc("empty_end", 0))
    s = M.doc("skewed")
    seeds = [e0, m0, s + 40, s + 3, s + 40, e1, m1, M.doc("esc", 1), s + 3, s + 59, s, e2, m0]
    check_terms(g.mlt_terms_batch(seeds), seeds, {})
    got = g.more_like_this_batch(seeds, 10)
    check_hits(got, seeds, 10, True, {})
    assert [got[i] for i in (0, 1, 5, 6, 11, 12)] == [[]] * 6 and got[2] == got[4] and got[2]
    assert g.mlt_terms_batch([]) == [] and g.more_like_this_batch([], 10) == []
    assert g.last_mlt_stats() == (0, 0)
    # a seed >= num_docs: nothing written
    n = len(M.TEXTS)
    bad = np.array([s, n, s + 1], np.uint32)
    docs = np.full((3, 4), 0xABABABAB, np.uint32)
    scores = np.full((3, 4), -1.0, np.float32)
    cnt = np.full(3, 77, np.uint32)
    p = E.mlt_params()
    rc = L.load().tfidf_more_like_this_batch(g._h, L.ptr(bad, C.c_uint32), 3, C.byref(p), 4, 0, L.ptr(docs, C.c_uint32),
                                             L.ptr(scores, C.c_float), L.ptr(cnt, C.c_uint32))
    assert rc == L.E_INVALID_ARG
    assert (docs == 0xABABABAB).all() and (scores == -1.0).all() and (cnt == 77).all()
    offs = np.full(4, 99, np.uint64)
    cand = np.full(3, 99, np.uint64)
    nt, nb = C.c_uint64(5), C.c_uint64(5)
    rc = L.load().tfidf_mlt_terms_batch(g._h, L.ptr(bad, C.c_uint32), 3, C.byref(p), L.ptr(offs, C.c_uint64),
                                        L.ptr(cand, C.c_uint64), None, None, 0, None, None, None, 0, C.byref(nt),
                                        C.byref(nb))
    assert rc == L.E_INVALID_ARG and (offs == 99).all() and (cand == 99).all() and (nt.value, nb.value) == (5, 5)
    with pytest.raises(L.TfidfError) as e:
        g.more_like_this(n, 10)
    assert e.value.code == L.E_INVALID_ARG


def test_before_the_first_commit_is_a_state_error():
    g = ShardIndex()
    try:
        for call in (lambda: g.more_like_this_batch([0], 10), lambda: g.mlt_terms_batch([0]), lambda: g.more_like_this(0)):
            with pytest.raises(L.TfidfError) as e:
                call()
            assert e.value.code == L.E_STATE
    finally:
        g.close()


# 9. the buffer protocol of the terms call
def test_terms_buffer_protocol():
    g = index()
    seeds = [M.doc("skewed", 5), M.doc("empty_mid", 1), M.doc("esc", 0), M.doc("skewed", 9)]
    full = g.mlt_terms_batch_arrays(seeds)
    m, nb = len(full[4]), len(full[3])
    assert m > 3 and nb > m
    sd = np.array(seeds, np.uint32)
    p = E.mlt_params()
    lib = L.load()

    def call(t_cap, b_cap):
        offs = np.zeros(len(seeds) + 1, np.uint64)
        cand = np.zeros(len(seeds), np.uint64)
        b_offs = np.full(m + 2, 7, np.uint64)
        blob = np.full(nb + 2, 0xEE, np.uint8)
        tf, df = np.zeros(m + 1, np.uint32), np.zeros(m + 1, np.uint32)
        sc = np.zeros(m + 1, np.float32)
        nt, nbytes = C.c_uint64(), C.c_uint64()
        have = t_cap or b_cap
        rc = lib.tfidf_mlt_terms_batch(g._h, L.ptr(sd, C.c_uint32), len(seeds), C.byref(p), L.ptr(offs, C.c_uint64),
                                       L.ptr(cand, C.c_uint64), L.ptr(b_offs, C.c_uint64) if have else None,
                                       blob.ctypes.data_as(C.c_void_p) if have else None, b_cap,
                                       L.ptr(tf, C.c_uint32) if have else None, L.ptr(df, C.c_uint32) if have else None,
                                       L.ptr(sc, C.c_float) if have else None, t_cap, C.byref(nt), C.byref(nbytes))
        return rc, offs, cand, nt.value, nbytes.value, b_offs, blob

    for t_cap, b_cap in ((0, 0), (m - 1, nb), (m, nb - 1)):
        rc, offs, cand, nt, nbytes, b_offs, blob = call(t_cap, b_cap)
        assert rc == L.E_BUFFER and (nt, nbytes) == (m, nb)
        assert (offs == full[0]).all() and (cand == full[1]).all()
        assert (b_offs == 7).all() and (blob == 0xEE).all()          # no partial payload
    rc, offs, cand, nt, nbytes, b_offs, blob = call(m, nb)
    assert rc == L.OK and (b_offs[:m + 1] == full[2]).all() and blob[:nb].tobytes() == full[3]


# 10. candidate chunks
def equal_arrays(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, bytes):
            assert x == y
        else:
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("budget", [1, 40, 1500])
def test_candidate_chunks_give_the_unchunked_arrays(budget, monkeypatch):
    g = index()
    seeds = [M.doc("skewed", i) for i in range(12)] + [M.doc("empty_mid", 1), M.doc("tie"), M.doc("big"), M.doc("esc", 0),
                                                        M.doc("skewed", 2)]
    params = dict(min_tf=1, min_df=1, max_terms=30)
    if "chunk_whole" not in _state:
        _state["chunk_whole"] = (g.mlt_terms_batch_arrays(seeds, **params), g.last_mlt_stats(),
                                 g.more_like_this_batch_arrays(seeds, 5, **params))
    whole, stats, hits = _state["chunk_whole"]
    assert stats[1] == 1
    with g.reader() as rd:
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        monkeypatch.setenv("TFIDF_MLT_CAND_BUDGET", str(budget))
        equal_arrays(rd.mlt_terms_batch_arrays(seeds, **params), whole)
        entries, chunks = g.last_mlt_stats()
        assert entries == stats[0]
        counts = whole[1].tolist()
        assert chunks > 1 and (chunks == sum(1 for c in counts if c) if budget == 1 else chunks < len(seeds))
        equal_arrays(rd.more_like_this_batch_arrays(seeds, 5, **params), hits)


# 11. a reader keeps its snapshot
def test_reader_answers_from_its_snapshot():
    g = ShardIndex()
    g.add_documents(list(M.SKEWED[:30]))
    g.commit()
    r = M.MltRef(M.SKEWED[:30])
    try:
        seeds = list(range(30))
        with g.reader() as rd:
            g.add_documents(list(M.SKEWED[30:]))
            g.commit()
            got = rd.mlt_terms_batch(seeds, **LOOSE)
            for (lst, n), d in zip(got, seeds):
                sel, nc = r.terms(d, **{**M.DEFAULTS, **LOOSE})
                assert (M.exact_terms(lst), n) == (M.exact_terms(sel), nc), d
            check_hits(rd.more_like_this_batch(seeds, 10, **LOOSE), seeds, 10, True, LOOSE, r)
            with pytest.raises(L.TfidfError):
                rd.more_like_this(30)
        assert g.more_like_this(30) is not None and g.stats()["num_docs"] == 60
    finally:
        r.close()
        g.close()


# 12. the single forms are the batch of one
def test_single_forms_equal_the_batch_of_one():
    g = index()
    with g.reader() as rd:
        for d in (M.doc("skewed", 4), M.doc("empty_front", 1), M.doc("esc", 0), M.doc("tie")):
            for excl in (True, False):
                one = M.exact_hits(g.more_like_this(d, 6, excl))
                assert one == M.exact_hits(ref().more_like_this(d, 6, excl))
                assert one == M.exact_hits(rd.more_like_this(d, 6, excl)) == M.exact_hits(g.more_like_this_batch([d], 6, excl)[0])
            assert g.mlt_terms(d) == rd.mlt_terms(d) == g.mlt_terms_batch([d])[0]
    ms_scoring, ms_total = g.last_search_ms()
    assert ms_total >= ms_scoring >= 0.0


# 13. Worker.search_similar
def test_worker_search_similar():
    w = Worker()
    names = ["docs/%02d.txt" % i for i in range(len(M.SKEWED))]
    w.index.add_documents(list(M.SKEWED), [n.encode() for n in names])
    w.commit()
    r = M.MltRef(M.SKEWED)
    try:
        for d in (0, 17, 42):
            got = w.search_similar(names[d], 5)
            want = r.more_like_this(d, 5, True)
            assert want and [(x["document"]["name"], M.bits(x["score"])) for x in got] == \
                [(names[e], M.bits(s)) for e, s in want]
            assert set(got[0]) == set(w.search_index("wba")[0])
        assert w.search_similar("docs/none.txt") == []
    finally:
        r.close()
