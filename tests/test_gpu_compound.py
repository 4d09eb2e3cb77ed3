"""Compound queries on the device (tfidf_search_compound_batch and its reader
form) against compound_ref.py, on two corpora: the route corpus of routes_ref
(25 200 documents in 4 blocks, route documents at 8191 / 8192 and the other
block and commit edges: the smallest corpus where a (query, block) pair, an
empty block in the middle of a query and a run merge across blocks all occur)
and the Lucene fixture (one block: two runs per query, one always empty).
Float scores are compared by their bits.

  1  every kind with every occur and with every other kind, `*` as FILTER and
     as MUST_NOT, a clause with an empty row in each occur, SHOULD clauses
     that share documents, a 64-clause query; on ShardIndex and on a Reader
  2  the identities: a one-clause query is its route's row byte for byte; the
     operator words of tfidf_search_batch_all
  3  chunking: TFIDF_COMPOUND_CHUNK of a few entries gives the same bytes in
     many chunks, a query larger than the budget runs alone
  4  ties: all scores 2.0 and all scores 0.0 come out doc-ascending across the
     block edge
  5  protocol and errors
  6  lifecycle: a reader across a commit; deleted documents
  7  a term-major index, (k1, b) = (2.0, 1.0), a caller's stream
  8  Worker.search_query
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import compound_ref as CR
import routes_ref as RR
from routes_ref import BASE, BLOCK, FIRST_A
from tfidf_amd import _lib as L
from tfidf_amd import engine as E
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker

from test_gpu_incremental_commit import add, keyed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DOCS = keyed(BASE)
A0 = BASE[:FIRST_A]
OCCURS = (E.should, E.must, E.must_not, E.filter_)
ABSENT = b"qqabsentqq"                                   # in no document: an empty row in every kind

_refs = {}


def ref_of(texts, k1=1.2, b=0.75):
    key = (len(texts), hash(tuple(texts)), k1, b)
    if key not in _refs:
        _refs[key] = CR.CompoundRef(texts, k1, b)
    return _refs[key]


def pools():
    return [[E.text(q) for q in RR.QUERIES],
            [E.phrase(p, s) for p in RR.PHRASES for s in RR.SLOPS],
            [E.wildcard(p) for p in RR.WILDCARDS],
            [E.regex(p) for p in RR.REGEXES],
            [E.fuzzy(t, e, p, RR.EXPANSIONS) for t in RR.FUZZY for e, p in RR.FUZZY_PARAMS]]


def batch():
    """The queries of case 1."""
    ps = pools()
    at = [0] * 5

    def take(k):
        at[k] += 1
        return ps[k][(at[k] * 7 + at[k] // len(ps[k])) % len(ps[k])]

    qs = []
    for k in range(5):                                   # one clause: each kind in each occur
        for oc in OCCURS:
            qs.append([oc(take(k))])
    for ka in range(5):                                  # each kind with each other kind, in every pair of occurs
        for kb in range(5):
            if ka != kb:
                for oa in OCCURS:
                    for ob in OCCURS:
                        qs.append([oa(take(ka)), ob(take(kb))])
    star = E.wildcard(b"*")
    qs += [[E.filter_(star), E.should(E.text(RR.M1))], [E.filter_(star)], [E.must_not(star), E.should(E.text(RR.M1))],
           [E.must(E.text(RR.M2)), E.must_not(star)], [E.must(star), E.should(E.fuzzy(RR.FUZ[0], 2, 0, 50))]]
    for k, empty in enumerate([E.text(ABSENT), E.phrase(ABSENT + b" " + RR.M1, 1), E.wildcard(ABSENT + b"*"),
                               E.regex(ABSENT + b".+"), E.fuzzy(b"qqqqqqqqqqqqqqqq", 1, 0, 50)]):
        for oc in OCCURS:
            qs.append([E.should(E.text(RR.M1)), oc(empty), E.must(E.wildcard(b"mq*"))])
            qs.append([oc(empty)])
    # SHOULD clauses that share documents: the phrase documents hold all of them
    qs.append([E.should(E.text(RR.M1)), E.should(E.text(RR.M2)), E.should(E.wildcard(b"mq*")),
               E.should(E.phrase(RR.M1 + b" " + RR.M2, 0)), E.should(E.regex(b"mq(alpha|beta)")),
               E.should(E.fuzzy(RR.M1[:-1], 1, 0, 50))])
    qs.append([E.must(E.text(RR.M1)), E.should(E.text(RR.M2)), E.should(E.phrase(RR.M2 + b" " + RR.M1, 2)),
               E.should(E.text(RR.M3)), E.must_not(E.text(RR.MX)), E.filter_(E.wildcard(b"mq*"))])
    # 64 clauses: common words (every block), the route words, one veto
    qs.append([E.should(E.text(RR.c(i + 1))) for i in range(56)] + [E.should(E.text(RR.M1)), E.should(E.wildcard(b"zorbl*")),
              E.should(E.phrase(RR.P_GAP, 0)), E.should(E.fuzzy(RR.FUZ[0], 2, 0, 50)), E.should(E.regex(RR.REGEXES[0])),
              E.must_not(E.text(RR.c(3))), E.should(E.text(RR.PIV_A)), E.should(E.text(RR.LONG_TERM))])
    qs.append([])
    assert len(qs[-2]) == 64
    # "zarblat" lies in blocks 0 and 2 only: block 1 is an empty run between two runs with hits
    qs.append([E.must(E.text(RR.FUZ[4])), E.should(E.wildcard(b"zorbl*")), E.should(E.wildcard(b"za*"))])
    return qs


def got_lists(arrays):
    docs, scores, offs, _ = arrays
    d, s, o = docs.tolist(), scores.view(np.uint32).tolist(), offs.tolist()
    return [list(zip(d[o[i]:o[i + 1]], s[o[i]:o[i + 1]])) for i in range(len(o) - 1)]


def check(h, ref, queries):
    got = got_lists(h.search_compound_batch_arrays(queries))
    assert len(got) == len(queries)
    for q, g in zip(queries, got):
        assert g == CR.exact(ref.search(q)), q
    return got


@pytest.fixture(scope="module")
def route_index():
    g = ShardIndex()
    add(g, DOCS)
    g.commit()
    yield g
    g.close()


@pytest.fixture(scope="module")
def lucene():
    with open(os.path.join(HERE, "golden", "lucene_sample8.json")) as f:
        fx = json.load(f)
    texts = [d["text"].encode() for d in fx["docs"]]
    g = ShardIndex()
    g.add_documents(texts, [d["name"].encode() for d in fx["docs"]])
    g.commit()
    yield g, texts
    g.close()


# 1 ------------------------------------------------------------------------------------------

def test_every_kind_with_every_occur_and_every_other_kind(route_index):
    ref, qs = ref_of(BASE), batch()
    got = check(route_index, ref, qs)
    with route_index.reader() as rd:
        assert got_lists(rd.search_compound_batch_arrays(qs)) == got
    # the batch reaches its cases
    by_blocks = [{d // BLOCK for d, _ in g} for g in got]
    assert any(b == {0, 1, 2, 3} for b in by_blocks) and by_blocks[-1] == {0, 2}
    assert sum(1 for g in got if g) > len(got) // 3 and sum(1 for g in got if not g) > 20
    assert len(qs[-3]) == 64 and len(got[-3]) > BLOCK    # the 64-clause query hits documents of every block
    assert {d // BLOCK for d, _ in got[-3]} == {0, 1, 2, 3}
    entries, chunks, pairs, ms = route_index.last_compound_stats()
    assert chunks == 1 and pairs == len(qs) * 4 and entries > 100000 and ms > 0.0


def test_the_lucene_fixture(lucene):
    g, texts = lucene
    ref = CR.CompoundRef(texts)
    T = E.text
    qs = [[E.must(T(b"fast")), E.should(T(b"food"))], [E.should(T(b"best")), E.should(T(b"wireless")), E.should(T(b"earbuds"))],
          [E.must(E.phrase(b"fast food", 0))], [E.must(E.phrase(b"food fast", 2)), E.must_not(T(b"kheder"))],
          [E.filter_(E.wildcard(b"*")), E.should(T(b"fast"))], [E.must(E.wildcard(b"f*")), E.should(E.fuzzy(b"fsat", 2, 0, 50))],
          [E.should(E.regex(b"f(a|o).*")), E.must_not(E.fuzzy(b"food", 1, 1, 5))], [E.must_not(T(b"fast"))], [],
          [E.should(T(b"fast AND food")), E.should(T(b"fast OR (")), E.filter_(T(b"best fast"))]]
    got = check(g, ref, qs)
    with g.reader() as rd:
        assert got_lists(rd.search_compound_batch_arrays(qs)) == got
    assert sum(1 for x in got if x) >= 6 and got[7] == [] and got[8] == []
    for q, want in zip(qs, got):                         # the batch of one
        assert [(d, CR.bits(s)) for d, s in g.search_compound(q)] == want
    ref.close()


# 2 ------------------------------------------------------------------------------------------

def canon(*arrays):
    return [(a.dtype.str, a.tobytes()) for a in arrays]


def test_a_one_clause_query_is_its_route_row_byte_for_byte(route_index):
    g = route_index
    ph = [p for p in RR.PHRASES for _ in RR.SLOPS]
    sl = [s for _ in RR.PHRASES for s in RR.SLOPS]
    for oc in (E.should, E.must):
        d, s, o, _ = g.search_compound_batch_arrays([[oc(E.text(q))] for q in RR.QUERIES])
        assert canon(d, s, o) == canon(*g.search_batch_all_arrays(RR.QUERIES))
        d, s, o, _ = g.search_compound_batch_arrays([[oc(E.phrase(p, x))] for p, x in zip(ph, sl)])
        pd, ps, _, po = g.search_phrase_slop_batch_arrays(ph, sl)[:4]
        assert canon(d, s, o) == canon(pd, ps, po)
        d, s, o, _ = g.search_compound_batch_arrays([[oc(E.fuzzy(t, 2, 0, RR.EXPANSIONS))] for t in RR.FUZZY])
        fd, fs, fo = g.search_fuzzy_batch_arrays(RR.FUZZY, 2, 0, RR.EXPANSIONS)[:3]
        assert canon(d, s, o) == canon(fd, fs, fo)
        for kind, pats, route in ((E.wildcard, RR.WILDCARDS, g.search_wildcard_batch_arrays),
                                  (E.regex, RR.REGEXES, g.search_regex_batch_arrays)):
            d, s, o, _ = g.search_compound_batch_arrays([[oc(kind(p))] for p in pats])
            wd, wo = route(pats)[:2]
            assert canon(d, o) == canon(wd, wo) and set(s.view(np.uint32).tolist()) == {CR.bits(1.0)}
            for i in range(len(pats)):                   # a set row: ascending documents
                row = d[int(o[i]):int(o[i + 1])].tolist()
                assert row == sorted(row)


def test_the_operator_word_identities(route_index):
    g = route_index
    words = [RR.M1, RR.M2, RR.M3, RR.MX, RR.PIV_A, RR.c(7), RR.c(1), RR.c(120), RR.LONG_TERM, RR.FUZ[1]]
    pairs = [(a, b) for a in words for b in words if a != b][:40]
    T = E.text
    for make, word in ((lambda a, b: [E.must(T(a)), E.must(T(b))], b" AND "),
                       (lambda a, b: [E.must(T(a)), E.must_not(T(b))], b" AND NOT "),
                       (lambda a, b: [E.should(T(a)), E.should(T(b))], b" ")):
        d, s, o, _ = g.search_compound_batch_arrays([make(a, b) for a, b in pairs])
        assert canon(d, s, o) == canon(*g.search_batch_all_arrays([a + word + b for a, b in pairs])), word
        assert len(d) > 20 and sum(1 for i in range(len(pairs)) if o[i + 1] > o[i]) >= 5     # not a vacuous comparison


# 3 ------------------------------------------------------------------------------------------

def test_chunking_does_not_change_the_bytes(route_index, monkeypatch):
    g, qs = route_index, batch()[::3] + batch()[-4:]
    d0, s0, o0, _ = g.search_compound_batch_arrays(qs)
    entries0, chunks0, _, _ = g.last_compound_stats()
    assert chunks0 == 1
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    for budget in ("5", "40000"):
        monkeypatch.setenv("TFIDF_COMPOUND_CHUNK", budget)
        d, s, o, _ = g.search_compound_batch_arrays(qs)
        assert canon(d, s, o) == canon(d0, s0, o0)
        entries, chunks, pairs, _ = g.last_compound_stats()
        assert chunks > 1 and entries == entries0 and pairs == len(qs) * 4
        if budget == "5":
            assert chunks > len(qs) // 2                 # only a query without entries shares a chunk
    monkeypatch.setenv("TFIDF_COMPOUND_CHUNK", "5")
    big = [[E.must(E.wildcard(b"*")), E.should(E.text(RR.M1))]]          # 25 200 entries and more under a budget of 5
    d, s, o, _ = g.search_compound_batch_arrays(big)
    assert g.last_compound_stats()[1] == 1 and len(d) == len(BASE)
    monkeypatch.delenv("TFIDF_COMPOUND_CHUNK")
    d1, s1, o1, _ = g.search_compound_batch_arrays(big)
    assert canon(d, s, o) == canon(d1, s1, o1)


# 4 ------------------------------------------------------------------------------------------

def test_ties_come_out_in_document_order_across_the_block_edge(route_index):
    g = route_index
    star, mq = E.wildcard(b"*"), E.regex(b"mq.*")
    d, s, o, _ = g.search_compound_batch_arrays([[E.must(star), E.must(E.regex(b".*"))], [E.filter_(star)],
                                                 [E.should(mq), E.should(E.wildcard(b"mq*"))], [E.filter_(mq)]])
    o = o.tolist()
    n = len(BASE)
    assert o[:3] == [0, n, 2 * n]
    for i, bits in enumerate((CR.bits(2.0), CR.bits(0.0), CR.bits(2.0), CR.bits(0.0))):
        row = d[o[i]:o[i + 1]].tolist()
        assert row == sorted(row) and set(s[o[i]:o[i + 1]].view(np.uint32).tolist()) == {bits}
        assert BLOCK - 1 in row and BLOCK in row         # the edge documents hold mq words
    assert d[:n].tolist() == list(range(n))


# 5 ------------------------------------------------------------------------------------------

def raw(fn, handle, queries, cap, sentinel=0xAB):
    """One library call on sentinel-filled outputs -> (rc, docs, scores, offsets, n)."""
    blob, c_offs, arr, q_offs = E._clause_arrays(queries)
    docs = np.full(max(cap, 1), sentinel, np.uint32)
    scores = np.full(max(cap, 1), np.float32(-7.0))
    offs = np.full(len(queries) + 1, sentinel, np.uint64)
    n = C.c_uint64(sentinel)
    rc = fn(handle, blob, L.ptr(c_offs, C.c_uint64), arr, L.ptr(q_offs, C.c_uint64), len(queries),
            L.ptr(docs, C.c_uint32) if cap else None, L.ptr(scores, C.c_float) if cap else None, cap,
            L.ptr(offs, C.c_uint64), C.byref(n), None)
    return rc, docs, scores, offs, n.value


def untouched(res, sentinel=0xAB):
    _, docs, scores, offs, n = res
    return (set(docs.tolist()) == {sentinel} and set(scores.tolist()) == {-7.0} and set(offs.tolist()) == {sentinel} and
            n == sentinel)


def test_protocol_and_errors(route_index):
    g = route_index
    fn = L.load().tfidf_search_compound_batch
    T = E.text
    assert g.search_compound_batch([]) == []
    rc, _, _, offs, n = raw(fn, g._h, [], 0)
    assert (rc, offs.tolist(), n) == (L.OK, [0], 0)
    assert g.search_compound_batch([[], [E.should(T(RR.M1))], []])[0::2] == [[], []]
    qs = [[E.should(T(RR.M1))], [E.must(T(RR.M2)), E.must_not(T(RR.M1))]]
    want = got_lists(g.search_compound_batch_arrays(qs))
    total = sum(len(w) for w in want)
    assert total > 4
    rc, docs, scores, offs, n = raw(fn, g._h, qs, 0)     # the size query
    assert rc == L.E_BUFFER and n == total and offs.tolist() == [0, len(want[0]), total]
    rc, docs, scores, offs, n = raw(fn, g._h, qs, total - 1)
    assert rc == L.E_BUFFER and n == total and offs.tolist() == [0, len(want[0]), total]
    rc, docs, scores, offs, n = raw(fn, g._h, qs, total)
    assert rc == L.OK and n == total and list(zip(docs.tolist(), scores.view(np.uint32).tolist())) == want[0] + want[1]
    # argument errors: nothing written
    res = raw(fn, g._h, [[E.should(T(RR.c(i + 1))) for i in range(65)]], 64)
    assert res[0] == L.E_INVALID_ARG and untouched(res)
    res = raw(fn, g._h, [[E.should(T(RR.M1))], [(L.OCCUR_MUST, 5, RR.M1)]], 64)
    assert res[0] == L.E_INVALID_ARG and untouched(res) and b"kind" in L.load().tfidf_last_error()
    res = raw(fn, g._h, [[(4, L.CLAUSE_TEXT, RR.M1)]], 64)
    assert res[0] == L.E_INVALID_ARG and untouched(res)
    # a route's failure fails the call with the route's code, nothing written, the clause named
    res = raw(fn, g._h, [[E.should(T(RR.M1))], [E.must(E.regex(b"mq.*"))], [E.should(T(RR.M2)), E.must(E.regex(b"a(b"))]], 64)
    assert res[0] == L.E_QUERY_SYNTAX and untouched(res)
    assert L.load().tfidf_last_error().startswith(b"query 2 clause 1:")
    res = raw(fn, g._h, [[E.should(T(RR.M1)), E.must(E.phrase(RR.M1 + b" " + RR.M1, 1))]], 64)
    assert res[0] == L.E_UNSUPPORTED_QUERY and untouched(res)
    assert L.load().tfidf_last_error().startswith(b"query 0 clause 1:")
    for bad in (E.fuzzy(RR.FUZ[0], 3, 0, 50), E.fuzzy(RR.FUZ[0], 2, 0, 65), E.fuzzy(RR.FUZ[0], 2, 0, 0)):
        res = raw(fn, g._h, [[E.should(bad)]], 64)
        assert res[0] == L.E_INVALID_ARG and untouched(res)
    with pytest.raises(L.TfidfError) as e:
        g.search_compound([E.must(E.regex(b"a(b"))])
    assert e.value.code == L.E_QUERY_SYNTAX
    # the index still answers
    assert got_lists(g.search_compound_batch_arrays(qs)) == want


def test_a_call_before_the_first_commit_is_a_state_error():
    g = ShardIndex()
    g.add_documents([b"alpha beta"], [b"k"])
    res = raw(L.load().tfidf_search_compound_batch, g._h, [[E.should(E.text(b"alpha"))]], 8)
    assert res[0] == L.E_STATE and untouched(res)
    g.close()


# 6 ------------------------------------------------------------------------------------------

def lifecycle_queries():
    T = E.text
    new = RR.NEW_WORDS[0]
    return [[E.must(T(RR.M1)), E.should(T(RR.M2)), E.must_not(E.phrase(RR.P_GAP, 0))],
            [E.should(T(new)), E.should(E.wildcard(RR.OLD_AND_NEW)), E.should(E.fuzzy(RR.N1, 1, 0, 50))],
            [E.filter_(E.regex(RR.REGEXES[3])), E.should(T(RR.LONG_TERM)), E.should(E.fuzzy(RR.FUZ[0], 2, 0, 50))],
            [E.must(E.wildcard(b"zorbl*")), E.must_not(T(RR.FUZ[1]))],
            [E.should(E.phrase(RR.M1 + b" " + RR.M2, 1)), E.should(T(RR.PIV_A)), E.must_not(T(new))]]


def test_a_reader_keeps_its_corpus_across_a_commit_and_deletes_renumber():
    qs = lifecycle_queries()
    g = ShardIndex()
    add(g, DOCS[:FIRST_A])
    g.commit()
    rd = g.reader()
    old = check(rd, ref_of(A0), qs)
    batch2 = RR.new_batch()
    add(g, keyed(batch2, FIRST_A))
    g.commit()
    texts = A0 + batch2
    new = check(g, ref_of(texts), qs)
    assert check(rd, ref_of(A0), qs) == old and new != old and new[1] != old[1]
    rd.close()
    dead = [3, 11, BLOCK - 1, FIRST_A + 1]               # a phrase document, "zorblat", the edge document, N1's document
    assert texts[FIRST_A + 1] == RR.N1_DOC
    keys = [DOCS[i][0] for i in dead[:3]] + [keyed(batch2, FIRST_A)[1][0]]
    assert g.delete_documents(keys) == len(dead)
    g.commit()
    live = [t for i, t in enumerate(texts) if i not in dead]
    after = check(g, ref_of(live), qs)
    assert after != new and g.stats()["num_docs"] == len(live)
    g.close()


# 7 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ctor", [dict(inversion=L.INVERSION_TERM), dict(k1=2.0, b=1.0), dict(stream=True)],
                         ids=["term_major", "k1_b", "caller_stream"])
def test_other_layouts_parameters_and_a_caller_stream(ctor):
    import torch
    ctor = dict(ctor)
    on_stream = ctor.pop("stream", False)
    qs = lifecycle_queries() + batch()[20:60:5]
    ref = ref_of(A0, ctor.get("k1", 1.2), ctor.get("b", 0.75))
    g = ShardIndex(**ctor)
    st = torch.cuda.Stream() if on_stream else None
    try:
        if st is not None:
            g.set_stream(st.cuda_stream)
        add(g, DOCS[:FIRST_A])
        g.commit()
        if "inversion" in ctor:
            assert g.stats()["term_major"] == 1
        got = check(g, ref, qs)
        assert sum(1 for x in got if x) >= 5
        if "k1" in ctor:
            assert got[0] != CR.exact(ref_of(A0).search(qs[0]))          # the parameters reach the scores
    finally:
        if st is not None:
            g.set_stream(None)
        g.close()


# 8 ------------------------------------------------------------------------------------------

def test_worker_search_query(tmp_path):
    texts = BASE[:40] + [RR.P_FULL + b" " + RR.FUZ[0], RR.P_FULL + b" " + RR.PIV_A, RR.FUZ[3] + b" " + RR.M1, RR.P_REV,
                         RR.M1 + b" " + RR.M2 + b" " + RR.c(9)]
    docs = tmp_path / "docs"
    docs.mkdir()
    names = ["d%03d.txt" % i for i in range(len(texts))]
    for n, t in zip(names, texts):
        (docs / n).write_bytes(t)
    w = Worker(documents_path=str(docs))
    w.init()
    with w.index.reader() as rd:
        order = [rd.doc_key(d).decode() for d in range(rd.num_docs)]
    by_name = dict(zip(names, texts))
    ref = CR.CompoundRef([by_name[n] for n in order])
    q = '+"mqalpha mqbeta" zorbl* -pivotalfa'
    want = ref.search([E.must(E.phrase(b"mqalpha mqbeta", 0)), E.should(E.wildcard(b"zorbl*")), E.must_not(E.text(b"pivotalfa"))])
    assert len(want) >= 3 and len({CR.bits(s) for _, s in want}) >= 2
    assert w.search_query(q, k=0) == [{"document": {"name": order[d]}, "score": float(s)} for d, s in want]
    assert w.search_query(q, k=2) == w.search_query(q, k=0)[:2]
    assert w.search_query("", k=0) == []
    with pytest.raises(L.QuerySyntaxError):
        w.search_query('"open')
    ref.close()
    w.index.close()
