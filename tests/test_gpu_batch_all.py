"""Batched all-hits search (tfidf_search_batch_all: searcher.search(q,
Integer.MAX_VALUE), Worker.java:230, for many requests in one pass) against the
C oracle's search(q, 0) per query and the engine's own single search(q, 0).
Bar: doc ids and float32 score bits identical.

Corpora, the smallest at which each merge structure can go wrong:
  300 docs              1 block  (no merge level: only the padding run)
  20 000 docs, V = 2000 3 blocks (not a power of two, below the 8-run group
                                  width: a group or a pairwise level that
                                  crossed a query boundary would mix queries)
  80 000 docs, V = 2000 10 blocks (group merge + one pairwise level; the corpus
                                  and queries of test_gpu_hits_merge.py, with
                                  groups over the LDS capacity)
"""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker
from test_gpu_hits_merge import QUERIES as MERGE_QUERIES
from test_gpu_parity import assert_hits_equal, build_pair

pytestmark = pytest.mark.gpu

W = synth.word                      # rank -> term; at V = 2000 ranks 1-3 each hit 30-60 % of the documents

# 14 queries: empty results first, in the middle and last; 1-, 2- and 3-term
# disjunctions (with terms in more than half the documents), operator queries,
# a pure negative, an unknown term, one that does not parse, one query twice
BATCH = [
    b"zzzzqq",                                        # unknown term
    W(1),
    W(1) + b" " + W(2),
    W(30) + b" " + W(200) + b" " + W(1500),
    b"AND",                                           # does not parse
    W(1) + b" AND " + W(3),
    W(1) + b" NOT " + W(2),
    W(5) + b" OR " + W(40) + b" AND " + W(7),
    b"NOT " + W(1),                                   # pure negative
    W(3) + b" " + W(1) + b" " + W(2),
    W(30) + b" " + W(200) + b" " + W(1500),           # the same query again
    W(700),
    W(150) + b" " + W(900),
    b"qqqqzz",                                        # unknown term
]


def oracle_hits(o, q):
    try:
        return o.search(q, 0)
    except O.QuerySyntaxError:
        return []                                     # Worker.java:182-185: the request answers []


def single_hits(g, q):
    try:
        return g.search(q, 0)
    except L.QuerySyntaxError:
        return []


def check_batch(g, o, queries, want=None):
    got = g.search_batch_all(queries)
    assert len(got) == len(queries)
    for i, q in enumerate(queries):
        assert_hits_equal(got[i], want[i] if want else oracle_hits(o, q))
    return got


@pytest.fixture(scope="module")
def small():
    g, o = build_pair(synth.corpus(300, V=2000, len_min=2, len_max=12))
    yield g, o
    g.close()
    o.close()


@pytest.fixture(scope="module")
def mid():
    """R = 3: block-major and term-major indexes of one corpus, the oracle and
    its answers to BATCH."""
    texts = synth.corpus(20_000, V=2000, len_min=2, len_max=12)
    _, o = pair = build_pair(texts)
    pair[0].close()
    idx = {}
    for name, inv in (("block", L.INVERSION_BLOCK), ("term", L.INVERSION_TERM)):
        idx[name] = ShardIndex(inversion=inv)
        idx[name].add_documents(texts)
        idx[name].commit()
    g, gt = idx["block"], idx["term"]
    assert g.stats()["term_major"] == 0 and gt.stats()["term_major"] == 1
    want = [oracle_hits(o, q) for q in BATCH]
    yield {"block": g, "term": gt, "o": o, "want": want, "texts": texts}
    g.close()
    gt.close()
    o.close()


@pytest.fixture(scope="module")
def big():
    g, o = build_pair(synth.corpus(80_000, V=2000, len_min=2, len_max=12))
    want = [o.search(q, 0) for q in MERGE_QUERIES]
    yield g, o, want
    g.close()
    o.close()


def test_one_block(small):
    g, o = small
    got = check_batch(g, o, BATCH)
    assert sum(len(h) for h in got) > 300             # queries share documents: more hits than documents
    for q, h in zip(BATCH, got):
        assert h == single_hits(g, q)


@pytest.mark.parametrize("layout", ["block", "term"])
def test_three_blocks(mid, layout):
    g = mid[layout]
    want = mid["want"]
    assert len(want[1]) > 10_000 and len(want[2]) > 10_000       # terms in more than half the documents
    assert [len(want[i]) for i in (0, 4, 8, 13)] == [0, 0, 0, 0]   # empty first, middle, last
    assert all(len(want[i]) for i in (1, 2, 3, 5, 6, 7, 9, 10, 11, 12))
    got = check_batch(g, None, BATCH, want)
    for q, h in zip(BATCH, got):
        assert h == single_hits(g, q)


@pytest.mark.parametrize("layout", ["block", "term"])
def test_one_query_and_none(mid, layout):
    g = mid[layout]
    for i in (2, 4, 7):
        assert_hits_equal(g.search_batch_all([BATCH[i]])[0], mid["want"][i])
    assert g.search_batch_all([]) == []
    d, s, offs = g.search_batch_all_arrays([])
    assert len(d) == 0 and len(s) == 0 and offs.tolist() == [0]


@pytest.mark.parametrize("layout", ["block", "term"])
@pytest.mark.parametrize("chunk", ["3", "1"])
def test_chunks_equal_one_pass(mid, monkeypatch, layout, chunk):
    """TFIDF_ALLHITS_CHUNK=3: 14 queries in five chunks, the last of two."""
    g = mid[layout]
    ref = g.search_batch_all(BATCH)
    monkeypatch.setenv("TFIDF_ALLHITS_CHUNK", chunk)
    got = check_batch(g, None, BATCH, mid["want"])
    assert got == ref


@pytest.mark.parametrize("force", [None, "TFIDF_HITS_GROUPS", "TFIDF_HITS_PAIRWISE"])
def test_ten_blocks_merge_paths(big, monkeypatch, force):
    g, o, want = big
    if force:
        monkeypatch.setenv(force, "1")
    big_q = sum(len(w) > 8 * 8192 * 0.125 for w in want)
    assert big_q >= 2                                  # groups over the LDS capacity exist
    # empty queries around and between the heavy ones
    qs = [b"zzzzqq"] + list(MERGE_QUERIES[:7]) + [b"AND"] + list(MERGE_QUERIES[7:]) + [b"qqqqzz"]
    ws = [[]] + want[:7] + [[]] + want[7:] + [[]]
    got = check_batch(g, o, qs, ws)
    if force is None:
        for q, h in zip(qs, got):
            assert h == single_hits(g, q)


def test_ten_blocks_chunked(big, monkeypatch):
    g, o, want = big
    monkeypatch.setenv("TFIDF_ALLHITS_CHUNK", "3")
    check_batch(g, o, list(MERGE_QUERIES), want)


@pytest.mark.parametrize("inversion", [L.INVERSION_BLOCK, L.INVERSION_TERM])
def test_terms_past_the_first_four(inversion):
    """The scorer prefetches a query's first four terms; whether a (query, block)
    pair is empty must also see the later ones.  Three blocks: the first four
    terms occur only in block 0, the fifth only in block 2, the sixth only in
    block 1, a MUST_NOT term everywhere."""
    texts = [b"filler"] * 17_000
    for d in (5, 900, 8000):
        texts[d] = b"alpha beta gamma delta filler"
    for d in (8192, 12_000, 16_383):
        texts[d] = b"zeta zeta filler"
    for d in (16_384, 16_999):
        texts[d] = b"epsilon filler"
    o = O.OracleIndex()
    for i, t in enumerate(texts):
        o.add_doc(str(i).encode(), t)
    o.commit()
    g = ShardIndex(inversion=inversion)
    g.add_documents(texts)
    g.commit()
    qs = [b"alpha beta gamma delta epsilon zeta",
          b"alpha beta gamma delta epsilon zeta NOT filler",          # every pair: only the MUST_NOT term scores nothing
          b"alpha beta gamma delta nothing epsilon",
          b"alpha beta gamma delta (epsilon AND filler) zeta"]
    got = check_batch(g, o, qs)
    assert [d for d, _ in sorted(got[0])] == [5, 900, 8000, 8192, 12_000, 16_383, 16_384, 16_999]
    assert got[1] == [] and len(got[2]) == 5
    g.close()
    o.close()


@pytest.mark.parametrize("reader", [False, True])
def test_buffer_protocol(mid, reader):
    g, want = mid["block"], mid["want"]
    cum = np.cumsum([0] + [len(w) for w in want]).tolist()
    total = cum[-1]
    offs = np.zeros(len(BATCH) + 1, np.uint64)
    offs[1:] = np.cumsum([len(q) for q in BATCH], dtype=np.uint64)
    blob = b"".join(BATCH)
    rd = g.reader() if reader else None
    fn = L.load().tfidf_reader_search_batch_all if reader else L.load().tfidf_search_batch_all
    h = rd._h if reader else g._h

    def call(cap):
        docs = np.zeros(cap, np.uint32)
        scores = np.zeros(cap, np.float32)
        ho = np.full(len(BATCH) + 1, 99, np.uint64)
        n = C.c_uint64(99)
        rc = fn(h, blob, L.ptr(offs, C.c_uint64), len(BATCH), L.ptr(docs, C.c_uint32), L.ptr(scores, C.c_float), cap,
                L.ptr(ho, C.c_uint64), C.byref(n))
        return rc, n.value, ho.tolist(), docs, scores

    rc, n, ho, _, _ = call(total - 1)
    assert (rc, n, ho) == (L.E_BUFFER, total, cum)
    rc, n, ho, docs, scores = call(total)
    assert (rc, n, ho) == (L.OK, total, cum)
    for i, w in enumerate(want):
        assert_hits_equal(list(zip(docs[cum[i]:cum[i + 1]].tolist(), scores[cum[i]:cum[i + 1]].tolist())), w)
    if rd:
        rd.close()
    # the wrapper's retry: a first attempt of one slot, then the reported size
    d, s, o2 = g.search_batch_all_arrays(BATCH, cap=1)
    assert o2.tolist() == cum and d.tolist() == docs.tolist() and s.tolist() == scores.tolist()


def test_reader_keeps_its_snapshot(mid):
    g = ShardIndex()
    g.add_documents(mid["texts"])
    g.commit()
    with g.reader() as rd:
        g.add_documents(synth.corpus(9000, V=2000, len_min=2, len_max=12, doc_base=20_000))
        g.commit()
        got = rd.search_batch_all(BATCH)
        now = g.search_batch_all(BATCH)
    for h, w in zip(got, mid["want"]):
        assert_hits_equal(h, w)
    assert len(now[1]) > len(got[1])                   # the index itself answers from the second commit
    g.close()


def test_coalesced_all_hits_and_top_k(mid):
    g, o = mid["block"], mid["o"]
    qs = [BATCH[i] for i in (1, 2, 3, 5, 6, 7, 9, 12)]
    jobs = [(q, 0) for q in qs] + [(q, 10) for q in qs]
    before = g.stats()
    out = [None] * len(jobs)
    gate = threading.Barrier(len(jobs))

    def run(i):
        gate.wait()
        try:
            out[i] = g.search_coalesced(jobs[i][0], jobs[i][1], wait_us=200)
        except Exception as e:                         # reported by the assertions below
            out[i] = e

    th = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for (q, k), got in zip(jobs, out):
        assert isinstance(got, list), got
        assert_hits_equal(got, o.search(q, k))
    st = g.stats()
    assert st["coalesced_queries"] - before["coalesced_queries"] == 16
    assert st["coalesced_batches"] - before["coalesced_batches"] < 16

    # one all-hits caller with a single result slot; its companions are served
    jobs2 = [(qs[0], 0, 1), (qs[1], 0, None), (qs[2], 0, None), (qs[3], 10, None)]
    out2 = [None] * len(jobs2)
    gate2 = threading.Barrier(len(jobs2))

    def run2(i):
        gate2.wait()
        q, k, cap = jobs2[i]
        try:
            out2[i] = g.search_coalesced(q, k, wait_us=200, cap=cap)
        except L.TfidfError as e:
            out2[i] = e

    th = [threading.Thread(target=run2, args=(i,)) for i in range(len(jobs2))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert isinstance(out2[0], L.TfidfError) and out2[0].code == L.E_BUFFER
    for (q, k, _), got in list(zip(jobs2, out2))[1:]:
        assert_hits_equal(got, o.search(q, k))


def test_coalesced_buffer_error_reports_the_size(mid):
    g, want = mid["block"], mid["want"]
    docs = np.zeros(1, np.uint32)
    scores = np.zeros(1, np.float32)
    n = C.c_uint64()
    rc = L.load().tfidf_search_coalesced(g._h, BATCH[3], len(BATCH[3]), 0, L.ptr(docs, C.c_uint32),
                                         L.ptr(scores, C.c_float), 1, C.byref(n), 0)
    assert (rc, n.value) == (L.E_BUFFER, len(want[3]))


def test_worker_batch_json(lucene_fixture):
    w = Worker()
    w.index.add_documents([d["text"].encode() for d in lucene_fixture["docs"]],
                          [d["name"].encode() for d in lucene_fixture["docs"]])
    w.commit()
    qs = ["fast food", "nothing here", "best wireless earbuds", "AND", "kheder", "fast AND food", "fast food"]
    per = [w.process_documents(q) for q in qs]
    assert per[0] and per[2] and per[4] and per[3] == []
    assert w.process_documents_batch(qs) == per
    assert w.process_documents_batch([]) == []
    w.close()
