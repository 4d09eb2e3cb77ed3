"""The index on a caller's stream (tfidf_set_stream with a torch stream): the
commits, every query route, compaction and concurrent searches of the other
test files, which run all of them on the index's own stream.

With a caller's stream installed ix->stream and ix->user_stream change: the
writers (commit, compaction, the exchange) queue their work on it and every
search and reader runs on that one stream instead of its context's own
(CtxLease::stream()).  What each case reaches in tfidf_capi.hip:

  a, b  commit_once with mirror_side == false: a caller's stream and a
        dictionary below 32 MB (2^18 slots x 16 B = 4 MB, the constructor's
        default).  The whole and delta dictionary, df and column-rank mirrors
        are copied on the main stream behind the inversion, and the deferred
        hashed-key identity check (launch_verify_deferred) and, term-major,
        launch_count_nonzero run there too.  b is the only check that the
        identity check on that branch sees the collision the side-stream one
        sees (TFIDF_TEST_WEAK_HASH).
  c     mirror_side forced by the dictionary's size on a stream that is not the
        index's own (vocab_capacity_log2 = 21: 2^21 x 16 B = 32 MB, the
        smallest such capacity): side_work with mir_ev[0] and mir_ev[2]
        recorded on the caller's stream, waited for by copy_stream, and
        mir_ev[1] waited for by the caller's stream.
  d     every route of routes_ref.sweep on one shared stream, on the index and
        on a reader, and once more with tfidf_set_query_timing(0) on either
        stream (X.q_timing guards the event records of the phrase, highlight,
        all-hits, wildcard and fuzzy paths).
  e     tfidf_set_stream between commits; a reader opened on the caller's
        stream whose searches move to the contexts' own streams.
  f     compact_locked's gather copy on ix->stream, with a reader held across it.
  g     four threads on one index: on a caller's stream all search contexts
        share one queue and keep their own events and pinned buffers.
  h     tfidf_set_stream(ix, NULL): the writers on the legacy default stream,
        searches on their contexts' own streams (user_stream stays null).

The references are those of the tests whose histories are replayed: a fresh
one-commit index that never leaves its own stream and the CPU oracle
(test_gpu_incremental_commit.assert_same_as_fresh), and routes_ref.expected.
Every comparison is exact (float32 scores by their bits, arrays byte for byte).
Every test puts the index back on its own stream before it closes it or drops
the torch stream: tfidf_destroy synchronises ix->stream.
"""
import contextlib
import threading

import numpy as np
import pytest
import torch

import routes_ref as RR
from routes_ref import APPEND_A, BASE, BLOCK, FIRST_A, expected, hit_bits, sweep
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_incremental_commit import LONG_TERM, QUERIES, add, commit_and_expect, keyed, more_docs, path_batch
from test_gpu_routes_incremental import A1, DOCS
from test_gpu_routes_incremental import commit as route_commit

pytestmark = pytest.mark.gpu

MIRRORS = ("mirror_dict", "mirror_df", "mirror_crank")
SMALL, SMALL_APPEND = 300, 30                            # a corpus of seconds for the cases that need no block edge


@contextlib.contextmanager
def caller_stream(*indexes):
    """A torch stream installed on the indexes; their own streams again on the way out."""
    st = torch.cuda.Stream()
    try:
        for g in indexes:
            g.set_stream(st.cuda_stream)
        yield st
    finally:
        for g in indexes:
            g.set_stream(None)


def mirror_forms(g):
    p = g.commit_host_profile()
    return tuple(p[m] for m in MIRRORS)


def both_snapshots_full(g, docs):
    """`docs` added and committed into both snapshots; each one's first build is a full one."""
    add(g, docs)
    for _ in range(2):
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": len(docs), "was_full": True}


def scorer_sweep(h, exp):
    """The scorer part of routes_ref.sweep."""
    w = exp.want
    for q, got in zip(RR.QUERIES, h.search_batch_all(RR.QUERIES)):
        assert hit_bits(got) == w["search", q, 0], q
    docs, scores, counts = h.search_batch(RR.QUERIES, 10)
    for i, q in enumerate(RR.QUERIES):
        n = int(counts[i])
        assert list(zip(docs[i, :n].tolist(), scores[i, :n].view(np.uint32).tolist())) == w["search", q, 10], q
        assert hit_bits(h.search(q, 10)) == w["search", q, 10], q


# a. commits on a caller's stream: the mirrors on the main stream --------------------------------

ESCAPE_DOC = b"zq zq " + b"ab " * 17000 + b"tail"        # tf 17 000 >= 2047: a posting escape (and a CSR escape)


@pytest.mark.parametrize("ctor", [{}, dict(inversion=L.INVERSION_TERM)], ids=["block", "term"])
def test_commits_mirror_on_the_main_stream(ctor):
    first = keyed(synth.corpus(SMALL, V=3000, len_min=20, len_max=80))
    later = keyed(path_batch() + [ESCAPE_DOC], SMALL)
    more = keyed(path_batch()[:40] + [b"another bad \xc3 one"], SMALL + len(later))
    qs = QUERIES[:12] + ["café".encode(), "it’s".encode(), "中文".encode(), LONG_TERM, b"fine text", b"ab zq tail"]
    # (batch added before the commit, documents the commit tokenizes)
    history = [(first, SMALL), ([], SMALL),                       # both snapshots, in full
               (later, len(later)),                               # a delta dictionary mirror + the deferred identity check
               ([], len(later)), ([], 0),                         # nothing added: the other snapshot; nothing at all
               (more, len(more))]
    g, h = ShardIndex(**ctor), ShardIndex(**ctor)                 # h replays the history on its own stream
    try:
        with caller_stream(g):
            docs = []
            for i, (batch, n_tok) in enumerate(history):
                if batch:
                    add(g, batch)
                    add(h, batch)
                    docs = docs + batch
                commit_and_expect(g, docs, n_tok, i < 2, queries=qs, **ctor)
                h.commit()
                assert h.commit_tokenized_docs() == g.commit_tokenized_docs()
                assert mirror_forms(g) == mirror_forms(h), i      # the mirror plan does not depend on the stream
                assert g.stats()["term_major"] == (1 if ctor else 0)
                if i == 2:                                        # term-major mirrors whole; block-major the new slots
                    assert mirror_forms(g)[0] == ("whole" if ctor else "delta")
            assert g.doc_terms(SMALL + len(later) - 1) == {b"zq": 2, b"ab": 17000, b"tail": 1}
            s = g.stats()
            assert s["long_docs"] >= 2 and s["unicode_docs"] >= 3 and s["malformed_docs"] >= 3
    finally:
        g.close()
        h.close()


# b. a collision detected on the main stream ------------------------------------------------------

def weak_hash_history(on_caller):
    """test_weak_hash_rebuilds_every_commit's scenario -> hash_rebuilds after each commit."""
    twin = LONG_TERM[:-1] + b"z"                                  # collides with LONG_TERM under the weak seed
    docs = keyed(synth.corpus(100, V=3000, len_min=20, len_max=80) + [LONG_TERM + b" and " + twin])
    qs = QUERIES[:6] + [LONG_TERM, twin]
    g = ShardIndex()
    rebuilds = []
    try:
        with caller_stream(g) if on_caller else contextlib.nullcontext():
            add(g, docs)
            commit_and_expect(g, docs, 101, True, queries=qs)
            rebuilds.append(g.stats()["hash_rebuilds"])
            commit_and_expect(g, docs, 101, True, queries=qs)
            rebuilds.append(g.stats()["hash_rebuilds"])
            extra = more_docs(500)
            add(g, extra)
            docs += extra
            commit_and_expect(g, docs, 131, True, queries=qs)
            rebuilds.append(g.stats()["hash_rebuilds"])
            assert g.df(LONG_TERM) == g.df(twin) == (1, 1)
    finally:
        g.close()
    return rebuilds


def test_collision_detected_on_the_main_stream(monkeypatch):
    monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    own = weak_hash_history(False)
    assert own[0] == 1 and own[2] == 1
    assert weak_hash_history(True) == own


# c. a dictionary of 32 MB: the side stream fed by events of the caller's stream -----------------------

def test_large_dictionary_mirrors_on_the_side_stream():
    ctor = dict(vocab_capacity_log2=21)
    first = keyed(synth.corpus(SMALL, V=3000, len_min=20, len_max=80))
    later = keyed(synth.corpus(200, V=3000, len_min=20, len_max=80, doc_base=SMALL) +
                  [LONG_TERM + b" first seen here " + LONG_TERM], SMALL)
    qs = QUERIES[:10] + [LONG_TERM]
    g = ShardIndex(**ctor)
    try:
        with caller_stream(g):
            add(g, first)
            commit_and_expect(g, first, SMALL, True, queries=qs, **ctor)
            assert mirror_forms(g) == ("whole", "whole", "whole")
            g.commit()                                            # the other snapshot
            assert g.commit_tokenized_docs() == {"docs": SMALL, "was_full": True}
            add(g, later)
            commit_and_expect(g, first + later, len(later), False, queries=qs, **ctor)
            assert mirror_forms(g)[0] == "delta"                  # the new slots' keys come over the side stream
            commit_and_expect(g, first + later, len(later), False, queries=qs, **ctor)
    finally:
        g.close()


# d. every route on the caller's stream --------------------------------------------------------------

def test_every_route_on_the_caller_stream():
    g = ShardIndex()
    try:
        with caller_stream(g):
            both_snapshots_full(g, DOCS[:FIRST_A])
            add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
            for _ in range(2):                                    # either snapshot
                route_commit(g, len(A1), 1, APPEND_A)
                sweep(g, expected(A1))
            with g.reader() as rd:
                sweep(rd, expected(A1))
            g.set_query_timing(False)
            try:
                sweep(g, expected(A1))
                assert g.last_search_ms() == (-1.0, -1.0)
                g.set_stream(None)
                sweep(g, expected(A1))
                assert g.last_search_ms() == (-1.0, -1.0)
            finally:
                g.set_query_timing(True)
            assert g.search(RR.QUERIES[0], 10) and g.last_search_ms()[1] > 0
    finally:
        g.close()


# e. switching streams between commits -----------------------------------------------------------------

def test_switching_streams_between_commits():
    docs = keyed(BASE[:SMALL])
    extra = keyed(BASE[SMALL:SMALL + SMALL_APPEND], SMALL)
    g = ShardIndex()
    rd = None
    try:
        add(g, docs)
        commit_and_expect(g, docs, SMALL, True)                   # own stream
        commit_and_expect(g, docs, SMALL, True)
        add(g, extra)
        docs = docs + extra
        exp = expected([t for _, t in docs])
        with caller_stream(g):
            commit_and_expect(g, docs, SMALL_APPEND, False)       # incremental, on the caller's stream
            rd = g.reader()
            sweep(rd, exp)
            sweep(g, exp)
        commit_and_expect(g, docs, SMALL_APPEND, False)           # own stream again: the other snapshot, nothing added
        sweep(rd, exp)                                            # the reader's searches moved to the contexts' streams
        sweep(g, exp)
        with caller_stream(g):                                    # and back: the snapshot the reader holds is no target
            commit_and_expect(g, docs, len(docs), True)
            sweep(rd, exp)
        sweep(rd, exp)
    finally:
        if rd is not None:
            rd.close()
        g.close()


# f. delete, compact and commit on the caller's stream --------------------------------------------------

def test_delete_compact_then_incremental_on_the_caller_stream():
    dead = [0, 4, 13]                                             # as test_gpu_routes_incremental's case g
    live = [d for i, d in enumerate(DOCS[:FIRST_A]) if i not in dead]
    texts = [t for _, t in live]
    sample = list(range(0, len(texts), 97)) + list(range(24)) + [len(texts) - 1]
    g = ShardIndex()
    rd = None
    try:
        with caller_stream(g):
            both_snapshots_full(g, DOCS[:FIRST_A])
            assert g.delete_documents([DOCS[i][0] for i in dead]) == len(dead)
            route_commit(g, len(texts), 0, len(texts), full=True)
            sweep(g, expected(texts))
            rd = g.reader()                                       # held across the compaction: it keeps the old text
            before = texts
            assert g.compact()["bytes_reclaimed"] > 0
            assert [rd.doc_text(d) for d in sample] == [before[d] for d in sample]
            for _ in range(2):
                route_commit(g, len(texts), 0, len(texts), full=True)
                sweep(g, expected(texts))
            add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
            texts = texts + BASE[FIRST_A:FIRST_A + APPEND_A]
            assert len(texts) - APPEND_A > BLOCK
            for _ in range(2):
                route_commit(g, len(texts), 1, APPEND_A)
                sweep(g, expected(texts))
            tail = list(range(len(before), len(texts), 7))
            assert [g.doc_text(d) for d in sample + tail] == [texts[d] for d in sample + tail]
            assert rd.num_docs == len(before)
            assert [rd.doc_text(d) for d in sample] == [before[d] for d in sample]
            sweep(rd, expected(before))
    finally:
        if rd is not None:
            rd.close()
        g.close()


# g. concurrent searches on one shared stream -----------------------------------------------------------

def test_four_threads_share_the_caller_stream():
    exp = expected(A1)
    per = [exp.route_ids] * len(RR.TEXT_QUERIES)
    g = ShardIndex()
    try:
        with caller_stream(g):
            add(g, DOCS[:len(A1)])
            g.commit()

            def work():
                singles = [hit_bits(g.search(RR.QUERIES[i % len(RR.QUERIES)], 10)) for i in range(50)]
                batch = [hit_bits(h) for h in g.search_batch_all(RR.QUERIES)]
                return singles, batch, g.snippets_batch(RR.TEXT_QUERIES, per, RR.WIDTH)

            alone = work()                                        # single-threaded, and against the references
            assert alone[0] == [exp.want["search", RR.QUERIES[i % len(RR.QUERIES)], 10] for i in range(50)]
            assert alone[1] == [exp.want["search", q, 0] for q in RR.QUERIES]
            assert alone[2] == [exp.want["snippets", q] for q in RR.TEXT_QUERIES]
            results, errors = [None] * 4, []

            def run(i):
                try:
                    results[i] = work()
                except BaseException as e:                        # (reported below, in the test's thread)
                    errors.append(e)

            threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            for r in results:
                assert r == alone
    finally:
        g.close()


# h. the NULL stream ---------------------------------------------------------------------------------------

def test_null_stream_is_the_legacy_default_stream_for_writers():
    docs = keyed(BASE[:SMALL])
    extra = keyed(BASE[SMALL:SMALL + SMALL_APPEND], SMALL)
    g = ShardIndex()
    try:
        L.check(L.load().tfidf_set_stream(g._h, None))            # NULL (the wrapper's None is TFIDF_OWN_STREAM)
        add(g, docs)
        commit_and_expect(g, docs, SMALL, True)
        scorer_sweep(g, expected([t for _, t in docs]))
        g.commit()
        add(g, extra)
        docs = docs + extra
        commit_and_expect(g, docs, SMALL_APPEND, False)
        exp = expected([t for _, t in docs])
        scorer_sweep(g, exp)
        with g.reader() as rd:
            for q, got in zip(RR.QUERIES, rd.search_batch_all(RR.QUERIES)):
                assert hit_bits(got) == exp.want["search", q, 0], q
        g.set_stream(None)
        scorer_sweep(g, exp)
    finally:
        g.set_stream(None)
        g.close()
