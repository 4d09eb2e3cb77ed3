"""Node-level all-hits batches: tfidf_node_search_batch_all /
tfidf_dist_search_batch_all (GLOBAL statistics: every hit of every query over
the shards, merged by k_merge_segments) and tfidf_node_search_names_batch /
tfidf_dist_shard_search_batch (SHARD statistics: the Leader merge by name of
every query) against the C oracle.  Bar: doc ids and float32 score bits
identical, double sums exactly equal.

Corpora, the smallest at which each structure can go wrong:
  A  multirank.corpus(): 1 200 documents, one block per shard; 18 queries, the
     last two do not parse
  B  20 000 short documents: 2 shards of 2 blocks (the local run merges feed
     the cross-rank merge) or 3 of one; empty results first, in the middle, last
  C  hand-routed 3 shards: equal scores across ranks (ordered by global doc
     id), (rank, query) segments empty at the first and at the last ranks
Collective calls over Comm.inproc run on one thread per rank under a join
timeout (nodebatch.run_ranks).
"""
import ctypes as C

import numpy as np
import pytest

import multirank as M
import nodebatch as NB
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex
from test_gpu_batch_all import BATCH
from test_gpu_parity import assert_hits_equal

pytestmark = pytest.mark.gpu

B_COUNTS = [0, 11250, 14075, 671, 0, 2883, 7271, 54, 0, 15365, 671, 27, 133, 0]
B_TOTAL = 52400
B_SHARED = [3176, 4955, 11, 197, 1340, 0, 5900, 11, 0, 1]   # names summing two shards' scores, non-empty queries


def same_lists(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert_hits_equal(g, w)


def same_names(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [n for n, _ in g] == [n for n, _ in w]
        assert [s for _, s in g] == [s for _, s in w]            # double sums, exactly


@pytest.fixture(scope="module")
def corpus_a():
    texts, names = M.corpus()
    return {"texts": texts, "names": names, "want": NB.oracle_global(texts, M.QUERIES)}


@pytest.fixture(scope="module")
def corpus_b():
    texts, names = NB.corpus_b()
    want = NB.oracle_global(texts, BATCH)
    assert [len(h) for h in want] == B_COUNTS and sum(B_COUNTS) == B_TOTAL
    return {"texts": texts, "names": names, "want": want}


@pytest.fixture(scope="module")
def nodes_b(corpus_b):
    """GLOBAL nodes of 2 and 3 shards over corpus B (2 blocks / 1 block per shard)."""
    nodes = {w: NB.make_node(corpus_b["texts"], corpus_b["names"], w, L.STATS_GLOBAL) for w in (2, 3)}
    yield nodes
    for n in nodes.values():
        n.close()


# ---- 1. GLOBAL, corpus A ---------------------------------------------------------

@pytest.mark.parametrize("shards", [2, 3])
def test_global_corpus_a_equals_oracle_and_single_searches(shards, corpus_a):
    n = NB.make_node(corpus_a["texts"], corpus_a["names"], shards, L.STATS_GLOBAL)
    got = n.search_batch_all(M.QUERIES)
    same_lists(got, corpus_a["want"])
    assert got[-2:] == [[], []] and all(got[:4])             # the unparsable ones give []
    assert got == [n.search(q, 0) for q in M.QUERIES]
    n.close()


# ---- 2. GLOBAL, corpus B, chunk knobs ----------------------------------------------

@pytest.mark.parametrize("shards", [2, 3])
def test_global_corpus_b_equals_oracle_in_any_chunking(shards, corpus_b, nodes_b, monkeypatch):
    n = nodes_b[shards]
    one = n.search_batch_all(BATCH)
    same_lists(one, corpus_b["want"])
    for node_chunk, local_chunk in (("3", None), ("1", None), ("3", "1")):
        monkeypatch.setenv("TFIDF_DIST_ALLHITS_CHUNK", node_chunk)
        if local_chunk:
            monkeypatch.setenv("TFIDF_ALLHITS_CHUNK", local_chunk)   # node and local chunks disagree
        assert n.search_batch_all(BATCH) == one


# ---- 3. GLOBAL, corpus C -----------------------------------------------------------

def test_global_corpus_c_ties_across_ranks_and_empty_segments():
    texts = [t for sh in NB.C_SHARDS for t in sh]
    want = NB.oracle_global(texts, NB.C_QUERIES)
    ties = [1, 2, 4, 6, 8]                                   # "tie word": shard 0 docs 1, 2; shard 1 docs 0, 2; shard 2 doc 1
    for qi in (2, 6):                                        # b"tie", b"tie word"
        assert [d for d, _ in want[qi]] == ties and len({np.float32(s) for _, s in want[qi]}) == 1
    assert [d for d, _ in want[0]] == [0] and sorted(d for d, _ in want[1]) == [7, 9] and want[5] == []
    n = D.Node(devices=[0, 0, 0], stats_mode=L.STATS_GLOBAL)
    for g, sh in enumerate(NB.C_SHARDS):
        n.add_documents(sh, [b"c%d_%d" % (g, i) for i in range(len(sh))], shard=g)
    n.commit()
    docs, scores, offs = n.search_batch_all_arrays(NB.C_QUERIES)
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(h) for h in want])]).tolist()   # exact
    same_lists(D._hit_lists(docs, scores, offs), want)
    n.close()


# ---- 4. buffer protocol ----------------------------------------------------------------

def _raw_batch_all(node, queries, cap):
    offs = D._offsets(queries)
    docs = np.zeros(max(cap, 1), np.uint64)
    scores = np.zeros(max(cap, 1), np.float32)
    ho = np.full(len(queries) + 1, 77, np.uint64)
    n = C.c_uint64(77)
    rc = L.load().tfidf_node_search_batch_all(node._h, b"".join(queries), L.ptr(offs, C.c_uint64), len(queries),
                                              L.ptr(docs, C.c_uint64), L.ptr(scores, C.c_float), cap,
                                              L.ptr(ho, C.c_uint64), C.byref(n))
    return rc, docs, scores, ho, n.value


def test_buffer_protocol(corpus_b, nodes_b):
    n = nodes_b[2]
    full_offs = np.concatenate([[0], np.cumsum(B_COUNTS)]).tolist()
    rc, _, _, ho, tot = _raw_batch_all(n, BATCH, B_TOTAL - 1)
    assert rc == L.E_BUFFER and tot == B_TOTAL and ho.tolist() == full_offs
    rc, docs, scores, ho, tot = _raw_batch_all(n, BATCH, B_TOTAL)
    assert rc == L.OK and tot == B_TOTAL and ho.tolist() == full_offs
    d1, s1, o1 = n.search_batch_all_arrays(BATCH, cap=1)      # retried once with the reported size
    assert o1.tolist() == full_offs
    assert d1.tolist() == docs[:tot].tolist() and s1.tobytes() == scores[:tot].tobytes()
    same_lists(D._hit_lists(d1, s1, o1), corpus_b["want"])
    rc, _, _, ho, tot = _raw_batch_all(n, [], 4)
    assert rc == L.OK and tot == 0 and ho.tolist() == [0]


# ---- 5. RCCL communicator, world 1 -----------------------------------------------------

def test_rccl_world1_doc_base():
    lib = L.load()
    uid = (C.c_uint8 * 128)()
    L.check(lib.tfidf_rccl_unique_id(uid))
    h = C.c_void_p()
    L.check(lib.tfidf_comm_init_rccl(uid, 0, 1, 0, C.byref(h)))
    comm = D.Comm(h)
    texts, _ = M.corpus()
    idx = ShardIndex(device=0)
    idx.add_documents(texts, [b"d%05d.txt" % i for i in range(len(texts))])
    idx.commit()
    ad = D.DistShard(idx, comm, doc_base=1000)
    ad.global_commit()
    want = idx.search_batch_all(M.QUERIES)
    assert sum(len(w) for w in want) > 1000
    got = ad.search_batch_all(M.QUERIES)
    same_lists(got, [[(d + 1000, s) for d, s in w] for w in want])
    comm.close()
    idx.close()


# ---- 6. SPMD over the in-process transport ---------------------------------------------

def test_spmd_inproc3_every_rank_gets_the_result(corpus_a):
    comms, idx, ads = NB.make_ranks(corpus_a["texts"], corpus_a["names"], 3)
    res = NB.run_ranks([lambda a=a: a.global_commit() for a in ads])
    assert [e for _, e in res] == [None] * 3
    res = NB.run_ranks([lambda a=a: a.search_batch_all(M.QUERIES) for a in ads])
    for got, e in res:
        assert e is None
        same_lists(got, corpus_a["want"])
    NB.close_ranks(comms, idx)


# ---- 7. failure semantics, GLOBAL ---------------------------------------------------------

def _code(res):
    return [e.code if isinstance(e, L.TfidfError) else ("ok" if e is None else repr(e)) for _, e in res]


def test_stale_rank_and_overlapping_ranges_fail_on_every_rank(corpus_a):
    texts, names = corpus_a["texts"], corpus_a["names"]
    comms, idx, ads = NB.make_ranks(texts, names, 2)
    NB.run_ranks([lambda a=a: a.global_commit() for a in ads])
    idx[1].commit()                                          # rank 1: local statistics again
    res = NB.run_ranks([lambda a=a: a.search_batch_all(M.QUERIES) for a in ads])
    assert _code(res) == [L.E_STATE, L.E_STATE], res
    res = NB.run_ranks([lambda a=a: a.global_commit() for a in ads])
    assert _code(res) == ["ok", "ok"]
    res = NB.run_ranks([lambda a=a: a.search_batch_all(M.QUERIES) for a in ads])   # serving again
    assert _code(res) == ["ok", "ok"]
    for got, _ in res:
        same_lists(got, corpus_a["want"])
    NB.close_ranks(comms, idx)
    comms, idx, ads = NB.make_ranks(texts, names, 2, bases=[0, 0])
    NB.run_ranks([lambda a=a: a.global_commit() for a in ads])
    res = NB.run_ranks([lambda a=a: a.search_batch_all(M.QUERIES) for a in ads])
    assert _code(res) == [L.E_INVALID_ARG, L.E_INVALID_ARG], res
    NB.close_ranks(comms, idx)


# ---- 8. a rank fails inside the batch --------------------------------------------------------

def test_mid_batch_failure_fails_every_rank_together(corpus_a, monkeypatch):
    """An injected host-level error code of the scoring call (no device fault):
    every fourth scoring call fails after its kernels are queued.  One query
    per node chunk, 8 queries with hits on both ranks: >= 16 scoring calls, so
    at least two are hit whatever the counter's state."""
    texts, names = corpus_a["texts"], corpus_a["names"]
    queries = [synth.word(r) for r in range(1, 9)]
    want = NB.oracle_global(texts, queries)
    lo, hi = D.shard_range(len(texts), 1, 2)
    for q, w in zip(queries, want):                           # hits on both ranks: both score every query
        assert any(d < lo for d, _ in w) and any(d >= lo for d, _ in w)
    comms, idx, ads = NB.make_ranks(texts, names, 2)
    NB.run_ranks([lambda a=a: a.global_commit() for a in ads])
    monkeypatch.setenv("TFIDF_DIST_ALLHITS_CHUNK", "1")
    monkeypatch.setenv("TFIDF_TEST_FAIL_SCORING", "4")
    res = NB.run_ranks([lambda a=a: a.search_batch_all(queries) for a in ads])
    assert _code(res) == [L.E_HIP, L.E_HIP], res
    monkeypatch.delenv("TFIDF_TEST_FAIL_SCORING")
    res = NB.run_ranks([lambda a=a: a.search_batch_all(queries) for a in ads])
    assert _code(res) == ["ok", "ok"], res
    for got, _ in res:
        same_lists(got, want)
    NB.close_ranks(comms, idx)


# ---- 9. SHARD ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [2, 3])
def test_shard_corpus_a_equals_leader_merge(shards, corpus_a, monkeypatch):
    n = NB.make_node(corpus_a["texts"], corpus_a["names"], shards, L.STATS_SHARD)
    want = M.expected_shard(shards)
    one = n.search_names_batch(M.QUERIES)
    same_names(one, want)
    assert one == [n.search_names(q) for q in M.QUERIES]
    for chunk in ("3", "1"):
        monkeypatch.setenv("TFIDF_DIST_ALLHITS_CHUNK", chunk)
        assert n.search_names_batch(M.QUERIES) == one
    n.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_shard_corpus_b_equals_leader_merge(shards, corpus_b, monkeypatch):
    texts, names = corpus_b["texts"], corpus_b["names"]
    want, shared = NB.oracle_shard(texts, names, shards, BATCH)
    assert [s for s, c in zip(shared, B_COUNTS) if c] == B_SHARED      # names that sum two shards' scores
    n = NB.make_node(texts, names, shards, L.STATS_SHARD)
    one = n.search_names_batch(BATCH)
    same_names(one, want)
    assert one == [n.search_names(q) for q in BATCH]
    for chunk in ("3", "1"):
        monkeypatch.setenv("TFIDF_DIST_ALLHITS_CHUNK", chunk)
        assert n.search_names_batch(BATCH) == one
    n.close()


# ---- 10. SHARD, a stale shard ---------------------------------------------------------------

def test_shard_batch_skips_a_recommitted_shard(corpus_a):
    n = NB.make_node(corpus_a["texts"], corpus_a["names"], 3, L.STATS_SHARD)
    L.check(L.load().tfidf_commit(n.shard(1)))
    same_names(n.search_names_batch(M.QUERIES), M.expected_shard(3, skip=(1,)))
    assert n.last_failed() == 0b10
    n.commit()
    same_names(n.search_names_batch(M.QUERIES), M.expected_shard(3))
    assert n.last_failed() == 0
    n.close()


# ---- 11. Leader.start_batch ------------------------------------------------------------------

def test_leader_start_batch_over_a_node(lucene_fixture):
    from tfidf_amd.reference_api import Leader, Worker
    docs = lucene_fixture["docs"]
    texts = [d["text"].encode() for d in docs]
    keys = [d["name"].encode() for d in docs]
    node = NB.make_node(texts, keys, 2, L.STATS_SHARD)
    workers = []
    for r in range(2):
        lo, hi = D.shard_range(len(docs), r, 2)
        w = Worker()
        w.index.add_documents(texts[lo:hi], keys[lo:hi])
        w.commit()
        workers.append(w)
    leader = Leader(workers, node=node)
    qs = ["fast food", "AND", "the quick", docs[0]["text"].split()[0], "zzzzqq"]
    want = [leader.start(q) for q in qs]
    assert want[1] == {} and any(want)
    got = leader.start_batch(qs)
    assert got == want and [list(g) for g in got] == [list(w) for w in want]
    assert Leader(workers).start_batch(qs) == want           # no node: the plain loop
    for w in workers:
        w.close()
    node.close()
