"""Node-level delete and compact (tfidf_node_delete_docs / tfidf_node_compact):
two shards on cuda:0 over the in-process transport, in both statistics modes,
against the oracle construction of test_gpu_node.py (tests/multirank.py) built
over the surviving documents."""
import ctypes as C

import numpy as np
import pytest

import multirank as M
from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

pytestmark = pytest.mark.gpu

SHARDS = 2
# M.corpus(): shard 0 holds f00000 .. f00599, shard 1 f00600 .. f00699 and f00000 .. f00499
ON_BOTH = [b"f00010.txt", b"f00020.txt"]
ONLY_1 = [b"f00650.txt"]
ONLY_0 = [b"f00550.txt"]
SHARD0_ONLY_CALL = [b"f00030.txt"]           # on both shards, deleted on shard 0 alone


def survivors():
    """Per shard: (names, texts) after the deletes of delete_and_commit()."""
    texts, names = M.corpus()
    everywhere = set(ON_BOTH + ONLY_1 + ONLY_0)
    out = []
    for r in range(SHARDS):
        lo, hi = D.shard_range(M.N_DOCS, r, SHARDS)
        gone = everywhere | (set(SHARD0_ONLY_CALL) if r == 0 else set())
        keep = [i for i in range(lo, hi) if names[i] not in gone]
        out.append(([names[i] for i in keep], [texts[i] for i in keep]))
    return out


def delete_and_commit(n):
    assert n.delete_documents(ON_BOTH + ONLY_1 + ONLY_0 + [b"nope.txt"] + ON_BOTH[:1]) == 6   # summed over the shards
    assert n.delete_documents(SHARD0_ONLY_CALL, shard=0) == 1
    assert n.delete_documents(SHARD0_ONLY_CALL, shard=0) == 0
    with pytest.raises(L.TfidfError):
        n.delete_documents(ON_BOTH, shard=SHARDS)
    texts, names = M.corpus()
    gone0 = [i for i in range(600) if names[i] in set(ON_BOTH + ONLY_0 + SHARD0_ONLY_CALL)]
    gone1 = [i for i in range(600, M.N_DOCS) if names[i] in set(ON_BOTH + ONLY_1)]
    assert n.compact() == sum(len(texts[i]) for i in gone0 + gone1)
    assert n.compact() == 0


def shard_stats(n, g):
    """tfidf_stats of shard g (the handle stays the node's)."""
    s = L.IndexStats()
    L.check(L.load().tfidf_stats(n.shard(g), C.byref(s)))
    return {f: getattr(s, f) for f, _ in L.IndexStats._fields_}


def search(o, q, k):
    try:
        return o.search(q, k)
    except O.QuerySyntaxError:
        return []


def f32(hits):
    return [(d, np.float32(s)) for d, s in hits]


def test_node_global_delete_compact_commit():
    texts, names = M.corpus()
    n = D.Node(devices=[0] * SHARDS, stats_mode=L.STATS_GLOBAL)
    n.add_documents(texts, names)
    n.commit()
    before = [n.search(q, M.K) for q in M.QUERIES]
    delete_and_commit(n)
    # staged only: the node serves its last commit until the next one
    assert [n.search(q, M.K) for q in M.QUERIES] == before
    assert n.stats()["num_docs"] == M.N_DOCS
    n.commit()
    surv = survivors()
    one = O.OracleIndex()
    flat_names = []
    for nm, tx in surv:
        for k, t in zip(nm, tx):
            one.add_doc(b"%d" % len(flat_names), t)
            flat_names.append(k)
    one.commit()
    st = n.stats()
    assert (st["num_docs"], st["doc_count"], st["sum_ttf"], st["num_terms"]) == \
        (len(flat_names), one.doc_count, one.sum_ttf, one.num_terms)
    assert st["num_docs"] == M.N_DOCS - 7
    bd, bs, bc = n.search_batch(M.QUERIES, M.K)
    for i, q in enumerate(M.QUERIES):
        want = f32(search(one, q, M.K))
        assert f32(n.search(q, M.K)) == want
        assert f32(zip(bd[i, :bc[i]].tolist(), bs[i, :bc[i]].tolist())) == want
    for q in M.QUERIES[:6]:
        assert f32(n.search(q, 0)) == f32(search(one, q, 0))
    hits = n.search_batch_all(M.QUERIES[:6])
    assert [f32(h) for h in hits] == [f32(search(one, q, 0)) for q in M.QUERIES[:6]]
    for d in (0, 9, 10, len(surv[0][0]) - 1, len(surv[0][0]), len(flat_names) - 1):
        assert n.doc_key(d) == flat_names[d]
    for g in range(SHARDS):
        s = shard_stats(n, g)
        assert (s["dead_docs"], s["dead_bytes"], s["compactions"]) == (0, 0, 1)
        assert s["text_bytes"] == sum(len(t) for t in surv[g][1])
    one.close()
    n.close()


def test_node_shard_mode_delete_compact_commit():
    texts, names = M.corpus()
    n = D.Node(devices=[0] * SHARDS, stats_mode=L.STATS_SHARD)
    n.add_documents(texts, names)
    n.commit()
    before = [n.search_names(q) for q in M.QUERIES[:4]]
    delete_and_commit(n)
    assert [n.search_names(q) for q in M.QUERIES[:4]] == before
    n.commit()
    workers = []
    for nm, tx in survivors():
        o = O.OracleIndex()
        for k, t in zip(nm, tx):
            o.add_doc(k, t)
        o.commit()
        workers.append(o)
    for q in M.QUERIES:
        resp = [[(o.doc_key(d), float(s)) for d, s in search(o, q, 0)] for o in workers]
        want = O.leader_merge(resp)
        got = n.search_names(q)
        assert [nm for nm, _ in got] == [nm for nm, _ in want]
        assert [s for _, s in got] == [s for _, s in want]               # double sums, exactly
    # f00030 was deleted on shard 0 alone: shard 1's copy still answers
    assert n.delete_documents(SHARD0_ONLY_CALL, shard=0) == 0
    assert n.delete_documents(SHARD0_ONLY_CALL, shard=1) == 1
    for o in workers:
        o.close()
    n.close()
