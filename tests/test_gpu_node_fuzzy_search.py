"""Fuzzy search over a node (tfidf_node_search_fuzzy_batch): the fixture corpus
of fuzzy_search_ref.py dealt over the shards of one device list, in both
statistics modes.  Every shard expands over its own vocabulary; the weights use
the df and docCount of the statistics in force (SHARD: the shard's own; GLOBAL:
those of all documents); the lists are merged by (score descending, global id
ascending).  Compared exactly: ids, order and float32 score bits."""
import numpy as np
import pytest

import fuzzy_ref as F
import fuzzy_search_ref as R
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D
from tfidf_amd.engine import ShardIndex

pytestmark = pytest.mark.gpu

TERMS = [R.WORD_D, R.MISSPELT_D[0], b"kangaru", R.FAMILY_A[0], R.FAMILY_B[40], b"qqxqq", b"abc", b"a", b"ABCA",
         F.CAFES[1], b"", b"\xff\xfe", b"zzzzzzzzzzzz", R.WORD_D]
PARAMS = [(2, 0, 50), (1, 1, 5), (2, 0, 64)]


def deal(n_shards):
    """Contiguous shards."""
    texts = R.texts()
    return [texts[slice(*D.shard_range(len(texts), g, n_shards))] for g in range(n_shards)]


def expected(shards, mode, e, p, k):
    refs = [R.Shard(s) for s in shards]
    stats = {}
    if mode == L.STATS_GLOBAL:
        df = {}
        for r in refs:
            for t, v in r.vocab.items():
                df[t] = df.get(t, 0) + v
        stats = dict(df_of=df, doc_count=sum(r.doc_count for r in refs), sum_ttf=sum(r.sum_ttf for r in refs))
    out, n_exp = [], []
    for t in TERMS:
        merged, n = [], 0
        base = 0
        for r in refs:
            exp, _ = R.expansion(r.vocab, t, e, p, k)
            n += len(exp)
            merged += [(d + base, s) for d, s in R.hits(R.clause_scores(r, exp, **stats))]
            base += r.n
        merged.sort(key=lambda h: (-float(h[1]), h[0]))
        out.append(R.bits(merged))
        n_exp.append(n)
    return out, n_exp


def node_of(n_shards, mode):
    n = D.Node(devices=[0] * n_shards, stats_mode=mode, vocab_capacity_log2=16)
    for g, s in enumerate(deal(n_shards)):
        n.add_documents(s, [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    return n


@pytest.mark.parametrize("mode", [L.STATS_SHARD, L.STATS_GLOBAL])
def test_node_hits_are_the_merged_shard_hits(mode):
    shards = deal(2)
    n = node_of(2, mode)
    assert n.stats()["num_docs"] == sum(len(s) for s in shards)
    for e, p, k in PARAMS:
        want, want_n = expected(shards, mode, e, p, k)
        docs, scores, offs, n_exp, _ = n.search_fuzzy_batch_arrays(TERMS, e, p, k)
        o = offs.tolist()
        for i, t in enumerate(TERMS):
            got = list(zip(docs[o[i]:o[i + 1]].tolist(), scores[o[i]:o[i + 1]].view(np.int32).tolist()))
            assert got == want[i], (t[:40], e, p, k)
        assert n_exp.tolist() == want_n
        if (e, p, k) == (2, 0, 50):
            # the fixture: b"ABCA" expands to 50 terms on each shard and its hits lie on both; the families lie on the second
            cut = len(shards[0])
            abca = [d for d, _ in want[TERMS.index(b"ABCA")]]
            assert any(d < cut for d in abca) and any(d >= cut for d in abca) and want_n[TERMS.index(b"ABCA")] == 100
            assert all(d >= cut for d, _ in want[0]) and want[3] and want[4] and want[10] == want[12] == []
    assert n.search_fuzzy_batch([]) == []
    with pytest.raises(L.TfidfError) as ei:
        n.search_fuzzy_batch([b"a"], 2, 0, 65)
    assert ei.value.code == L.E_INVALID_ARG
    n.close()


def test_one_global_shard_is_the_single_index():
    texts = R.texts()
    n = node_of(1, L.STATS_GLOBAL)
    g = ShardIndex(vocab_capacity_log2=16)
    g.add_documents(texts, [b"d%05d" % i for i in range(len(texts))])
    g.commit()
    a = n.search_fuzzy_batch_arrays(TERMS, 2, 0, 50)
    b = g.search_fuzzy_batch_arrays(TERMS, 2, 0, 50)
    assert a[0].tolist() == b[0].tolist() and a[1].view(np.int32).tolist() == b[1].view(np.int32).tolist()
    assert a[2].tolist() == b[2].tolist() and a[3].tolist() == b[3].tolist() and len(a[0]) > 100
    want, _ = expected([texts], L.STATS_GLOBAL, 2, 0, 50)
    o = a[2].tolist()
    for i in range(len(TERMS)):
        assert list(zip(a[0][o[i]:o[i + 1]].tolist(), a[1][o[i]:o[i + 1]].view(np.int32).tolist())) == want[i]
    g.close()
    n.close()


def test_node_fuzzy_search_before_commit_is_a_state_error():
    n = D.Node(devices=[0, 0], vocab_capacity_log2=12)
    n.add_documents([b"alpha beta", b"beta alpha"])
    with pytest.raises(L.TfidfError) as e:
        n.search_fuzzy_batch([b"alpha"])
    assert e.value.code == L.E_STATE
    n.close()
