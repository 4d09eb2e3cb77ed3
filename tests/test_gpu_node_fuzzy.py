"""Fuzzy term lookup over a node (tfidf_node_fuzzy_terms_batch): the dense
corpus of fuzzy_ref.py over two shards of one device, some terms on both
shards and some on one.  The result is fuzzy_ref.expected over the union
vocabulary with the df summed over the shards: the oracle's vocabulary of all
documents in one index."""
import functools

import pytest

import fuzzy_ref as F
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

pytestmark = pytest.mark.gpu

# two terms that tie on (dist, df) over the node but on neither shard: 3 + 1 and 1 + 3 documents
TIE_A, TIE_B = b"kkkx", b"kkky"


def shard_texts():
    texts = F.dense_texts()
    sh = [[t for i, t in enumerate(texts) if i % 3 != 2], [t for i, t in enumerate(texts) if i % 3 == 2]]
    sh[0] += [TIE_A] * 3 + [TIE_B]
    sh[1] += [TIE_A] + [TIE_B] * 3
    return sh


@functools.lru_cache(maxsize=None)
def union_vocab():
    sh = shard_texts()
    return F.oracle_vocab(sh[0] + sh[1])


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_node_lookup_equals_the_reference_over_the_union(mode):
    sh = shard_texts()
    per = [F.oracle_vocab(s) for s in sh]
    vocab = union_vocab()
    # the fixture: terms on one shard only and on both, df summed; the global tie is no tie on a shard
    only = [set(per[0]) - set(per[1]), set(per[1]) - set(per[0])]
    assert len(only[0]) > 100 and len(only[1]) > 10 and len(set(per[0]) & set(per[1])) > 100
    assert all(vocab[t] == per[0].get(t, 0) + per[1].get(t, 0) for t in vocab)
    assert vocab[TIE_A] == vocab[TIE_B] == 4 and per[0][TIE_A] != per[0][TIE_B] and per[1][TIE_A] != per[1][TIE_B]
    n = D.Node(devices=[0, 0], stats_mode=mode, vocab_capacity_log2=16)
    for g, s in enumerate(sh):
        n.add_documents(s, [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    terms = F.dense_terms() + [b"kkkz", TIE_A, b"kkk"]
    for e, p, k in ((2, 0, 5), (1, 1, 1024), (2, 3, 1), (0, 0, 5), (2, 0, 1024)):
        got = n.fuzzy_terms_batch(terms, e, p, k)
        assert len(got) == len(terms)
        for t, gt in zip(terms, got):
            assert gt == F.expected(vocab, t, e, p, k), (t[:40], e, p, k)
    tie = n.fuzzy_terms_batch([b"kkkz"], 1, 0, 5)[0]
    assert tie == ([(TIE_A, 4, 1), (TIE_B, 4, 1)], 2)
    # max_out applies to the merged list: the one winner over the node
    assert n.fuzzy_terms_batch([b"kkkz"], 1, 0, 1)[0] == ([(TIE_A, 4, 1)], 2)
    with pytest.raises(L.TfidfError) as ei:
        n.fuzzy_terms_batch([b"a"], 3)
    assert ei.value.code == L.E_INVALID_ARG
    n.close()


def test_node_lookup_before_commit_is_a_state_error():
    n = D.Node(devices=[0, 0], vocab_capacity_log2=12)
    n.add_documents([b"abc", b"abd"])
    with pytest.raises(L.TfidfError) as ei:
        n.fuzzy_terms_batch([b"abc"])
    assert ei.value.code == L.E_STATE
    n.close()
