"""Wildcard search over a node (tfidf_node_wildcard_terms_batch,
tfidf_node_search_wildcard_batch): the dense corpus of fuzzy_ref.py over two
and three shards of one device, some terms on several shards and some on one,
in both statistics modes.  The result is wildcard_ref over the concatenated
corpus in one oracle index: df summed over the shards, distinct n_matched,
global doc ids."""
import functools

import pytest

import wildcard_ref as W
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

pytestmark = pytest.mark.gpu

# two terms that tie on df over the node but on no shard: 3 + 1 and 1 + 3 documents
TIE_A, TIE_B = b"kkkx", b"kkky"
PATTERNS = [b"*", b"a*", b"*c", b"a?c*", b"kkk?", b"kkk*", b"caf?", b"zqxjkvwypmnbghtrd*", W.LONG255[:40] + b"*", b"",
            b"\xff*", b"nothing*", b"?", b"abcab", b"x"]


@functools.lru_cache(maxsize=None)
def shard_texts(n_shards):
    texts = W.dense_texts()
    sh = [[t for i, t in enumerate(texts) if i % n_shards == g] for g in range(n_shards)]
    sh[0] += [TIE_A] * 3 + [TIE_B]
    sh[-1] += [TIE_A] + [TIE_B] * 3
    return sh


@functools.lru_cache(maxsize=None)
def union(n_shards):
    allt = [t for s in shard_texts(n_shards) for t in s]
    ix = W.oracle_index(allt)
    out = ix.vocab(), W.doc_term_sets(ix, len(allt))
    ix.close()
    return out


def check(n, n_shards):
    vocab, sets = union(n_shards)
    for k in (1, 5, 1024):
        got = n.wildcard_terms_batch(PATTERNS, k)
        assert len(got) == len(PATTERNS)
        for p, gt in zip(PATTERNS, got):
            assert gt == W.expected_terms(vocab, p, k), (p[:40], k)
    got = n.search_wildcard_batch(PATTERNS)
    for p, gd in zip(PATTERNS, got):
        assert gd == W.expected_docs(sets, vocab, p), p[:40]
    assert n.wildcard_terms_batch([b"kkk?"], 5)[0] == ([(TIE_A, 4), (TIE_B, 4)], 2)
    assert n.wildcard_terms_batch([b"kkk?"], 1)[0] == ([(TIE_A, 4)], 2)     # max_out applies to the merged list
    assert n.wildcard_terms_batch([]) == [] == n.search_wildcard_batch([])


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
@pytest.mark.parametrize("n_shards", [2, 3])
def test_node_equals_the_reference_over_the_concatenated_corpus(mode, n_shards):
    sh = shard_texts(n_shards)
    per = [W.oracle_vocab(s) for s in sh]
    vocab, sets = union(n_shards)
    # the fixture: terms on one shard only and on several, df summed; the global tie is no tie on a shard
    assert len(set(per[0]) - set(per[1])) > 10 and len(set(per[0]) & set(per[1])) > 100
    assert all(vocab[t] == sum(p.get(t, 0) for p in per) for t in vocab)
    assert vocab[TIE_A] == vocab[TIE_B] == 4 and per[0][TIE_A] != per[0][TIE_B]
    assert W.expected_docs(sets, vocab, b"*")[0] == list(range(sum(len(s) for s in sh)))
    n = D.Node(devices=[0] * n_shards, stats_mode=mode, vocab_capacity_log2=16)
    for g, s in enumerate(sh):
        n.add_documents(s, [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    check(n, n_shards)
    with pytest.raises(L.TfidfError) as ei:
        n.wildcard_terms_batch([b"a*"], 0)
    assert ei.value.code == L.E_INVALID_ARG
    n.close()


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_an_empty_shard(mode):
    sh = shard_texts(2)
    n = D.Node(devices=[0, 0, 0], stats_mode=mode, vocab_capacity_log2=16)
    n.add_documents(sh[0], [b"s0_%05d" % i for i in range(len(sh[0]))], shard=0)
    n.add_documents(sh[1], [b"s2_%05d" % i for i in range(len(sh[1]))], shard=2)
    n.commit()
    check(n, 2)                                                             # shard 1 has no documents
    n.close()


def test_node_calls_before_commit_are_state_errors():
    n = D.Node(devices=[0, 0], vocab_capacity_log2=12)
    n.add_documents([b"abc", b"abd"])
    for call in (lambda: n.wildcard_terms_batch([b"ab*"]), lambda: n.search_wildcard_batch([b"ab*"])):
        with pytest.raises(L.TfidfError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    n.close()
