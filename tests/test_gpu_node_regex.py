"""Regular-expression search over a node (tfidf_node_regex_terms_batch,
tfidf_node_search_regex_batch): the dense corpus of fuzzy_ref.py over two and
three shards of one device, some terms on several shards and some on one, in
both statistics modes (the shards of test_gpu_node_wildcard.py).  The result is
regex_ref over the concatenated corpus in one oracle index: df summed over the
shards, distinct n_matched, global doc ids."""
import pytest

import regex_ref as R
import test_gpu_node_wildcard as NW
import wildcard_ref as W
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

pytestmark = pytest.mark.gpu

TIE_A, TIE_B = NW.TIE_A, NW.TIE_B
PATTERNS = [b".*", b"a.*", b".*c", b"a.c.*", b"kkk.", b"kkk[xy]?", b"caf.", b"zqxjkvwypmnbghtrd.*", W.LONG255[:40] + b".*",
            b"", b"\xff.*", b"nothing.*", b".", b"abcab", b"x", b"[ab]{2,3}", b"~(a.*)&[a-c]{1,2}", b"(a|b)*a(a|b){7}", b"#"]


def check(n, n_shards):
    vocab, sets = NW.union(n_shards)
    for k in (1, 5, 1024):
        got = n.regex_terms_batch(PATTERNS, k)
        assert len(got) == len(PATTERNS)
        for p, gt in zip(PATTERNS, got):
            assert gt == R.expected_terms(vocab, p, k), (p[:40], k)
    got = n.search_regex_batch(PATTERNS)
    for p, gd in zip(PATTERNS, got):
        assert gd == R.expected_docs(sets, vocab, p), p[:40]
    assert n.regex_terms_batch([b"kkk."], 5)[0] == ([(TIE_A, 4), (TIE_B, 4)], 2)
    assert n.regex_terms_batch([b"kkk."], 1)[0] == ([(TIE_A, 4)], 2)        # max_out applies to the merged list
    assert n.regex_terms_batch([]) == [] == n.search_regex_batch([])
    # a pattern in error fails the node call with its status
    for bad, code in ((b"a|", L.E_QUERY_SYNTAX), (b"<x>", L.E_UNSUPPORTED_QUERY)):
        for call in (lambda: n.regex_terms_batch([b"a.*", bad]), lambda: n.search_regex_batch([bad, b"a.*"])):
            with pytest.raises(L.TfidfError) as ei:
                call()
            assert ei.value.code == code


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
@pytest.mark.parametrize("n_shards", [2, 3])
def test_node_equals_the_reference_over_the_concatenated_corpus(mode, n_shards):
    sh = NW.shard_texts(n_shards)
    vocab, sets = NW.union(n_shards)
    assert vocab[TIE_A] == vocab[TIE_B] == 4
    assert R.expected_docs(sets, vocab, b".*")[0] == list(range(sum(len(s) for s in sh)))
    n = D.Node(devices=[0] * n_shards, stats_mode=mode, vocab_capacity_log2=16)
    for g, s in enumerate(sh):
        n.add_documents(s, [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    check(n, n_shards)
    with pytest.raises(L.TfidfError) as ei:
        n.regex_terms_batch([b"a.*"], 0)
    assert ei.value.code == L.E_INVALID_ARG
    n.close()


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_an_empty_shard(mode):
    sh = NW.shard_texts(2)
    n = D.Node(devices=[0, 0, 0], stats_mode=mode, vocab_capacity_log2=16)
    n.add_documents(sh[0], [b"s0_%05d" % i for i in range(len(sh[0]))], shard=0)
    n.add_documents(sh[1], [b"s2_%05d" % i for i in range(len(sh[1]))], shard=2)
    n.commit()
    check(n, 2)                                                             # shard 1 has no documents
    n.close()


def test_node_calls_before_commit_are_state_errors():
    n = D.Node(devices=[0, 0], vocab_capacity_log2=12)
    n.add_documents([b"abc", b"abd"])
    for call in (lambda: n.regex_terms_batch([b"ab.*"]), lambda: n.search_regex_batch([b"ab.*"])):
        with pytest.raises(L.TfidfError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    n.close()
