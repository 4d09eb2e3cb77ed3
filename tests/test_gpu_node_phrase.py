"""Exact phrase search over a node (tfidf_node_search_phrase_batch): the
corpora of phrase_ref.py dealt over three shards of one device, in both
statistics modes.  GLOBAL: one PhraseRef (one OracleIndex) over all documents in
global id order.  SHARD: one PhraseRef per shard, the lists merged by (score
descending, global id ascending).  Compared exactly: ids, order, freq and
float32 score bits."""
import pytest

import phrase_ref as P
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

pytestmark = pytest.mark.gpu

PHRASES = [P.NO_WORK[0]] + P.PHRASES + [P.NO_WORK[3], P.PHRASES[0], P.NO_WORK[2]]


def expected(shards, mode):
    if mode == L.STATS_GLOBAL:
        r = P.PhraseRef([t for s in shards for t in s])
        out = [P.exact(r.search(p)) for p in PHRASES]
        r.close()
        return out
    refs = [P.PhraseRef(s) if s else None for s in shards]
    bases = [sum(len(s) for s in shards[:g]) for g in range(len(shards))]
    out = [P.exact(P.merge([(r.search(p), b) for r, b in zip(refs, bases) if r])) for p in PHRASES]
    for r in refs:
        if r:
            r.close()
    return out


def node_of(shards, mode):
    n = D.Node(devices=[0] * len(shards), stats_mode=mode, inproc=True)
    for g, s in enumerate(shards):
        if s:
            n.add_documents(list(s), [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    return n


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_node_phrase_hits_are_the_merged_shard_hits(mode):
    shards = [P.TEXTS[g::3] for g in range(3)]
    want = expected(shards, mode)
    n = node_of(shards, mode)
    assert n.stats()["num_docs"] == len(P.TEXTS)
    got = [P.exact(h) for h in n.search_phrase_batch(PHRASES)]
    assert len(got) == len(PHRASES)
    for p, g, w in zip(PHRASES, got, want):
        assert g == w, p[:24]
    # the fixture: one phrase's hits lie on all shards, another's on one
    bases = [0, len(shards[0]), len(shards[0]) + len(shards[1])]
    by = dict(zip(PHRASES, got))
    shard_of = lambda d: max(g for g in range(3) if bases[g] <= d)          # noqa: E731
    assert {shard_of(d) for d, _, _ in by[b"alpha beta"]} == {0, 1, 2}
    assert len({shard_of(d) for d, _, _ in by["月星".encode()]}) == 1 and by["月星".encode()][0][2] == 1366
    assert by[P.NO_WORK[0]] == by[P.NO_WORK[2]] == by[P.NO_WORK[3]] == []
    assert n.search_phrase_batch([]) == []
    with pytest.raises(L.TfidfError) as e:
        n.search_phrase_batch([b"alpha", P.PHRASE_1025])
    assert e.value.code == L.E_INVALID_ARG
    n.close()


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_node_with_an_empty_shard(mode):
    cut = P.doc("ops", 2)
    shards = [P.TEXTS[:cut], [], P.TEXTS[cut:]]
    want = expected(shards, mode)
    n = node_of(shards, mode)
    got = [P.exact(h) for h in n.search_phrase_batch(PHRASES)]
    for p, g, w in zip(PHRASES, got, want):
        assert g == w, p[:24]
    assert any(d >= cut for d, _, _ in got[PHRASES.index(b"alpha beta")])
    n.close()


def test_node_phrase_search_before_commit_is_a_state_error():
    n = D.Node(devices=[0, 0], inproc=True)
    n.add_documents([b"alpha beta", b"beta alpha"])
    with pytest.raises(L.TfidfError) as e:
        n.search_phrase_batch([b"alpha beta"])
    assert e.value.code == L.E_STATE
    n.close()
