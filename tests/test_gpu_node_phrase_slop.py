"""Sloppy phrase search over a node (tfidf_node_search_phrase_slop_batch):
phrase_slop_ref's documents dealt over two shards of one device over the
in-process transport, in both statistics modes.  Each shard has its own
PhraseRef: on its own statistics (SHARD) or on the statistics of all documents
given as global_stats (GLOBAL); the shards' lists are merged by (score
descending, global id ascending).  Compared exactly: ids, order, float32
frequency bits and float32 score bits."""
import pytest

import phrase_ref as P
import phrase_slop_ref as S
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

pytestmark = pytest.mark.gpu

BATCH = ([(S.NO_WORK[0], 1)] + [(p, s) for _, p, s, _, _ in S.STATED] +
         [(b"alpha beta", 2), (b"beta alpha", 2), (b"alpha beta", 0), (b"b x a", 3), (b"a b", 1), (S.M64, 5),
          (b"beta beta", 0), (b"alpha", 4), (S.NO_WORK[3], 2), (b"lambda alpha", 1), (S.NO_WORK[2], 3)])


def expected(shards, mode):
    stats = None
    if mode == L.STATS_GLOBAL:
        whole = P.PhraseRef([t for s in shards for t in s])
        terms = {t for p, _ in BATCH for t in (P.terms_of(p) or ())}
        stats = (whole.o.doc_count, whole.o.sum_ttf, {t: max(whole.o.df(t), 0) for t in terms})
        whole.close()
    refs = [P.PhraseRef(s, global_stats=stats) for s in shards]
    bases = [sum(len(s) for s in shards[:g]) for g in range(len(shards))]
    out = [S.exact(S.merge([(S.search(r, p, s), b) for r, b in zip(refs, bases)])) for p, s in BATCH]
    for r in refs:
        r.close()
    return out


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_node_sloppy_hits_are_the_merged_shard_hits(mode):
    shards = [S.TEXTS[g::2] for g in range(2)]
    want = expected(shards, mode)
    n = D.Node(devices=[0, 0], stats_mode=mode, inproc=True)
    for g, s in enumerate(shards):
        n.add_documents(list(s), [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    assert n.stats()["num_docs"] == len(S.TEXTS)
    got = [S.exact(h) for h in n.search_phrase_slop_batch([p for p, _ in BATCH], [s for _, s in BATCH])]
    assert len(got) == len(BATCH)
    for (p, s), g, w in zip(BATCH, got, want):
        assert g == w, (p[:24], s)
    # the fixture: one phrase's hits lie on both shards, global ids past the first shard among them
    by = dict(zip(BATCH, got))
    first = len(shards[0])
    assert {d >= first for d, _, _ in by[(b"alpha beta", 2)]} == {False, True}
    assert {d >= first for d, _, _ in by[(b"a b", 1)]} == {False, True}
    assert len(by[(S.M64, 5)]) == 1 and by[(S.NO_WORK[0], 1)] == by[(S.NO_WORK[3], 2)] == by[(S.NO_WORK[2], 3)] == []
    assert n.search_phrase_slop_batch([], []) == []
    with pytest.raises(L.TfidfError) as e:
        n.search_phrase_slop_batch([b"alpha", b"a a"], [1, 1])
    assert e.value.code == L.E_UNSUPPORTED_QUERY
    with pytest.raises(L.TfidfError) as e:
        n.search_phrase_slop_batch([b"alpha", P.PHRASE_1025], [1, 0])
    assert e.value.code == L.E_INVALID_ARG
    n.close()


def test_node_sloppy_search_before_commit_is_a_state_error():
    n = D.Node(devices=[0, 0], inproc=True)
    n.add_documents([b"alpha beta", b"beta alpha"])
    with pytest.raises(L.TfidfError) as e:
        n.search_phrase_slop_batch([b"alpha beta"], [1])
    assert e.value.code == L.E_STATE
    n.close()
