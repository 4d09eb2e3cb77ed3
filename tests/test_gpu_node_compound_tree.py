"""Nested compound queries over a node (tfidf_node_search_nested_batch): the
route corpus of routes_ref dealt over two shards of one device over the
in-process transport, in both statistics modes, as test_gpu_node_compound.py
runs the flat call.  Each shard has its own NestedRef, on its own statistics
(SHARD) or on the statistics of all documents (GLOBAL); the shards' lists are
merged by (score bits descending, global id ascending).  Compared exactly: ids,
order and float32 score bits."""
import numpy as np
import pytest

import compound_ref as CR
import compound_tree_ref as TR
import routes_ref as RR
from routes_ref import BASE
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D
from tfidf_amd import engine as E

from test_gpu_compound_tree import case_batch, lifecycle_queries
from test_gpu_node_compound import deal

pytestmark = pytest.mark.gpu

QUERIES = case_batch()[::4] + case_batch()[-2:] + lifecycle_queries()
G = E.group


def expected(shards, mode):
    stats = None
    if mode == L.STATS_GLOBAL:
        own = [CR.CompoundRef(s) for s in shards]
        df = {}
        for r in own:
            for t, v in r.vocab.items():
                df[t] = df.get(t, 0) + v
        stats = (sum(r.o.doc_count for r in own), sum(r.o.sum_ttf for r in own), df)
        for r in own:
            r.close()
    refs = [TR.NestedRef(s, global_stats=stats) for s in shards]
    bases = [sum(len(s) for s in shards[:g]) for g in range(len(shards))]
    out = [CR.exact(CR.merge([(r.search(q), b) for r, b in zip(refs, bases)])) for q in QUERIES]
    for r in refs:
        r.close()
    return out


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_node_hits_are_the_merged_shard_hits(mode):
    shards = deal()
    want = expected(shards, mode)
    n = D.Node(devices=[0, 0], stats_mode=mode, inproc=True)
    for g, s in enumerate(shards):
        n.add_documents(list(s), [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    assert n.stats()["num_docs"] == len(BASE)
    docs, scores, offs, _ = n.search_nested_batch_arrays(QUERIES)
    assert docs.dtype == np.uint64
    d, s, o = docs.tolist(), scores.view(np.uint32).tolist(), offs.tolist()
    got = [list(zip(d[o[i]:o[i + 1]], s[o[i]:o[i + 1]])) for i in range(len(QUERIES))]
    for q, g, w in zip(QUERIES, got, want):
        assert g == w, q
    assert [[(a, CR.bits(b)) for a, b in hits] for hits in n.search_nested_batch(QUERIES[:5])] == want[:5]
    # the fixture: queries whose hits lie on both shards, nested ones among them
    first = len(shards[0])
    both = [q for q, g in zip(QUERIES, got) if g and {x >= first for x, _ in g} == {False, True}]
    assert len(both) >= 8 and max(TR.depth(q) for q in both) >= 3 and sum(1 for g in got if g) > len(got) // 3
    assert n.search_nested_batch([]) == []
    # a failing shard query fails the call with the shard's code; so does an argument rule
    for bad, code in (([QUERIES[0], G([E.must(G([E.should(E.regex(b"a(b"))]))])], L.E_QUERY_SYNTAX),
                      ([G([E.should(G([E.must(E.phrase(RR.M1 + b" " + RR.M1, 1))]))])], L.E_UNSUPPORTED_QUERY),
                      ([G([E.should(E.text(RR.c(i + 1))) for i in range(64)])], L.E_INVALID_ARG),
                      ([G([E.should(G([E.should(G([E.should(G([E.should(G([]))]))]))]))])], L.E_INVALID_ARG),
                      ([G([(L.OCCUR_MUST, 7, RR.M1)])], L.E_INVALID_ARG)):
        with pytest.raises(L.TfidfError) as e:
            n.search_nested_batch(bad)
        assert e.value.code == code
    assert n.search_nested_batch(QUERIES[:1]) == [[(a, float(np.uint32(b).view(np.float32))) for a, b in want[0]]]
    n.close()


def test_node_nested_search_before_commit_is_a_state_error():
    n = D.Node(devices=[0, 0], inproc=True)
    n.add_documents([b"alpha beta", b"beta alpha"])
    with pytest.raises(L.TfidfError) as e:
        n.search_nested_batch([G([E.should(E.text(b"alpha"))])])
    assert e.value.code == L.E_STATE
    n.close()
