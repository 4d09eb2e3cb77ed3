"""More-like-this over a node (tfidf_node_more_like_this_batch): the corpora of
mlt_ref.py dealt over two and three shards of one device, in both statistics
modes.  The shard that owns a seed selects its terms (one MltRef per shard:
its own df and num_docs); every shard scores the term strings, with its own
statistics (SHARD) or the node's (GLOBAL: doc_count, sum_ttf and df summed over
the shards); the lists are merged by (score descending, global id ascending).
Compared exactly: ids, order and float32 score bits."""
import pytest

import mlt_ref as M
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

pytestmark = pytest.mark.gpu

LOOSE = dict(min_tf=1, min_df=1)


class NodeRef:
    def __init__(self, shards, mode):
        self.refs = [M.MltRef(s) if s else None for s in shards]
        self.bases = [sum(len(s) for s in shards[:g]) for g in range(len(shards))]
        self.n = sum(len(s) for s in shards)
        if mode == L.STATS_GLOBAL:
            live = [r for r in self.refs if r]
            df = {}
            for r in live:
                for t, p in r.post.items():
                    df[t] = df.get(t, 0) + len(p)
            dc, ttf = sum(r.o.doc_count for r in live), sum(r.o.sum_ttf for r in live)
            for r in live:
                r.set_global_stats(dc, ttf, df)

    def close(self):
        for r in self.refs:
            if r:
                r.close()

    def owner(self, doc):
        g = max(g for g in range(len(self.bases)) if self.bases[g] <= doc and self.refs[g])
        return g, doc - self.bases[g]

    def more_like_this(self, doc, k, exclude, **params):
        g, local = self.owner(doc)
        sel, _ = self.refs[g].terms(local, **{**M.DEFAULTS, **params})
        terms = [t for t, _, _, _ in sel]
        kk = k + 1 if exclude else k
        lists = [(r.hits_of_terms(terms, kk), b) for r, b in zip(self.refs, self.bases) if r]
        return terms, M.merge(lists, k, doc if exclude else None)


def node_of(shards, mode):
    n = D.Node(devices=[0] * len(shards), stats_mode=mode, inproc=True)
    for g, s in enumerate(shards):
        if s:
            n.add_documents(list(s), [b"s%d_%05d" % (g, i) for i in range(len(s))], shard=g)
    n.commit()
    return n


def global_id(shards, text_index):
    G = len(shards)
    g, i = text_index % G, text_index // G
    return sum(len(s) for s in shards[:g]) + i


@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD], ids=["global", "shard"])
@pytest.mark.parametrize("G", [2, 3])
def test_node_hits_are_the_merged_shard_hits(G, mode):
    shards = [M.TEXTS[g::G] for g in range(G)]
    r = NodeRef(shards, mode)
    n = node_of(shards, mode)
    try:
        assert n.stats()["num_docs"] == len(M.TEXTS)
        picks = [M.doc("skewed", i) for i in range(0, 12)] + [M.doc("esc", 0), M.doc("esc", 3), M.doc("empty_mid", 0),
                                                              M.doc("tie"), M.doc("skewed", 3), M.doc("empty_end")]
        seeds = [global_id(shards, t) for t in picks]
        assert {r.owner(s)[0] for s in seeds} == set(range(G))            # a seed on every shard
        for params, k, excl in (({}, 10, True), (LOOSE, 7, False), (dict(min_tf=2, min_df=1, max_terms=40), 3, True)):
            got = n.more_like_this_batch(seeds, k, excl, **params)
            assert len(got) == len(seeds)
            hits_on = set()
            for s, h in zip(seeds, got):
                terms, want = r.more_like_this(s, k, excl, **params)
                assert M.exact_hits(h) == M.exact_hits(want), (s, params)
                hits_on |= {r.owner(d)[0] for d, _ in h}
                if excl:
                    assert s not in [d for d, _ in h]
            assert hits_on == set(range(G))
        # terms the non-owning shards lack: the tie document's are its own alone
        tie = global_id(shards, M.doc("tie"))
        terms, want = r.more_like_this(tie, 3, False, min_tf=2, min_df=1, max_terms=40)
        g_own = r.owner(tie)[0]
        assert all(t not in r.refs[g].post for g in range(G) if g != g_own for t in terms) and len(terms) == 40
        assert [d for d, _ in want] == [tie]
        assert n.more_like_this_batch([], 10) == []
        for bad in ([len(M.TEXTS)], [seeds[0], 1 << 40]):
            with pytest.raises(L.TfidfError) as e:
                n.more_like_this_batch(bad, 10)
            assert e.value.code == L.E_INVALID_ARG
        with pytest.raises(L.TfidfError) as e:
            n.more_like_this_batch(seeds, 1024, True)
        assert e.value.code == L.E_INVALID_ARG
    finally:
        r.close()
        n.close()


def test_node_with_an_empty_shard():
    cut = M.doc("tie")
    shards = [M.TEXTS[:cut], [], M.TEXTS[cut:]]
    r = NodeRef(shards, L.STATS_GLOBAL)
    n = node_of(shards, L.STATS_GLOBAL)
    try:
        seeds = [M.doc("skewed", 2), cut, M.doc("esc", 1), M.doc("skewed", 59)]
        got = n.more_like_this_batch(seeds, 10, True)
        for s, h in zip(seeds, got):
            assert M.exact_hits(h) == M.exact_hits(r.more_like_this(s, 10, True)[1]), s
        assert any(h for h in got)
    finally:
        r.close()
        n.close()


def test_node_more_like_this_before_commit_is_a_state_error():
    n = D.Node(devices=[0, 0], inproc=True)
    n.add_documents([b"alpha beta", b"beta alpha"])
    with pytest.raises(L.TfidfError) as e:
        n.more_like_this_batch([0], 10)
    assert e.value.code == L.E_STATE
    n.close()
