"""The query routes over a node whose shards were committed incrementally, one
GPU, two shards on it (a repeated device, as in test_gpu_node.py).  Each shard
takes 8300 documents of the route corpus (routes_ref.py) into both of its
snapshots; then 200 documents with 50 new words go to shard 1 only.  In the
node commits that follow shard 0 adds nothing (block 0 kept, the per-slot df
left standing) while shard 1 moves its kept block to new columns, and the
GLOBAL exchange reads both shards' device df again.

GLOBAL: statistics, all hits, phrases, wildcard and regex lists, snippets and
matches by global id equal those of one index over shard 0's then shard 1's
documents (routes_ref.expected); fuzzy search and more-like-this expand and
select per shard and score under the node's statistics, merged as
test_gpu_node_fuzzy_search and test_gpu_node_mlt merge.  SHARD: the Leader sums
by name of per-shard oracles, as nodebatch.oracle_shard takes them.  All
compared exactly (float32 score bits, double sums)."""
import ctypes as C

import numpy as np
import pytest

import fuzzy_search_ref as R
import mlt_ref as M
import phrase_ref as P
import phrase_slop_ref as S
import routes_ref as RR
from nodebatch import oracle_hits
from oracle import oracle as O
from routes_ref import APPEND_A, BASE, FIRST_A, expected
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D

from test_gpu_node_batch_all import same_names
from test_gpu_node_mlt import NodeRef

pytestmark = pytest.mark.gpu

T0 = BASE[:FIRST_A]
T1 = BASE[FIRST_A + APPEND_A:2 * FIRST_A + APPEND_A]     # 8300 more; route documents of blocks 1 and 2 among them
BATCH = RR.new_batch()
NAMES = [b"f%05d.txt" % i for i in range(FIRST_A + APPEND_A)]        # shard 1 repeats shard 0's names
FUZZY_PARAMS = [(2, 0), (1, 2)]


def reported(n, g):
    """What shard g's last commit says it did."""
    lib, h = L.load(), n.shard(g)
    f, nb, r, docs, full = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    L.check(lib.tfidf_commit_inverted_blocks(h, C.byref(f), C.byref(nb), C.byref(r)))
    L.check(lib.tfidf_commit_tokenized_docs(h, C.byref(docs), C.byref(full)))
    return {"first_block": f.value, "n_blocks": nb.value, "remapped": r.value, "docs": docs.value,
            "was_full": bool(full.value)}


def history(mode):
    """The node after both shards' 8300 documents went into both of their snapshots and the batch was staged."""
    n = D.Node(devices=[0, 0], stats_mode=mode)
    n.add_documents(T0, NAMES[:FIRST_A], shard=0)
    n.add_documents(T1, NAMES[:FIRST_A], shard=1)
    for _ in range(2):
        n.commit()
        for g in (0, 1):
            assert reported(n, g) == {"first_block": 0, "n_blocks": 2, "remapped": 0, "docs": FIRST_A, "was_full": True}
    n.add_documents(BATCH, NAMES[FIRST_A:], shard=1)
    return n


# per node commit after the batch: (tokenized, remapped) of shard 1; shard 0 tokenizes nothing and keeps block 0
COMMITS = [(APPEND_A, 1), (APPEND_A, 1), (0, 0)]         # either snapshot takes the batch; then nothing is added


def commit(n, tokenized, remapped):
    n.commit()
    assert reported(n, 0) == {"first_block": 1, "n_blocks": 2, "remapped": 0, "docs": 0, "was_full": False}
    assert reported(n, 1) == {"first_block": 1, "n_blocks": 2, "remapped": remapped, "docs": tokenized,
                              "was_full": False}


def fuzzy_hits(shards, all_, t, e, p):
    """Every shard expands over its own vocabulary and weights under the node's statistics (test_gpu_node_fuzzy_search)."""
    stats = dict(df_of=all_.vocab, doc_count=all_.o.doc_count, sum_ttf=all_.o.sum_ttf)
    merged, n_exp, base = [], 0, 0
    for sh in shards:
        exp, _ = R.expansion(sh.vocab, t, e, p, RR.EXPANSIONS)
        n_exp += len(exp)
        merged += [(d + base, s) for d, s in R.hits(R.clause_scores(sh, exp, **stats))]
        base += sh.n
    merged.sort(key=lambda h: (-float(h[1]), h[0]))
    return R.bits(merged), n_exp


def test_global_node_with_one_shard_appended():
    shards = [T0, T1 + BATCH]
    all_ = expected(shards[0] + shards[1])
    per_shard = [R.Shard(s) for s in shards]
    mlt = NodeRef(shards, L.STATS_GLOBAL)
    w = all_.want
    want_fuzzy = {(t, e, p): fuzzy_hits(per_shard, all_, t, e, p) for t in RR.FUZZY for e, p in FUZZY_PARAMS}
    want_mlt = {(d, i): M.exact_hits(mlt.more_like_this(d, 10, True, **params)[1])
                for d in all_.seeds for i, params in enumerate(RR.MLT_PARAMS)}
    # the fixture: seeds and fuzzy hits on either shard, new words beside old ones in one wildcard list
    assert {mlt.owner(d)[0] for d in all_.seeds} == {0, 1}
    assert {d >= FIRST_A for d, _ in want_fuzzy[RR.FUZ[0], 2, 0][0]} == {False, True}
    assert {t in RR.NEW_WORDS for t, _ in w["wild_terms", RR.OLD_AND_NEW, 1024][0]} == {False, True}
    n = history(L.STATS_GLOBAL)
    try:
        for tokenized, remapped in COMMITS:
            commit(n, tokenized, remapped)
            s = n.stats()
            assert (s["n_shards"], s["num_docs"], s["doc_count"], s["sum_ttf"], s["num_terms"]) == \
                (2, len(all_.texts), all_.o.doc_count, all_.o.sum_ttf, all_.o.num_terms)
            for q, got in zip(RR.QUERIES, n.search_batch_all(RR.QUERIES)):
                assert RR.hit_bits(got) == w["search", q, 0], q
            for p, got in zip(RR.PHRASES, n.search_phrase_batch(RR.PHRASES)):
                assert P.exact(got) == w["phrase", p], p
            ph, sl = all_.slop_batch()
            for p, slop, got in zip(ph, sl, n.search_phrase_slop_batch(ph, sl)):
                assert S.exact(got) == w["slop", p, slop], (p, slop)
            for name, pats, terms, docs in (("wild", RR.WILDCARDS, n.wildcard_terms_batch, n.search_wildcard_batch),
                                            ("regex", RR.REGEXES, n.regex_terms_batch, n.search_regex_batch)):
                for m in (5, 1024):
                    for p, got in zip(pats, terms(pats, m)):
                        assert got == w[name + "_terms", p, m], (p, m)
                for p, got in zip(pats, docs(pats)):
                    assert got == w[name + "_docs", p], p
            for e, p in FUZZY_PARAMS:
                d, sc, offs, n_exp, _ = n.search_fuzzy_batch_arrays(RR.FUZZY, e, p, RR.EXPANSIONS)
                o = offs.tolist()
                for i, t in enumerate(RR.FUZZY):
                    got = list(zip(d[o[i]:o[i + 1]].tolist(), sc[o[i]:o[i + 1]].view(np.int32).tolist()))
                    assert (got, int(n_exp[i])) == want_fuzzy[t, e, p], (t, e, p)
            for i, params in enumerate(RR.MLT_PARAMS):
                for seed, got in zip(all_.seeds, n.more_like_this_batch(all_.seeds, 10, True, **params)):
                    assert M.exact_hits(got) == want_mlt[seed, i], (seed, params)
            per = [all_.route_ids] * len(RR.TEXT_QUERIES)
            for q, got in zip(RR.TEXT_QUERIES, n.snippets_batch(RR.TEXT_QUERIES, per, RR.WIDTH)):
                assert got == w["snippets", q], q
            for q, got in zip(RR.TEXT_QUERIES, n.matches_batch(RR.TEXT_QUERIES, per)):
                assert got == w["matches", q], q
    finally:
        n.close()
        mlt.close()


def test_shard_node_sums_by_name():
    workers = []
    for texts, names in ((T0, NAMES[:FIRST_A]), (T1 + BATCH, NAMES)):
        o = O.OracleIndex()
        for name, t in zip(names, texts):
            o.add_doc(name, t)
        o.commit()
        workers.append(o)
    want = [O.leader_merge([[(o.doc_key(d), float(s)) for d, s in oracle_hits(o, q)] for o in workers])
            for q in RR.QUERIES]
    for o in workers:
        o.close()
    sums = {q: sum(1 for _ in x) for q, x in zip(RR.QUERIES, want)}
    assert sums[RR.M1] and sums[RR.NEW_WORDS[0]] and sums[RR.LONG_TERM]
    n = history(L.STATS_SHARD)
    try:
        for tokenized, remapped in COMMITS:
            commit(n, tokenized, remapped)
            same_names(n.search_names_batch(RR.QUERIES), want)
            assert n.last_failed() == 0
    finally:
        n.close()
