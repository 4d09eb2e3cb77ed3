"""Nested compound queries on the device (tfidf_search_nested_batch and its
reader form) against compound_tree_ref.NestedRef, on the two corpora of
test_gpu_compound.py: the route corpus of routes_ref (25 200 documents in 4
blocks, route documents at 8191 / 8192: the smallest corpus with a block edge
and an empty middle block) and the Lucene fixture.  Ids, order and float32 score
bits are compared exactly.

  1  the case batch: every kind as a leaf at depths 1..4 and inside a group of
     every occur, `*` inside nested groups as SHOULD, FILTER and MUST_NOT (every
     slot of every tile is written and read), min_should_match of 0, 1, 2, |S|,
     |S| + 1 and 256 at the root and in inner groups, a 64-node tree, empty and
     MUST_NOT-only groups, the empty-middle-block query one level down; on
     ShardIndex and on a Reader
  2  the identities, byte for byte: the flat batch sent as root groups is the
     flat call's arrays; group([should(x)]) is x; m = 1 on a pure disjunction
     is m = 0
  3  chunking: TFIDF_COMPOUND_CHUNK of 5 and of 40 000 gives the same bytes in
     many chunks.  The tile follows the deepest query of a chunk: in one chunk
     every query runs on 512-document tiles, under a budget of 5 a query with
     entries starts a chunk of its own, so queries of 1, 2, 3 and 4 levels run
     on 2048-, 1024- and 512-document tiles (asserted below); equal bytes show
     that the result does not depend on the tile
  4  ties: 2.0 everywhere and 0.0 everywhere come out doc-ascending across
     8191 / 8192
  5  protocol and errors
  6  lifecycle: a reader across a commit; deleted documents
  7  a term-major index, (k1, b) = (2.0, 1.0), a caller's stream
  8  Worker.search_expr
"""
import ctypes as C

import numpy as np
import pytest

import compound_ref as CR
import compound_tree_ref as TR
import routes_ref as RR
from routes_ref import BASE, BLOCK, FIRST_A
from tfidf_amd import _lib as L
from tfidf_amd import engine as E
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker

import test_gpu_compound as FLAT
from test_compound_tree_cpu import arg_cases, max_group_depth
from test_gpu_compound import A0, DOCS, OCCURS, canon, got_lists, lucene, pools, ref_of, route_index, untouched  # noqa: F401
from test_gpu_incremental_commit import add, keyed

pytestmark = pytest.mark.gpu

T = E.text
STAR = E.wildcard(b"*")
G = E.group
M_VALUES = lambda n_should: (0, 1, 2, n_should, n_should + 1, 256)          # noqa: E731


def nref(texts, k1=1.2, b=0.75):
    return TR.NestedRef(None, ref=ref_of(texts, k1, b))


def wrap(child, depth, ocs=(E.must, E.should)):
    """The occurred node ``child`` at depth ``depth`` (1..4) below a root, each group on the way its only child."""
    for i in range(depth - 1):
        child = ocs[i % len(ocs)](G([child]))
    return G([child])


def shoulds():
    return [E.should(T(RR.M1)), E.should(T(RR.M2)), E.should(E.wildcard(b"mq*")),
            E.should(E.phrase(RR.M1 + b" " + RR.M2, 0)), E.should(T(RR.c(1)))]


def case_batch():
    ps = pools()
    at = [0] * 5

    def take(k):
        at[k] += 1
        return ps[k][(at[k] * 5 + at[k] // len(ps[k])) % len(ps[k])]

    common = E.should(T(RR.c(2)))
    qs = []
    for k in range(5):                                   # every kind as a leaf at depths 1..4
        for depth in (1, 2, 3, 4):
            qs.append(wrap((E.should, E.must)[depth & 1](take(k)), depth))
    for k in range(5):                                   # every kind inside a group of every occur
        for oc in OCCURS:
            qs.append(G([oc(G([E.should(take(k)), E.should(take(k))])), common]))
    # `*` in nested groups as SHOULD, FILTER and MUST_NOT: every slot of every tile
    qs.append(G([E.must(G([E.should(STAR), E.should(T(RR.M1))])),
                 E.must_not(G([E.must(E.wildcard(b"mq*")), E.must(E.regex(b"mq(alpha|beta)"))]))]))
    qs.append(G([E.filter_(G([E.filter_(G([E.should(STAR)]))])), E.should(T(RR.M1))]))
    qs.append(G([E.must_not(G([E.should(G([E.must(STAR)]))])), E.should(T(RR.M1))]))
    qs.append(wrap(E.should(STAR), 4, (E.should,)))
    qs.append(G([E.should(G([E.should(G([E.filter_(G([E.must(STAR)])), E.should(T(RR.M2))]))])), E.must_not(T(RR.MX))]))
    s = shoulds()
    for m in M_VALUES(len(s)):                           # min_should_match at the root and in inner groups, without and with R
        qs.append(G(s, m))
        qs.append(G([E.must(G(s, m)), common]))
        qs.append(G([E.must(T(RR.c(1)))] + s, m))
        qs.append(G([E.should(G([E.filter_(E.wildcard(b"mq*"))] + s, m)), E.should(G(s[:2], min(m, 3)))]))
    # 64 nodes: the root, seven groups that each ask for two of their eight common words
    qs.append(G([E.should(G([E.should(T(RR.c(8 * i + j + 1))) for j in range(8)], 2)) for i in range(7)]))
    assert TR.n_nodes(qs[-1]) == 64
    for oc in OCCURS:                                    # empty and MUST_NOT-only groups
        qs.append(G([oc(G([])), E.should(T(RR.M1))]))
        qs.append(G([oc(G([E.must_not(T(RR.M2))])), E.should(T(RR.M1))]))
    qs += [G([]), G([E.should(G([]))]), G([E.must_not(T(RR.M1))])]
    # "zarblat" lies in blocks 0 and 2 only: block 1 is an empty run between two runs with hits, one level down
    qs.append(G([E.must(G([E.must(T(RR.FUZ[4])), E.should(E.wildcard(b"zorbl*")), E.should(E.wildcard(b"za*"))]))]))
    return qs


def check(h, ref, queries):
    got = got_lists(h.search_nested_batch_arrays(queries))
    assert len(got) == len(queries)
    for q, g in zip(queries, got):
        assert g == CR.exact(ref.search(q)), q
    return got


# 1 ------------------------------------------------------------------------------------------

def test_the_case_batch(route_index):
    ref, qs = nref(BASE), case_batch()
    got = check(route_index, ref, qs)
    with route_index.reader() as rd:
        assert got_lists(rd.search_nested_batch_arrays(qs)) == got
    by_blocks = [{d // BLOCK for d, _ in g} for g in got]
    assert any(b == {0, 1, 2, 3} for b in by_blocks) and by_blocks[-1] == {0, 2}
    assert sum(1 for g in got if g) > len(got) // 3 and sum(1 for g in got if not g) >= 10
    assert {TR.depth(q) for q, g in zip(qs, got) if g} >= {1, 2, 3, 4}
    # `*` at depth 4 reaches every document; the m cases shrink as m grows and end empty
    star4 = qs.index(wrap(E.should(STAR), 4, (E.should,)))
    assert [d for d, _ in got[star4]] == list(range(len(BASE)))
    s = shoulds()
    sizes = [len(got[qs.index(G(s, m))]) for m in M_VALUES(len(s))]
    assert sizes[0] == sizes[1] > sizes[2] > sizes[3] and sizes[2] > 0 and sizes[4:] == [0, 0]
    entries, chunks, pairs, ms = route_index.last_compound_stats()
    assert chunks == 1 and pairs == len(qs) * 4 and entries > 100000 and ms > 0.0


def test_the_lucene_fixture(lucene):
    g, texts = lucene
    ref = TR.NestedRef(texts)
    qs = [G([E.must(G([E.should(T(b"fast")), E.should(T(b"best"))])), E.should(G([E.must(T(b"food"))]))]),
          G([E.should(T(b"best")), E.should(T(b"wireless")), E.should(T(b"earbuds")), E.should(T(b"fast"))], 2),
          G([E.must(G([E.should(E.phrase(b"fast food", 0)), E.should(E.fuzzy(b"fsat", 2, 0, 50))], 1)),
             E.must_not(G([E.should(T(b"kheder")), E.should(T(b"wireless"))]))]),
          G([E.filter_(G([E.should(STAR)])), E.should(G([E.should(G([E.should(G([E.should(T(b"fast"))]))]))]))]),
          G([E.should(E.regex(b"f(a|o).*")), E.should(T(b"food"))], 3), G([])]
    got = check(g, ref, qs)
    with g.reader() as rd:
        assert got_lists(rd.search_nested_batch_arrays(qs)) == got
    assert sum(1 for x in got if x) >= 4 and got[4] == [] and got[5] == []
    for q, want in zip(qs, got):                         # the batch of one
        assert [(d, CR.bits(s)) for d, s in g.search_nested(q)] == want
    ref.close()


# 2 ------------------------------------------------------------------------------------------

def test_the_identities_hold_byte_for_byte(route_index):
    g = route_index
    # the flat batch; its 64-clause query gives up its last clause to the root (64 nodes: the largest tree)
    flat = [q[:63] for q in FLAT.batch()]
    assert max(len(q) for q in flat) == 63 and len(flat[-3]) == 63
    d, s, o, _ = g.search_nested_batch_arrays(flat)                           # a plain list is a root with m = 0
    assert canon(d, s, o) == canon(*g.search_compound_batch_arrays(flat)[:3])
    assert canon(*g.search_nested_batch_arrays([G(q) for q in flat])[:3]) == canon(d, s, o)
    assert len(d) > 100000
    qs = case_batch()
    want = canon(*g.search_nested_batch_arrays(qs)[:3])
    deep = [q for q in qs if max_group_depth(q) <= 2 and TR.n_nodes(q) < 64]  # room for one more level and node
    assert len(deep) > len(qs) // 2
    base = canon(*g.search_nested_batch_arrays(deep)[:3])
    assert canon(*g.search_nested_batch_arrays([G([E.should(q)]) for q in deep])[:3]) == base
    assert canon(*g.search_nested_batch_arrays([G([E.must(q)]) for q in deep])[:3]) == base
    # one MUST child and m = 1 asks for a SHOULD child that does not exist: by the match rule, nothing
    assert len(g.search_nested_batch_arrays([G([E.must(q)], 1) for q in deep])[0]) == 0
    assert canon(*g.search_nested_batch_arrays([G([E.should(q)], 1) for q in deep])[:3]) == base
    # m = 1 on a pure disjunction is m = 0
    pure = [q for q in qs if q[2] == 0 and q[1] and all(c[0] == L.OCCUR_SHOULD for c in q[1])]
    assert len(pure) >= 5
    assert canon(*g.search_nested_batch_arrays([G(q[1], 1) for q in pure])[:3]) == canon(
        *g.search_nested_batch_arrays(pure)[:3])
    assert canon(*g.search_nested_batch_arrays(qs)[:3]) == want


# 3 ------------------------------------------------------------------------------------------

def test_chunking_and_the_tile_do_not_change_the_bytes(route_index, monkeypatch):
    g, qs = route_index, case_batch()
    d0, s0, o0, _ = g.search_nested_batch_arrays(qs)
    entries0, chunks0, _, _ = g.last_compound_stats()
    assert chunks0 == 1 and max(max_group_depth(q) for q in qs) == 3          # the one chunk ran on 512-document tiles
    # the levels that run on a tile of their own under the small budget: queries with hits
    o = o0.tolist()
    alone = {max_group_depth(q) + 1 for i, q in enumerate(qs) if o[i + 1] - o[i] > 5}
    assert alone == {1, 2, 3, 4}
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    for budget in ("5", "40000"):
        monkeypatch.setenv("TFIDF_COMPOUND_CHUNK", budget)
        d, s, o, _ = g.search_nested_batch_arrays(qs)
        assert canon(d, s, o) == canon(d0, s0, o0)
        entries, chunks, pairs, _ = g.last_compound_stats()
        assert chunks > 1 and entries == entries0 and pairs == len(qs) * 4
        if budget == "5":
            assert chunks > len(qs) // 2                 # only a query without entries shares a chunk


# 4 ------------------------------------------------------------------------------------------

def test_ties_come_out_in_document_order_across_the_block_edge(route_index):
    g = route_index
    two = G([E.must(G([E.should(STAR)])), E.must(G([E.must(G([E.filter_(STAR), E.should(E.regex(b".*"))]))]))])
    zero = G([E.filter_(G([E.should(STAR)]))])
    d, s, o, _ = g.search_nested_batch_arrays([two, zero])
    n = len(BASE)
    assert o.tolist() == [0, n, 2 * n]
    for i, bits in enumerate((CR.bits(2.0), CR.bits(0.0))):
        assert d[i * n:(i + 1) * n].tolist() == list(range(n))
        assert set(s[i * n:(i + 1) * n].view(np.uint32).tolist()) == {bits}


# 5 ------------------------------------------------------------------------------------------

def raw_arrays(fn, handle, blob, c_offs, arr, q_offs, cap, sentinel=0xAB):
    """One library call on sentinel-filled outputs -> (rc, docs, scores, offsets, n)."""
    nq = len(q_offs) - 1
    docs = np.full(max(cap, 1), sentinel, np.uint32)
    scores = np.full(max(cap, 1), np.float32(-7.0))
    offs = np.full(nq + 1, sentinel, np.uint64)
    n = C.c_uint64(sentinel)
    rc = fn(handle, blob, L.ptr(c_offs, C.c_uint64), arr, L.ptr(q_offs, C.c_uint64), nq,
            L.ptr(docs, C.c_uint32) if cap else None, L.ptr(scores, C.c_float) if cap else None, cap,
            L.ptr(offs, C.c_uint64), C.byref(n), None)
    return rc, docs, scores, offs, n.value


def raw(fn, handle, queries, cap):
    return raw_arrays(fn, handle, *E._qnode_arrays(queries), cap)


def test_protocol_and_errors(route_index):
    g = route_index
    lib = L.load()
    fn = lib.tfidf_search_nested_batch
    assert g.search_nested_batch([]) == []
    rc, _, _, offs, n = raw(fn, g._h, [], 0)
    assert (rc, offs.tolist(), n) == (L.OK, [0], 0)
    # a query of 0 nodes has no hits
    some = G([E.must(G([E.should(T(RR.M1)), E.should(T(RR.M2))], 2))])
    blob, c_offs, arr, q_offs = E._qnode_arrays([some])
    q3 = np.array([0, 0, int(q_offs[1]), int(q_offs[1])], np.uint64)
    rc, docs, _, offs, n = raw_arrays(fn, g._h, blob, c_offs, arr, q3, 4096)
    assert rc == L.OK and n > 0 and offs.tolist() == [0, 0, n, n]
    qs = [some, G([E.must(T(RR.M2)), E.must_not(G([E.should(T(RR.M3))]))])]
    want = got_lists(g.search_nested_batch_arrays(qs))
    total = sum(len(w) for w in want)
    assert total > 4 and want[0] and want[1]
    for cap in (0, total - 1):                           # the size query; one slot too few
        rc, docs, scores, offs, n = raw(fn, g._h, qs, cap)
        assert rc == L.E_BUFFER and n == total and offs.tolist() == [0, len(want[0]), total]
    rc, docs, scores, offs, n = raw(fn, g._h, qs, total)
    assert rc == L.OK and n == total and list(zip(docs.tolist(), scores.view(np.uint32).tolist())) == want[0] + want[1]
    # every argument rule: nothing written, the query and the node named
    seen = set()
    for name, qo, co, nodes, rule, at in arg_cases():
        if rule == 0:                                    # the accepted cases are the host checker's
            continue
        arr = (L.QNode * max(len(nodes), 1))()
        for i, (oc, kind, parent) in enumerate(nodes):
            arr[i].occur, arr[i].kind, arr[i].parent = oc, kind, parent
        res = raw_arrays(fn, g._h, b"x" * int(co[-1]), np.array(co, np.uint64), arr, np.array(qo, np.uint64), 64)
        seen.add(rule)
        assert res[0] == L.E_INVALID_ARG and untouched(res), name
        if at is not None and rule >= 5:
            assert lib.tfidf_last_error().startswith(b"query %d node %d:" % at), (name, lib.tfidf_last_error())
    assert seen == set(range(1, 12))
    # kind 5 stays a nested kind only; a leaf's route fails the call with its code, nothing written, the node named
    bad = G([E.should(T(RR.M1)), E.must(G([E.should(G([E.should(T(RR.M2)), E.must(E.regex(b"a(b"))]))]))])
    res = raw(fn, g._h, [some, bad], 64)
    assert res[0] == L.E_QUERY_SYNTAX and untouched(res)
    assert lib.tfidf_last_error().startswith(b"query 1 node 5:"), lib.tfidf_last_error()
    res = raw(fn, g._h, [G([E.must(G([E.must(E.phrase(RR.M1 + b" " + RR.M1, 1))]))])], 64)
    assert res[0] == L.E_UNSUPPORTED_QUERY and untouched(res)
    assert lib.tfidf_last_error().startswith(b"query 0 node 2:")
    with pytest.raises(L.TfidfError) as e:
        g.search_nested(bad)
    assert e.value.code == L.E_QUERY_SYNTAX
    # the index still answers
    assert got_lists(g.search_nested_batch_arrays(qs)) == want


def test_a_call_before_the_first_commit_is_a_state_error():
    g = ShardIndex()
    g.add_documents([b"alpha beta"], [b"k"])
    res = raw(L.load().tfidf_search_nested_batch, g._h, [G([E.should(T(b"alpha"))])], 8)
    assert res[0] == L.E_STATE and untouched(res)
    g.close()


# 6 ------------------------------------------------------------------------------------------

def lifecycle_queries():
    both = G([E.should(T(RR.M1)), E.should(T(RR.M2))], 2)
    return [G([E.should(G(q)), E.should(both)]) for q in FLAT.lifecycle_queries()] + [
        G([E.must(G(FLAT.lifecycle_queries()[1], 1)), E.must_not(G([E.filter_(G([E.should(T(RR.M3))]))]))])]


def test_a_reader_keeps_its_corpus_across_a_commit_and_deletes_renumber():
    qs = lifecycle_queries()
    g = ShardIndex()
    add(g, DOCS[:FIRST_A])
    g.commit()
    rd = g.reader()
    old = check(rd, nref(A0), qs)
    batch2 = RR.new_batch()
    add(g, keyed(batch2, FIRST_A))
    g.commit()
    texts = A0 + batch2
    new = check(g, nref(texts), qs)
    assert check(rd, nref(A0), qs) == old and new != old and new[1] != old[1]
    rd.close()
    dead = [3, 11, BLOCK - 1, FIRST_A + 1]
    keys = [DOCS[i][0] for i in dead[:3]] + [keyed(batch2, FIRST_A)[1][0]]
    assert g.delete_documents(keys) == len(dead)
    g.commit()
    live = [t for i, t in enumerate(texts) if i not in dead]
    after = check(g, nref(live), qs)
    assert after != new and g.stats()["num_docs"] == len(live)
    g.close()


# 7 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ctor", [dict(inversion=L.INVERSION_TERM), dict(k1=2.0, b=1.0), dict(stream=True)],
                         ids=["term_major", "k1_b", "caller_stream"])
def test_other_layouts_parameters_and_a_caller_stream(ctor):
    import torch
    ctor = dict(ctor)
    on_stream = ctor.pop("stream", False)
    qs = lifecycle_queries() + case_batch()[3:60:7]
    ref = nref(A0, ctor.get("k1", 1.2), ctor.get("b", 0.75))
    g = ShardIndex(**ctor)
    st = torch.cuda.Stream() if on_stream else None
    try:
        if st is not None:
            g.set_stream(st.cuda_stream)
        add(g, DOCS[:FIRST_A])
        g.commit()
        if "inversion" in ctor:
            assert g.stats()["term_major"] == 1
        got = check(g, ref, qs)
        assert sum(1 for x in got if x) >= 5
        if "k1" in ctor:
            assert got[0] != CR.exact(nref(A0).search(qs[0]))                 # the parameters reach the scores
    finally:
        if st is not None:
            g.set_stream(None)
        g.close()


# 8 ------------------------------------------------------------------------------------------

def test_worker_search_expr(tmp_path):
    texts = BASE[:40] + [RR.P_FULL + b" " + RR.FUZ[0], RR.P_FULL + b" " + RR.PIV_A, RR.FUZ[3] + b" " + RR.M1, RR.P_REV,
                         RR.M1 + b" " + RR.M2 + b" " + RR.c(9)]
    docs = tmp_path / "docs"
    docs.mkdir()
    names = ["d%03d.txt" % i for i in range(len(texts))]
    for n, t in zip(names, texts):
        (docs / n).write_bytes(t)
    w = Worker(documents_path=str(docs))
    w.init()
    with w.index.reader() as rd:
        order = [rd.doc_key(d).decode() for d in range(rd.num_docs)]
    by_name = dict(zip(names, texts))
    ref = TR.NestedRef([by_name[n] for n in order])
    q = '+(mqalpha mqbeta zorbl* "mqalpha mqbeta")~2 -(pivotalfa %s)' % RR.c(9).decode()
    tree = G([E.must(G([E.should(T(b"mqalpha")), E.should(T(b"mqbeta")), E.should(E.wildcard(b"zorbl*")),
                        E.should(E.phrase(b"mqalpha mqbeta", 0))], 2)),
              E.must_not(G([E.should(T(b"pivotalfa")), E.should(T(RR.c(9)))]))])
    want = ref.search(tree)
    loose = ref.search(G([tree[1][0][:2] + (tree[1][0][2], 0), tree[1][1]]))
    assert len(want) >= 3 and len({CR.bits(s) for _, s in want}) >= 2 and len(loose) > len(want)     # ~2 and the veto bite
    assert w.search_expr(q, k=0) == [{"document": {"name": order[d]}, "score": float(s)} for d, s in want]
    assert w.search_expr(q, k=2) == w.search_expr(q, k=0)[:2]
    assert w.search_expr("mqalpha mqbeta", k=0, min_should_match=2) == [
        {"document": {"name": order[d]}, "score": float(s)}
        for d, s in ref.search(G([E.should(T(b"mqalpha")), E.should(T(b"mqbeta"))], 2))]
    assert w.search_expr("", k=0) == [] and w.search_expr("()", k=0) == []
    assert w.search_expr("mqalpha -pivotalfa", k=0) == w.search_query("mqalpha -pivotalfa", k=0)
    for bad in ("(mqalpha", "mqalpha)", '"open'):
        with pytest.raises(L.QuerySyntaxError):
            w.search_expr(bad)
    ref.close()
    w.index.close()
