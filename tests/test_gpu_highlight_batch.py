"""Batched hit highlighting on the device (tfidf_matches_batch /
tfidf_snippets_batch, their reader and node forms) against highlight_ref.py,
compared exactly.  One index holds the corpora of highlight_ref side by side
(document ids offset per corpus); the expected value of every row (query,
document) comes from highlight_ref alone.  Rows repeat within and across
queries, come in descending order, queries own no rows at the front, in the
middle and at the end; row chunks of every size through the budget knobs;
queries that do not parse; argument errors; the buffer protocol, also across
a chunk edge; hashed keys under forced collisions; snapshots beside commits;
nodes of three shards in both statistics modes; Worker.search_snippets_batch."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import highlight_ref as H
from tfidf_amd import _lib as L
from tfidf_amd import distributed as D
from tfidf_amd.engine import ShardIndex
from tfidf_amd.reference_api import Worker

pytestmark = pytest.mark.gpu

CORPORA = ["edge", "unicode", "ops", "dup", "dotted", "seventy", "malformed", "twins", "dense"]
WIDTHS = [16, 160, 1024]
TEXTS, BASE = [], {}
for _name in CORPORA:
    BASE[_name] = len(TEXTS)
    TEXTS += list(H.corpus(_name)[0])
N_DOCS = len(TEXTS)


def doc(name, i):
    return BASE[name] + i


def own(name):
    _, q, terms = H.corpus(name)
    return q, tuple(terms)


@functools.lru_cache(maxsize=None)
def exp_matches(terms, d):
    return H.matches(TEXTS[d], list(terms))


@functools.lru_cache(maxsize=None)
def exp_snippet(terms, d, W):
    a, b, ms = H.snippet(TEXTS[d], exp_matches(terms, d), W)
    return a, TEXTS[d][a:b], ms


_state = {}


def index():
    """The committed index over all corpora, shared by the tests (never changed)."""
    if "g" not in _state:
        g = ShardIndex()
        g.add_documents(list(TEXTS), [b"d/%05d" % i for i in range(N_DOCS)])
        g.commit()
        _state["g"] = g
    return _state["g"]


EDGE_BIG = doc("edge", H.LENGTHS.index(70000))                      # 70 000 bytes: 5 items
DENSE = doc("dense", 0)                                             # ~5 200 matches
ABSENT = (b"zzqqabsent yyqqabsent", (b"zzqqabsent", b"yyqqabsent"))


def batch():
    """[(query, positive terms, [documents])]: the mixed batch of most tests."""
    edge = [doc("edge", i) for i in range(63, -1, -1)]              # descending, every length of LENGTHS twice
    edge[5] = edge[6]                                               # a repeat within the query
    all_of = lambda name: [doc(name, i) for i in range(len(H.corpus(name)[0]))]     # noqa: E731
    return [
        (b"alpha", (b"alpha",), []),                                               # no rows, at the front
        own("edge") + (edge,),
        own("unicode") + (all_of("unicode") + [doc("ops", 4), EDGE_BIG],),         # a non-hit; a repeat across queries
        own("ops") + (all_of("ops") + [doc("unicode", 6), EDGE_BIG, doc("ops", 0)],),
        (b"beta", (b"beta",), []),                                                 # no rows, in the middle
        own("dup") + (all_of("dup") + all_of("dotted"),),
        own("dotted") + (all_of("dotted") + all_of("dup") + [doc("ops", 3)],),
        own("seventy") + (all_of("seventy") + [doc("edge", 30)],),                 # 70 terms
        own("malformed") + (all_of("malformed") + [DENSE],),                       # alpha 0, gamma 1
        own("twins") + (all_of("twins")[::-1],),
        own("dense") + (all_of("dense") + [EDGE_BIG, EDGE_BIG],),
        ABSENT + ([EDGE_BIG, doc("unicode", 0)],),                                 # no term present
        (b"gamma alpha", (b"gamma", b"alpha"), [DENSE] + all_of("malformed") + all_of("ops")),   # gamma 0, alpha 1
        (b"kappa", (b"kappa",), []),                                               # no rows, at the end
    ]


def want_matches(b):
    return [[exp_matches(terms, d) for d in docs] for _, terms, docs in b]


def want_snippets(b, W):
    return [[exp_snippet(terms, d, W) for d in docs] for _, terms, docs in b]


def args(b):
    return [q for q, _, _ in b], [docs for _, _, docs in b]


# 1. the mixed batch
def test_matches_of_the_mixed_batch():
    b = batch()
    g = index()
    got = g.matches_batch(*args(b))
    want = want_matches(b)
    assert [len(x) for x in got] == [len(x) for x in want]
    for qi, (gq, wq) in enumerate(zip(got, want)):
        for d, gm, wm in zip(b[qi][2], gq, wq):
            assert gm == wm, (qi, d)
    # the fixture reaches its cases
    assert len(got[10][0]) > 5000 and got[11] == [[], []] and got[2][-2] == []
    assert max(o for _, _, o in got[7][2]) == 69
    assert {o for _, _, o in got[8][-1]} == {0, 1} and [o for _, _, o in got[8][-1][:2]] == [0, 1]
    assert [o for _, _, o in got[12][0][:2]] == [1, 0]              # the same tokens under the other query's ordinals
    mal = H.corpus("malformed")[0]
    assert [H.doc_tokens(t) is None for t in mal] == [False, True, True, False, True]
    assert got[8][1] == got[8][2] == got[8][4] == [] and got[8][0] and got[8][3]
    with g.reader() as rd:
        assert rd.matches_batch(*args(b)) == got
        assert got == [rd.matches(q, docs) for q, _, docs in b]    # the loop of single-query calls


@pytest.mark.parametrize("W", WIDTHS)
def test_snippets_of_the_mixed_batch(W):
    b = batch()
    g = index()
    got = g.snippets_batch(*args(b), W)
    want = want_snippets(b, W)
    assert [len(x) for x in got] == [len(x) for x in want]
    for qi, (gq, wq) in enumerate(zip(got, want)):
        for d, gs, ws in zip(b[qi][2], gq, wq):
            assert gs == ws, (W, qi, d)
            assert len(gs[1]) <= W
    assert got[11][0] == (0, TEXTS[EDGE_BIG][:W], []) and got[11][1][0] == 0 and got[11][1][2] == []   # heads
    with g.reader() as rd:
        assert rd.snippets_batch(*args(b), W) == got
        assert got == [rd.snippets(q, docs, W) for q, _, docs in b]


def test_smallest_shapes():
    g = index()
    with g.reader() as rd:
        for h in (g, rd):
            assert h.matches_batch([], []) == [] and h.snippets_batch([], [], 64) == []                 # n_q = 0
            assert h.matches_batch([b"alpha", b"beta"], [[], []]) == [[], []]                           # R = 0
            assert h.snippets_batch([b"alpha", b"beta"], [[], []], 64) == [[], []]
            q, terms = own("unicode")
            d = doc("unicode", 1)
            assert h.matches_batch([q], [[d]]) == [[exp_matches(terms, d)]]                             # one row
            assert h.snippets_batch([q], [[d]], 16) == [[exp_snippet(terms, d, 16)]]
            assert h.snippets_batch([b"alpha", q, b"beta"], [[], [d], []], 160) == [[], [exp_snippet(terms, d, 160)], []]


# 2. row chunks
def equal_arrays(a, b):
    """Every array and the text of two *_batch_arrays results, bit for bit (not the device time)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, bytes):
            assert x == y
        elif not isinstance(x, float):
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all()


@pytest.mark.parametrize("knob, value", [("TFIDF_HL_CHUNK_ITEMS", "1"), ("TFIDF_HL_CHUNK_ITEMS", "3"),
                                         ("TFIDF_HL_CHUNK_MATCHES", "1"), ("TFIDF_HL_CHUNK_MATCHES", "7"),
                                         ("TFIDF_HL_CHUNK_MATCHES", "100"), ("both", "3/7")])
def test_any_chunking_gives_the_unchunked_output(knob, value, monkeypatch):
    """Items 1: every row with work is a chunk, edges inside each query's rows
    and between queries; items 3: the 70 000-byte document (5 items) is a
    chunk of its own beside chunks of several rows; matches 1 / 7 / 100:
    dense's ~5 200-match row exceeds the budget alone and rows of 0 matches
    ride along."""
    b = batch()
    g = index()
    with g.reader() as rd:
        whole_m = rd.matches_batch_arrays(*args(b))
        whole_s = {W: rd.snippets_batch_arrays(*args(b), W) for W in (16, 160)}
        assert g.last_highlight_chunks() == (1, 1)
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        if knob == "both":
            monkeypatch.setenv("TFIDF_HL_CHUNK_ITEMS", value.split("/")[0])
            monkeypatch.setenv("TFIDF_HL_CHUNK_MATCHES", value.split("/")[1])
        else:
            monkeypatch.setenv(knob, value)
        equal_arrays(rd.matches_batch_arrays(*args(b)), whole_m)
        for W in (16, 160):
            equal_arrays(rd.snippets_batch_arrays(*args(b), W), whole_s[W])
            item_chunks, row_chunks = g.last_highlight_chunks()
            n_rows = sum(len(docs) for _, _, docs in b)
            assert n_rows >= row_chunks >= item_chunks
            if knob == "TFIDF_HL_CHUNK_MATCHES":
                assert item_chunks == 1 and row_chunks > len(b)
            else:
                assert item_chunks > (len(b) if value == "1" else 8)
    assert sum(len(m) for m in want_matches(b)[1]) > 100 and len(whole_m[0]) > 20000


def test_single_calls_leave_the_chunk_report_alone(monkeypatch):
    """tfidf_last_highlight_chunks is of the last batched call: the single
    forms run the same rows machinery (cut by the same knob) and do not report."""
    b = batch()
    g = index()
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    monkeypatch.setenv("TFIDF_HL_CHUNK_ITEMS", "3")
    g.matches_batch(*args(b))
    report = g.last_highlight_chunks()
    assert report[1] >= report[0] > 8
    q, terms = own("edge")
    docs = [doc("edge", i) for i in range(24, 32)]                  # 14 items: far fewer chunks than the batch's
    assert g.matches(q, docs) == [exp_matches(terms, d) for d in docs]
    assert g.last_highlight_chunks() == report
    assert g.snippets(q, docs, 160) == [exp_snippet(terms, d, 160) for d in docs]
    assert g.last_highlight_chunks() == report


# 3. queries that do not parse
def test_unparseable_queries_have_no_matches_and_head_snippets():
    g = index()
    q, terms = own("ops")
    docs = [doc("ops", 0), doc("ops", 1), DENSE]
    queries = [b"AND x", q, b"alpha \xff", b"", q, b"x NOT"]
    per = [docs, docs, docs[::-1], [docs[0]], [], docs]
    got_m = g.matches_batch(queries, per)
    got_s = g.snippets_batch(queries, per, 64)
    for i in (0, 2, 3, 5):
        assert got_m[i] == [[] for _ in per[i]]
        assert got_s[i] == [(0, TEXTS[d][:64], []) for d in per[i]]
    assert got_m[1] == [exp_matches(terms, d) for d in docs] and got_m[4] == [] and got_m[1][0]
    assert got_s[1] == [exp_snippet(terms, d, 64) for d in docs] and got_s[4] == []


# 4. argument errors: nothing written
def raw_snippets(rd, queries, docs, d_offs, W, t_cap, m_cap, null=False, fill=7):
    """One tfidf_reader_snippets_batch call into sentinel-filled outputs."""
    lib = L.load()
    R = len(docs)
    q_offs = np.zeros(len(queries) + 1, np.uint64)
    q_offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    d = np.asarray(docs, np.uint32)
    do = np.asarray(d_offs, np.uint64)
    o = {"text": np.full(max(t_cap, 1), fill, np.uint8), "t_offs": np.full(R + 1, fill, np.uint64),
         "d_starts": np.full(max(R, 1), fill, np.uint64), "st": np.full(max(m_cap, 1), fill, np.uint64),
         "ln": np.full(max(m_cap, 1), fill, np.uint32), "od": np.full(max(m_cap, 1), fill, np.uint32),
         "m_offs": np.full(R + 1, fill, np.uint64)}
    nt, nm = C.c_uint64(fill), C.c_uint64(fill)
    rc = lib.tfidf_reader_snippets_batch(
        rd._h, b"".join(queries), L.ptr(q_offs, C.c_uint64), len(queries), L.ptr(d, C.c_uint32),
        L.ptr(do, C.c_uint64), W, None if null else o["text"].ctypes.data_as(C.c_void_p), t_cap,
        L.ptr(o["t_offs"], C.c_uint64), L.ptr(o["d_starts"], C.c_uint64),
        None if null else L.ptr(o["st"], C.c_uint64), None if null else L.ptr(o["ln"], C.c_uint32),
        None if null else L.ptr(o["od"], C.c_uint32), m_cap, L.ptr(o["m_offs"], C.c_uint64), C.byref(nt),
        C.byref(nm), None)
    return rc, o, nt.value, nm.value


def raw_matches(rd, queries, docs, d_offs, cap, null=False, fill=7):
    lib = L.load()
    R = len(docs)
    q_offs = np.zeros(len(queries) + 1, np.uint64)
    q_offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    d = np.asarray(docs, np.uint32)
    do = np.asarray(d_offs, np.uint64)
    o = {"st": np.full(max(cap, 1), fill, np.uint64), "ln": np.full(max(cap, 1), fill, np.uint32),
         "od": np.full(max(cap, 1), fill, np.uint32), "m_offs": np.full(R + 1, fill, np.uint64)}
    nm = C.c_uint64(fill)
    rc = lib.tfidf_reader_matches_batch(
        rd._h, b"".join(queries), L.ptr(q_offs, C.c_uint64), len(queries), L.ptr(d, C.c_uint32),
        L.ptr(do, C.c_uint64), None if null else L.ptr(o["st"], C.c_uint64),
        None if null else L.ptr(o["ln"], C.c_uint32), None if null else L.ptr(o["od"], C.c_uint32), cap,
        L.ptr(o["m_offs"], C.c_uint64), C.byref(nm), None)
    return rc, o, nm.value


def untouched(o, *totals):
    return all((a == 7).all() for a in o.values()) and all(t == 7 for t in totals)


def test_argument_errors_write_nothing():
    g = index()
    qs = [b"alpha", b"gamma"]
    with g.reader() as rd:
        good = [doc("ops", 0), doc("ops", 1), doc("ops", 2)]
        for docs, d_offs, W in ((good[:2] + [N_DOCS], [0, 1, 3], 64),        # a document out of range
                                (good, [0, 2, 1], 64),                       # doc_offsets decrease
                                (good, [1, 2, 3], 64),                       # ... or do not start at 0
                                (good, [0, 1, 3], 15), (good, [0, 1, 3], 65537), (good, [0, 1, 3], 0)):
            rc, o, nt, nm = raw_snippets(rd, qs, docs, d_offs, W, 4096, 256)
            assert rc == L.E_INVALID_ARG and untouched(o, nt, nm), (docs, d_offs, W)
        for docs, d_offs in ((good[:2] + [N_DOCS], [0, 1, 3]), (good, [0, 2, 1]), (good, [1, 2, 3])):
            rc, o, nm = raw_matches(rd, qs, docs, d_offs, 256)
            assert rc == L.E_INVALID_ARG and untouched(o, nm), (docs, d_offs)
        rc, o, nt, nm = raw_snippets(rd, qs, good, [0, 1, 3], 64, 4096, 256)
        assert rc == L.OK and nt == sum(min(64, len(TEXTS[d])) for d in good) and not untouched(o, nt, nm)
    with pytest.raises(L.TfidfError) as e:
        g.snippets_batch(qs, [[0], [N_DOCS]], 64)
    assert e.value.code == L.E_INVALID_ARG


# 5. buffer protocol
@pytest.mark.parametrize("chunk_matches", [None, "40"])
def test_buffer_protocol(chunk_matches, monkeypatch):
    """Sizes alone, text one short, matches one short: TFIDF_E_BUFFER, and the
    offsets, doc_starts and totals are those of the successful call, also
    when the short cap is met in a later chunk than the first."""
    if chunk_matches:
        monkeypatch.setenv("TFIDF_DEBUG", "1")
        monkeypatch.setenv("TFIDF_HL_CHUNK_MATCHES", chunk_matches)
    g = index()
    q, _ = own("edge")
    queries = [q, b"AND", q]
    per = [[doc("edge", i) for i in range(40, 60)], [doc("edge", 3)], [doc("edge", i) for i in range(70, 60, -1)]]
    docs = [d for p in per for d in p]
    d_offs = [0, 20, 21, 31]
    with g.reader() as rd:
        text, t_offs, d_starts, st, ln, od, m_offs, _, _ = rd.snippets_batch_arrays(queries, per, 160)
        nt, nm = len(text), len(st)
        assert nt == int(t_offs[-1]) > 2000 and nm == int(m_offs[-1]) > 10

        def call(t_cap, m_cap, null=False):
            rc, o, ct, cm = raw_snippets(rd, queries, docs, d_offs, 160, t_cap, m_cap, null)
            assert (ct, cm) == (nt, nm)
            assert (o["t_offs"] == t_offs).all() and (o["m_offs"] == m_offs).all() and (o["d_starts"] == d_starts).all()
            return rc, o
        assert call(0, 0, null=True)[0] == L.E_BUFFER
        assert call(nt - 1, nm)[0] == L.E_BUFFER
        assert call(nt, nm - 1)[0] == L.E_BUFFER
        rc, o = call(nt, nm)
        assert rc == L.OK and o["text"].tobytes() == text and (o["st"] == st).all() and (o["ln"] == ln).all() \
            and (o["od"] == od).all()
        # matches
        mst, mln, mod, mo, _, _ = rd.matches_batch_arrays(queries, per)
        total = len(mst)
        assert total == int(mo[-1]) > nm
        for cap, null in ((0, True), (total - 1, False)):
            rc, o, cm = raw_matches(rd, queries, docs, d_offs, cap, null)
            assert rc == L.E_BUFFER and cm == total and (o["m_offs"] == mo).all()
        rc, o, cm = raw_matches(rd, queries, docs, d_offs, total)
        assert rc == L.OK and cm == total and (o["st"] == mst).all() and (o["ln"] == mln).all() and (o["od"] == mod).all()


# 6. hashed keys under forced collisions
def test_twin_queries_under_a_weak_hash(monkeypatch):
    texts, q, terms = H.corpus("twins")
    q2 = H.TWIN_A[1] + b" " + H.TWIN_U[1]                            # the other twin of each pair
    terms2 = H.plain_terms(q2)
    monkeypatch.setenv("TFIDF_DEBUG", "1")
    monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    g = ShardIndex()
    g.add_documents(list(texts))
    g.commit()
    assert g.stats()["hash_rebuilds"] == 1
    docs = [0, 1, 2]
    got = g.matches_batch([q, q2], [docs, docs[::-1]])
    assert got[0] == [H.matches(texts[d], terms) for d in docs] == H.expected_matches("twins")
    assert got[1] == [H.matches(texts[d], terms2) for d in docs[::-1]]
    assert got[0][1] == [] and [o for _, _, o in got[1][1]] == [0, 1, 0]      # document 1 holds only the second twins
    for W in (16, 64):
        sn = g.snippets_batch([q, q2], [docs, docs[::-1]], W)
        for qi, (tt, dd) in enumerate(((terms, docs), (terms2, docs[::-1]))):
            for d, (a, text, ms) in zip(dd, sn[qi]):
                wa, wb, wm = H.snippet(texts[d], H.matches(texts[d], tt), W)
                assert (a, text, ms) == (wa, texts[d][wa:wb], wm)
    g.close()


# 7. snapshots
def test_reader_keeps_its_snapshot_and_batches_run_beside_commits():
    old, new = b"alpha one beta. " * 30 + b"gamma", b"delta gamma two. " * 30 + b"alpha alpha"
    qa, ta, qb, tb = b"alpha gamma", [b"alpha", b"gamma"], b"beta delta", [b"beta", b"delta"]

    def expect(t):
        return tuple((H.matches(t, tt), H.snippet(t, H.matches(t, tt), 64)) for tt in (ta, tb))
    exp = {t: expect(t) for t in (old, new)}
    filler = [H.edge_doc(i, 300) for i in range(20)]
    g = ShardIndex()
    g.add_documents([old] + filler, [b"k"] + [b"f%d" % i for i in range(20)])
    g.commit()
    rd = g.reader()
    g.add_documents([new], [b"k"])
    g.commit()
    g.compact()
    g.commit()

    def observe(h, d):
        m = h.matches_batch([qa, qb], [[d], [d]])
        s = h.snippets_batch([qa, qb], [[d], [d]], 64)
        return tuple((m[i][0], (s[i][0][0], s[i][0][0] + len(s[i][0][1]), s[i][0][2])) for i in (0, 1))
    assert observe(rd, 0) == exp[old]
    nd = g.stats()["num_docs"] - 1
    assert g.doc_text(nd) == new and observe(g, nd) == exp[new]
    assert observe(rd, 0) == exp[old]
    rd.close()
    seen, loose, errs = [], [], []

    def writer():
        try:
            for i in range(5):
                g.add_documents([old if i % 2 == 0 else new], [b"k"])
                g.commit()
        except Exception as e:                                      # pragma: no cover
            errs.append(e)

    def asker():
        try:
            for _ in range(12):
                with g.reader() as r:
                    seen.append((r.doc_text(r.num_docs - 1), observe(r, r.num_docs - 1)))
                loose.append(observe(g, g.stats()["num_docs"] - 1))   # index form: maybe another snapshot per call
        except Exception as e:                                      # pragma: no cover
            errs.append(e)
    ts = [threading.Thread(target=writer), threading.Thread(target=asker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errs == []
    assert len(seen) == len(loose) == 12
    for text, ob in seen:
        assert text in (old, new) and ob == exp[text]
    for ob in loose:
        for i in (0, 1):                                            # every row: one of the two states
            assert ob[i][0] in (exp[old][i][0], exp[new][i][0]) and ob[i][1] in (exp[old][i][1], exp[new][i][1])
    g.close()


# 8. the node
@pytest.mark.parametrize("mode", [L.STATS_GLOBAL, L.STATS_SHARD])
def test_node_routes_global_ids_to_their_shards(mode):
    """Three shards on one device, uneven, the middle one empty: shard 0 the
    first 37 documents, shard 2 the rest.  Global ids are positions in TEXTS."""
    n = D.Node(devices=[0, 0, 0], stats_mode=mode)
    cut = 37
    n.add_documents(TEXTS[:cut], [b"a%d" % i for i in range(cut)], shard=0)
    n.add_documents(TEXTS[cut:], [b"b%d" % i for i in range(N_DOCS - cut)], shard=2)
    n.commit()
    assert n.stats()["num_docs"] == N_DOCS
    b = batch()
    b[1] = (b[1][0], b[1][1], [0, cut, cut - 1, EDGE_BIG, 1, cut + 1, 36, doc("edge", 63), 36])   # shards 0 2 0 2 ...
    assert n.matches_batch(*args(b)) == want_matches(b)
    for W in (16, 160):
        assert n.snippets_batch(*args(b), W) == want_snippets(b, W)
    assert n.snippets_batch([], [], 64) == [] and n.matches_batch([b"alpha"], [[]]) == [[]]
    assert n.matches_batch([b"AND", b"alpha"], [[0, N_DOCS - 1], [N_DOCS - 1]]) == \
        [[[], []], [exp_matches((b"alpha",), N_DOCS - 1)]]
    for call in (lambda: n.matches_batch([b"alpha"], [[0, N_DOCS]]),
                 lambda: n.snippets_batch([b"alpha"], [[N_DOCS]], 64)):
        with pytest.raises(L.TfidfError) as e:
            call()
        assert e.value.code == L.E_INVALID_ARG
    n.close()


# 9. Worker.search_snippets_batch
def test_worker_search_snippets_batch(lucene_fixture):
    w = Worker()
    texts = [d["text"].encode() for d in lucene_fixture["docs"]]
    w.index.add_documents(texts, [d["name"].encode() for d in lucene_fixture["docs"]])
    w.commit()
    queries = ["fast food", "best wireless earbuds", "AND broken", "kheder", "zzzznothing", "fast food"]

    def single(q, k, W):
        try:
            return w.search_snippets(q, k=k, max_bytes=W)
        except L.TfidfError:
            return []                                               # a failing request yields []
    for k, W in ((5, 48), (2, 160), (10, 16)):
        got = w.search_snippets_batch(queries, k=k, max_bytes=W)
        assert got == [single(q, k, W) for q in queries]
        assert got[2] == [] and got[4] == [] and got[0] and got[0] == got[5] and got[0][0]["matches"]
    w.close()
