"""Document lifecycle on the GPU: tfidf_delete_docs, tfidf_compact (the
k_compact_text gather copy), tfidf_set_compact_threshold and tfidf_doc_text.

Expected results come from the CPU oracle built over the surviving documents
only; a compacted index must also equal, bit for bit, an index that deleted and
committed without compacting (the parent's live_map path).
"""
import functools
import os
import struct
import threading

import numpy as np
import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

pytestmark = pytest.mark.gpu


def f32bits(x):
    return np.float32(x).view(np.int32).item()


def bits(hits):
    return [(d, f32bits(s)) for d, s in hits]


# what an index holds; the path statistics (long_docs, pack_docs, ...) follow the corpus layout:
# which tokenizer path a ~4 KB document takes depends on where it lies in the buffer
RESULT_STATS = ("num_docs", "doc_count", "sum_ttf", "num_terms", "nnz", "malformed_docs")


def result_stats(g):
    s = g.stats()
    return {k: s[k] for k in RESULT_STATS}


def oracle_of(keys, texts):
    o = O.OracleIndex()
    for k, t in zip(keys, texts):
        o.add_doc(k, t)
    o.commit()
    return o


# ---------------------------------------------------------------------------
# 1. the edge corpus

LENGTHS = [0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095,
           4096, 4097, 20000, 70000]
N_EDGE = 400
WORDS = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"iota", b"kappa", b"lambda"]


def edge_doc(i, n):
    """n bytes: the document's own number, then words of a small shared vocabulary."""
    parts, size, j = [b"n%d" % i], len(b"n%d" % i), i
    while size < n:
        w = WORDS[j % len(WORDS)]
        parts.append(b" " if j % 13 else b"\n")
        parts.append(w)
        size += 1 + len(w)
        j += 1 + (i % 3)
    return b"".join(parts)[:n]


@functools.lru_cache(maxsize=None)
def edge_corpus():
    keys = [b"edge/%04d.txt" % i for i in range(N_EDGE)]
    texts = [edge_doc(i, LENGTHS[i % len(LENGTHS)]) for i in range(N_EDGE)]
    assert [len(t) for t in texts] == [LENGTHS[i % len(LENGTHS)] for i in range(N_EDGE)]
    return keys, texts


PATTERNS = {
    "none": lambda i: False,
    "first": lambda i: i == 0,
    "last": lambda i: i == N_EDGE - 1,
    "every_other": lambda i: i % 2 == 0,
    "block_100": lambda i: 150 <= i < 250,
    "all_but_one": lambda i: i != 123,
    "all": lambda i: True,
}


def run_table(lengths, dead):
    """The runs of csrc/compact_plan.h, computed naively: (src, dst, len)."""
    runs, src, dst, open_ = [], 0, 0, False
    for n, d in zip(lengths, dead):
        if d:
            open_ = False
        elif n:
            if open_:
                runs[-1][2] += n
            else:
                runs.append([src, dst, n])
            open_ = True
            dst += n
        src += n
    return runs


def test_edge_input_reaches_every_copy_path():
    """CPU-side conditions on the "every other" input: every (src - dst) mod 16,
    a run shorter than a chunk, and a 16-byte destination chunk holding three
    or more runs (so the slow path walks several runs)."""
    lengths = [LENGTHS[i % len(LENGTHS)] for i in range(N_EDGE)]
    runs = run_table(lengths, [PATTERNS["every_other"](i) for i in range(N_EDGE)])
    assert {(s - d) % 16 for s, d, _ in runs} == set(range(16))           # (a)
    assert any(n < 16 for _, _, n in runs)                                # (b)
    per_chunk = {}
    for _, d, n in runs:
        for c in range(d // 16, (d + n - 1) // 16 + 1):
            per_chunk[c] = per_chunk.get(c, 0) + 1
    assert max(per_chunk.values()) >= 3                                   # (c)
    # tile edges: with 1 KiB tiles some run starts strictly inside a tile, some run spans tiles
    assert any(d % 1024 for _, d, _ in runs) and any(d // 1024 != (d + n - 1) // 1024 for _, d, n in runs)


QUERIES = [b"alpha", b"beta gamma", b"n17", b"n399 theta", b"kappa iota eta", b"n0", b"n123", b"n200 lambda",
           b"zeta AND delta", b"missing"]


@functools.lru_cache(maxsize=None)
def edge_expected(pattern):
    """The oracle over the survivors of a pattern: computed once, shared."""
    keys, texts = edge_corpus()
    live = [i for i in range(N_EDGE) if not PATTERNS[pattern](i)]
    o = oracle_of([keys[i] for i in live], [texts[i] for i in live])
    n = len(live)
    sample = sorted(set(list(range(0, n, 7)) + list(range(min(n, 4))) + list(range(max(0, n - 4), n))))
    exp = {
        "live": live,
        "keys": [o.doc_key(d) for d in range(n)],
        "stats": {"num_docs": o.num_docs, "doc_count": o.doc_count, "sum_ttf": o.sum_ttf, "num_terms": o.num_terms,
                  "nnz": sum(o.vocab().values())},
        "sample": sample,
        "terms": {d: o.doc_terms(d) for d in sample},
        "lens": {d: (o.doc_len(d), o.doc_norm(d)) for d in sample},
        "all": [bits(o.search(q, 0)) for q in QUERIES],
        "top": [bits(o.search(q, 10)) for q in QUERIES],
    }
    o.close()
    return exp


def keys_of(g):
    blob, offs = g.doc_keys()
    b = blob.tobytes()
    return [b[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def observe(g, exp):
    """Everything the test compares, read from an index."""
    n = g.stats()["num_docs"]
    got = {
        "keys": keys_of(g),
        "text": [g.doc_text(d) for d in range(n)],
        "terms": {d: g.doc_terms(d) for d in exp["sample"]},
        "lens": {d: g.doc_len(d) for d in exp["sample"]},
        "all": [bits(g.search(q, 0)) for q in QUERIES],
        "top": [bits(g.search(q, 10)) for q in QUERIES],
        "batch_all": [bits(h) for h in g.search_batch_all(QUERIES)],
    }
    docs, scores, counts = g.search_batch(QUERIES, 10)
    got["batch_top"] = [bits(zip(docs[i, :counts[i]].tolist(), scores[i, :counts[i]].tolist()))
                        for i in range(len(QUERIES))]
    return got


@pytest.mark.parametrize("tile_log2", [None, "10"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_edge_corpus_bytes_and_parity(pattern, tile_log2, monkeypatch):
    if tile_log2:
        monkeypatch.setenv("TFIDF_COMPACT_TILE_LOG2", tile_log2)
    keys, texts = edge_corpus()
    exp = edge_expected(pattern)
    dead = [i for i in range(N_EDGE) if PATTERNS[pattern](i)]
    live_bytes = sum(len(texts[i]) for i in exp["live"])
    dead_bytes = sum(len(texts[i]) for i in dead)

    g, h = ShardIndex(), ShardIndex()            # g compacts, h commits through live_map as the parent does
    for x in (g, h):
        x.add_documents(texts, keys)
        assert x.delete_documents([keys[i] for i in dead]) == len(dead)
        s = x.stats()
        assert (s["dead_docs"], s["dead_bytes"], s["compactions"]) == (len(dead), dead_bytes, 0)
        assert s["text_bytes"] == live_bytes + dead_bytes
    r = g.compact()
    assert r["bytes_reclaimed"] == dead_bytes
    assert g.compact() == {"bytes_reclaimed": 0, "ms_device": 0.0}      # nothing dead: a no-op
    g.commit()
    h.commit()
    sg, sh = g.stats(), h.stats()
    assert (sg["dead_docs"], sg["dead_bytes"], sg["text_bytes"]) == (0, 0, live_bytes)
    assert sg["compactions"] == (1 if dead else 0)
    assert (sh["dead_docs"], sh["dead_bytes"], sh["text_bytes"], sh["compactions"]) == \
        (len(dead), dead_bytes, live_bytes + dead_bytes, 0)
    assert {k: sg[k] for k in exp["stats"]} == exp["stats"]
    assert result_stats(g) == result_stats(h)
    if dead_bytes >= 2 << 20:
        assert sg["device_bytes"] < sh["device_bytes"]

    got = observe(g, exp)
    assert got["text"] == [texts[i] for i in exp["live"]]
    assert got["keys"] == exp["keys"] == [keys[i] for i in exp["live"]]
    assert got["terms"] == exp["terms"]
    assert got["lens"] == exp["lens"]
    assert got["all"] == exp["all"] == got["batch_all"]
    assert got["top"] == exp["top"] == got["batch_top"]
    assert observe(h, exp) == got
    g.close()
    h.close()


# ---------------------------------------------------------------------------
# 2. delete semantics

def test_delete_semantics_keyed():
    texts = [b"red apple", b"green pear", b"red plum", b"blue berry", b"green apple"]
    keys = [b"a", b"b", b"c", b"d", b"e"]
    g = ShardIndex()
    g.add_documents(texts, keys)
    g.commit()
    assert g.delete_documents([]) == 0
    assert g.delete_documents([b"nope", b"", b"7"]) == 0                  # unknown keys: no error, not counted
    assert g.delete_documents([b"c", b"c", b"nope", b"a"]) == 2          # a key given twice counts once
    assert g.delete_documents([b"c"]) == 0                                # already dead
    # invisible until the commit
    assert [g.doc_key(d) for d, _ in g.search(b"red", 0)] == [b"a", b"c"]
    assert g.stats()["num_docs"] == 5 and g.stats()["dead_docs"] == 2
    g.commit()
    assert g.search(b"red", 0) == [] and g.stats()["num_docs"] == 3
    assert keys_of(g) == [b"b", b"d", b"e"]
    # a deleted key is forgotten: adding it again appends at the end
    g.add_documents([b"red cherry"], [b"a"])
    g.commit()
    assert keys_of(g) == [b"b", b"d", b"e", b"a"]
    o = oracle_of([b"b", b"d", b"e", b"a"], [texts[1], texts[3], texts[4], b"red cherry"])
    for q in (b"red", b"green apple", b"cherry"):
        assert bits(g.search(q, 0)) == bits(o.search(q, 0))
    # replace-by-key then delete: the replacement dies, the replaced one stays dead
    g.add_documents([b"red fig"], [b"b"])
    assert g.delete_documents([b"b"]) == 1
    g.commit()
    assert keys_of(g) == [b"d", b"e", b"a"]
    o.close()
    g.close()


def test_delete_and_compact_keep_keyless_ordinals():
    texts = [b"doc number %d word%d" % (i, i) for i in range(10)]
    g = ShardIndex()
    g.add_documents(texts)                                               # keys "0" .. "9"
    g.commit()
    assert keys_of(g) == [b"%d" % i for i in range(10)]
    assert g.delete_documents([b"3", b"03", b"3 ", b"+3", b"10", b"9", b"3"]) == 2   # canonical decimals only
    g.commit()
    assert keys_of(g) == [b"0", b"1", b"2", b"4", b"5", b"6", b"7", b"8"]
    assert g.compact()["bytes_reclaimed"] == len(texts[3]) + len(texts[9])
    g.commit()
    assert keys_of(g) == [b"0", b"1", b"2", b"4", b"5", b"6", b"7", b"8"]      # keys never change
    assert [g.doc_text(d) for d in range(8)] == [texts[i] for i in (0, 1, 2, 4, 5, 6, 7, 8)]
    g.add_documents([b"fresh one", b"fresh two"])                        # never reuse a reclaimed number
    g.commit()
    assert keys_of(g)[-2:] == [b"10", b"11"]
    assert g.delete_documents([b"9", b"3"]) == 0                         # reclaimed ordinals name nothing
    assert g.delete_documents([b"4", b"10"]) == 2                        # after a compaction: by ordinal, not position
    g.compact()
    g.add_documents([b"fresh three"])
    g.commit()
    assert keys_of(g) == [b"0", b"1", b"2", b"5", b"6", b"7", b"8", b"11", b"12"]
    assert g.doc_text(3) == texts[5] and g.doc_text(8) == b"fresh three"
    # explicit keys are looked up first; a keyed document is not addressed by its ordinal
    g.add_documents([b"keyed thirteen", b"keyed named seven"], [b"k", b"7"])   # ordinals 13, 14
    assert g.delete_documents([b"13"]) == 0
    assert g.delete_documents([b"7"]) == 1                               # the explicit key "7", not the keyless 7
    g.commit()
    assert keys_of(g) == [b"0", b"1", b"2", b"5", b"6", b"7", b"8", b"11", b"12", b"k"]
    assert g.doc_text(5) == texts[7]
    g.close()


def test_doc_text_buffer_protocol():
    lib = L.load()
    g = ShardIndex()
    g.add_documents([b"hello world", b""], [b"x", b"empty"])
    g.commit()
    n = L.C.c_uint64()
    buf = L.C.create_string_buffer(4)
    assert lib.tfidf_doc_text(g._h, 0, buf, 4, L.C.byref(n)) == L.E_BUFFER and n.value == 11
    assert lib.tfidf_doc_text(g._h, 2, buf, 4, L.C.byref(n)) == L.E_INVALID_ARG
    assert g.doc_text(0) == b"hello world" and g.doc_text(1) == b""
    with g.reader() as rd:
        assert lib.tfidf_reader_doc_text(rd._h, 0, buf, 4, L.C.byref(n)) == L.E_BUFFER and n.value == 11
        assert rd.doc_text(0) == b"hello world" and rd.doc_text(1) == b""
    g.close()


# ---------------------------------------------------------------------------
# 3. readers are pinned

def test_reader_is_pinned_across_delete_compact_commit():
    texts = synth.corpus(600, V=3000, len_min=20, len_max=90)
    keys = [b"p%04d" % i for i in range(600)]
    qs = synth.queries(8, lo=1, hi=600) + [b"aaaa"]
    g = ShardIndex()
    g.add_documents(texts, keys)
    g.commit()
    rd = g.reader()
    before = ([bits(rd.search(q, 0)) for q in qs], [bits(rd.search(q, 10)) for q in qs],
              [rd.doc_key(d) for d in range(600)], [rd.doc_text(d) for d in range(600)])
    assert before[3] == texts
    dead = list(range(0, 600, 3))
    assert g.delete_documents([keys[i] for i in dead]) == 200
    assert g.compact()["bytes_reclaimed"] == sum(len(texts[i]) for i in dead)
    more = synth.corpus(50, V=3000, len_min=20, len_max=90, doc_base=9000)
    mkeys = [b"q%04d" % i for i in range(50)]
    g.add_documents(more, mkeys)            # lands in the new buffers, over the offsets the reader's text had
    g.commit()
    after = ([bits(rd.search(q, 0)) for q in qs], [bits(rd.search(q, 10)) for q in qs],
             [rd.doc_key(d) for d in range(600)], [rd.doc_text(d) for d in range(600)])
    assert after == before
    assert rd.num_docs == 600
    rd.close()
    live = [i for i in range(600) if i % 3]
    o = oracle_of([keys[i] for i in live] + mkeys, [texts[i] for i in live] + more)
    assert g.stats()["num_docs"] == o.num_docs == 450
    assert [g.doc_text(d) for d in range(450)] == [texts[i] for i in live] + more
    for q in qs:
        assert bits(g.search(q, 0)) == bits(o.search(q, 0))
    o.close()
    g.close()


# ---------------------------------------------------------------------------
# 4. recovery from a failed commit

def test_delete_recovers_a_failed_commit():
    good = [b"fine words here %d" % (i % 7) for i in range(40)]
    gkeys = [b"good%02d" % i for i in range(40)]
    # 3 offenders with 400 distinct terms each: more than 1024 in all
    bad = [b" ".join(b"t%dx%d" % (j, i) for i in range(400)) for j in range(3)]
    bkeys = [b"bad%d" % j for j in range(3)]
    g = ShardIndex(vocab_capacity_log2=10)
    g.add_documents(good[:20], gkeys[:20])
    g.commit()
    g.add_documents(bad, bkeys)
    g.add_documents(good[20:], gkeys[20:])
    with pytest.raises(L.TfidfError) as e:
        g.commit()
    assert e.value.code == L.E_CAPACITY
    assert g.stats()["num_docs"] == 20                                   # the last commit still serves
    assert g.delete_documents(bkeys) == 3
    g.commit()
    o = oracle_of(gkeys, good)
    qs = [b"fine", b"words 3", b"here 6 5", b"t1x7"]
    want = [bits(o.search(q, 0)) for q in qs]
    assert [bits(g.search(q, 0)) for q in qs] == want
    assert keys_of(g) == gkeys and g.stats()["num_docs"] == o.num_docs == 40
    assert (g.stats()["doc_count"], g.stats()["sum_ttf"], g.stats()["num_terms"]) == \
        (o.doc_count, o.sum_ttf, o.num_terms)
    # the header's other path: clear, add the survivors, commit
    g.clear()
    g.add_documents(good, gkeys)
    g.commit()
    assert [bits(g.search(q, 0)) for q in qs] == want and keys_of(g) == gkeys
    o.close()
    g.close()


# ---------------------------------------------------------------------------
# 5. persistence

HEADER = struct.Struct("<8sIIffiiII5Q")      # FileHeader of tfidf_save


def test_persistence_after_replace_delete_compact(tmp_path):
    texts = synth.corpus(500, V=4000, len_min=20, len_max=120)
    keys = [b"f%03d.txt" % (i % 420) for i in range(500)]                # 80 replaced
    g = ShardIndex()
    g.add_documents(texts, keys)
    assert g.delete_documents([b"f%03d.txt" % i for i in range(100, 160)]) == 60
    g.commit()
    before, after = str(tmp_path / "before.idx"), str(tmp_path / "after.idx")
    g.save(before)
    # never compacted: the parent's version-1 layout, field by field
    raw = open(before, "rb").read()
    hd = HEADER.unpack_from(raw)
    key_bytes = sum(len(k) for k in keys)
    text_bytes = sum(len(t) for t in texts)
    assert hd[0] == b"TFIDFIX1" and hd[1] == 1 and hd[2] == 0
    assert (hd[3], hd[4], hd[5], hd[6], hd[7], hd[8]) == (np.float32(1.2), np.float32(0.75), 0, 0, 18, 0)
    assert hd[9:13] == (500, text_bytes, key_bytes, 140)
    assert len(raw) == HEADER.size + 2 * 501 * 8 + key_bytes + 2 * 500 + text_bytes
    offs = np.frombuffer(raw, np.uint64, 501, HEADER.size)
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in texts])]).tolist()
    live = np.frombuffer(raw, np.uint8, 500, HEADER.size + 2 * 501 * 8 + key_bytes + 500)
    dead = set(range(80)) | {i for i in range(500) if 100 <= i % 420 < 160}
    assert live.tolist() == [0 if i in dead else 1 for i in range(500)]
    assert raw[len(raw) - text_bytes:] == b"".join(texts)

    reclaimed = g.compact()["bytes_reclaimed"]
    assert reclaimed == sum(len(texts[i]) for i in dead)
    g.commit()
    g.save(after)
    assert os.path.getsize(after) <= os.path.getsize(before) - reclaimed
    assert HEADER.unpack_from(open(after, "rb").read(HEADER.size))[1] == 1   # keyed documents: still version 1
    qs = synth.queries(10, lo=1, hi=800)
    for path in (before, after):
        h = ShardIndex()
        h.load(path)
        h.commit()
        assert result_stats(h) == result_stats(g)
        assert keys_of(h) == keys_of(g)
        assert [h.doc_text(d) for d in range(360)] == [g.doc_text(d) for d in range(360)]
        for q in qs:
            assert bits(h.search(q, 0)) == bits(g.search(q, 0))
        h.close()
    h = ShardIndex()
    h.load(after)
    assert (h.stats()["dead_docs"], h.stats()["text_bytes"]) == (0, text_bytes - reclaimed)
    h.close()
    g.close()


def test_persistence_round_trips_keyless_ordinals(tmp_path):
    texts = [b"keyless %d body%d" % (i, i) for i in range(12)]
    g = ShardIndex()
    g.add_documents(texts)
    v1 = str(tmp_path / "v1.idx")
    g.save(v1)
    assert HEADER.unpack_from(open(v1, "rb").read(HEADER.size))[1] == 1
    assert g.delete_documents([b"2", b"5", b"11"]) == 3
    g.compact()
    g.commit()
    v2 = str(tmp_path / "v2.idx")
    g.save(v2)
    assert HEADER.unpack_from(open(v2, "rb").read(HEADER.size))[1] == 2     # ordinals differ from positions
    h = ShardIndex()
    h.load(v2)
    h.add_documents([b"after reload"])                                    # ordinal 12: 11 is not reused
    h.commit()
    assert keys_of(h) == [b"%d" % i for i in (0, 1, 3, 4, 6, 7, 8, 9, 10, 12)]
    assert h.doc_text(2) == texts[3] and h.doc_text(9) == b"after reload"
    assert h.delete_documents([b"5", b"6"]) == 1
    h.close()
    k = ShardIndex()
    k.load(v1)                                                            # version-1 files still load
    k.commit()
    assert keys_of(k) == [b"%d" % i for i in range(12)]
    k.close()
    g.close()


# ---------------------------------------------------------------------------
# 6. the commit-time threshold

def test_compact_threshold():
    base = synth.corpus(200, V=3000, len_min=40, len_max=80)
    keys = [b"t%03d" % i for i in range(200)]
    qs = synth.queries(6, lo=1, hi=500)
    never, auto = ShardIndex(), ShardIndex()
    auto.set_compact_threshold(20)
    for x in (never, auto):
        x.add_documents(base, keys)
        x.commit()
    state = list(base)
    trace = []
    for rnd in range(6):                      # each round replaces 20 documents: ~10 % of the base text
        new = synth.corpus(20, V=3000, len_min=40, len_max=80, doc_base=1000 + 100 * rnd)
        ks = keys[20 * rnd:20 * rnd + 20]
        for x in (never, auto):
            x.add_documents(new, ks)
        state[20 * rnd:20 * rnd + 20] = new
        # what the commit will see: dead x 100 >= 20 x staged
        s = auto.stats()
        expect_compaction = s["dead_bytes"] * 100 >= 20 * s["text_bytes"]
        c0 = s["compactions"]
        never.commit()
        auto.commit()
        s = auto.stats()
        assert s["compactions"] == c0 + (1 if expect_compaction else 0)
        if expect_compaction:
            assert s["dead_bytes"] == 0 and s["dead_docs"] == 0 and s["text_bytes"] == sum(len(t) for t in state)
        trace.append(expect_compaction)
        sn = never.stats()
        assert sn["compactions"] == 0 and sn["dead_docs"] == 20 * (rnd + 1)
        assert sn["dead_bytes"] == sn["text_bytes"] - sum(len(t) for t in state)
        assert result_stats(never) == result_stats(auto)
        assert keys_of(never) == keys_of(auto)
        for q in qs:
            assert bits(never.search(q, 0)) == bits(auto.search(q, 0))
    # dead / staged per round: 10/110, 20/120, 30/130 (compacts), then again from a dense corpus
    assert trace == [False, False, True, False, False, True]
    order = keys[120:] + keys[:120]
    o = oracle_of(order, [state[int(k[1:])] for k in order])
    for q in qs:
        assert bits(auto.search(q, 0)) == bits(o.search(q, 0))
    o.close()
    with pytest.raises(L.TfidfError):
        auto.set_compact_threshold(101)
    never.close()
    auto.close()


def test_worker_threshold_argument(tmp_path):
    from tfidf_amd.reference_api import Worker
    docs = tmp_path / "documents"
    docs.mkdir()
    (docs / "a.txt").write_bytes(b"first version of the file")
    (docs / "b.txt").write_bytes(b"another file")
    plain = Worker(str(docs), str(tmp_path / "ix1"))
    auto = Worker(str(docs), str(tmp_path / "ix2"), compact_threshold_pct=10)
    for w in (plain, auto):
        w.init()
    for w in (plain, auto):
        assert w.upload("a.txt", b"second version of the file, longer than the first")[0] == 200
    assert plain.index.stats()["compactions"] == 0 and plain.index.stats()["dead_docs"] == 1
    assert auto.index.stats()["compactions"] == 1 and auto.index.stats()["dead_docs"] == 0
    assert plain.process_documents("version file") == auto.process_documents("version file")
    plain.close()
    auto.close()


# ---------------------------------------------------------------------------
# 7. above 4 GiB

def test_compact_above_4_gib():
    """Offsets past 2^32 in source and destination.  cfg-2 document lengths;
    the corpus is generated on the device, keyless."""
    n_docs = 1_800_000                       # ~2470 bytes each: ~4.4e9 bytes
    dc = synth.DeviceCorpus(n_docs)
    assert dc.total_bytes > (1 << 32) + (64 << 20)
    g = ShardIndex()
    g.add_documents_device(dc.d_text, dc.d_offsets, n_docs, dc.total_bytes)
    offs = np.zeros(n_docs + 1, np.uint64)
    synth._d2h(offs, dc.d_offsets, (n_docs + 1) * 8)
    dc.free()
    dead = [3, 4, 1000, 77777]
    assert g.delete_documents([b"%d" % d for d in dead]) == 4
    r = g.compact()
    assert r["bytes_reclaimed"] == sum(int(offs[d + 1] - offs[d]) for d in dead)
    g.commit()
    assert g.stats()["num_docs"] == n_docs - 4
    line = int(np.searchsorted(offs, np.uint64(1 << 32)))                # first document past the 4 GiB line
    cdf = synth.zipf_cdf(100_000)
    for old in (0, 2, 5, 999, 1001, 77778, line - 6, line - 5, line - 4, line, line + 1, n_docs - 1):
        new = old - sum(1 for d in dead if d < old)
        assert g.doc_key(new) == b"%d" % old
        assert g.doc_text(new) == synth.doc_text(synth.SEED, old, 400, 600, cdf), old
    g.close()


# ---------------------------------------------------------------------------
# 8. searching beside a writer

def test_searches_beside_replace_delete_compact_commit():
    n, r = 800, 100
    base = synth.corpus(n, V=3000, len_min=20, len_max=90)
    alt = synth.corpus(r, V=3000, len_min=20, len_max=90, seed=4242)
    keys = [b"w%04d" % i for i in range(n)]
    qs = synth.queries(8, lo=1, hi=600) + [b"aaaa"]
    # state 0: every document, base text.  state 1: the first r replaced by alt, the next r deleted
    s1_keys = keys[:r] + keys[2 * r:]
    want = []
    for ks, ts in ((keys, base), (s1_keys, alt + base[2 * r:])):
        o = oracle_of(ks, ts)
        want.append([{o.doc_key(d): f32bits(s) for d, s in o.search(q, 0)} for q in qs])
        o.close()
    g = ShardIndex()
    g.add_documents(base, keys)
    g.commit()
    stop = threading.Event()
    errors, seen = [], [[0, 0] for _ in range(4)]

    def writer():
        try:
            for rnd in range(20):
                if rnd % 2 == 0:
                    g.add_documents(alt, keys[:r])
                    assert g.delete_documents(keys[r:2 * r]) == r
                else:
                    g.add_documents(base[:2 * r], keys[:2 * r])
                g.compact()
                g.commit()
        except Exception as e:          # noqa: BLE001
            errors.append(("writer", repr(e)))
        finally:
            stop.set()

    def searcher(t):
        i = 0
        while not stop.is_set() or i < 4:
            qi = (t + i) % len(qs)
            with g.reader() as rd:
                got = {rd.doc_key(d): f32bits(s) for d, s in rd.search(qs[qi], 0)}
            st = [s for s in (0, 1) if got == want[s][qi]]
            if not st:
                errors.append(("search", t, qi))
                return
            seen[t][st[0]] += 1
            i += 1

    th = [threading.Thread(target=searcher, args=(i,), daemon=True) for i in range(4)]
    w = threading.Thread(target=writer, daemon=True)
    for x in th:
        x.start()
    w.start()
    w.join(120)
    for x in th:
        x.join(120)
    assert not w.is_alive() and not any(x.is_alive() for x in th), "a thread did not finish"
    assert not errors, errors[:5]
    assert g.stats()["compactions"] == 20 and g.stats()["dead_docs"] == 0
    with g.reader() as rd:                   # 20 rounds: state 0 again
        assert {rd.doc_key(d): f32bits(s) for d, s in rd.search(qs[0], 0)} == want[0][0]
    g.close()
