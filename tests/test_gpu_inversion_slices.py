"""Sliced tiles and the split row scan (csrc/commit_plan.h slice_plan): when few
blocks are inverted, a (block, range) tile's documents are cut into slices (one
workgroup each, k_df_partial<true> / k_scatter_part<true>) and a block row's
columns into parts (k_row_scan_parts).  tfidf_commit_inversion_shape says which
shape the last commit ran in; TFIDF_TEST_INV_SLICES / TFIDF_TEST_SCAN_PARTS
force either number.  The published index must be the same under every shape.

Every case is compared two ways, bit for bit: with the CPU oracle, and with a
fresh one-commit index of the same documents built under TFIDF_TEST_INV_SLICES=1
TFIDF_TEST_SCAN_PARTS=1 (the unsliced kernels), which is itself held to the
oracle: tfidf_stats, df of every word, all hits (k = 0) and the top 10 of every
word and a few multi-word queries, doc_terms / doc_len of the inverted blocks'
documents and of a sample of the kept ones (the helpers of
test_gpu_incremental_inversion).  The references are computed once per document
list.  Documents are 3-6 words over <= 400 words, as there.
"""
import os
import random

import pytest

from oracle import oracle as O
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_incremental_commit import add, keyed, published
from test_gpu_incremental_inversion import BLOCK, DOCS, ESC_DOC, TEXTS, Expect
from test_gpu_parity import assert_hits_equal

pytestmark = pytest.mark.gpu

KNOBS = ("TFIDF_TEST_INV_SLICES", "TFIDF_TEST_SCAN_PARTS")
_ref = {}


def unsliced(fn):
    """fn() under TFIDF_TEST_INV_SLICES=1 TFIDF_TEST_SCAN_PARTS=1; the environment is put back."""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ[k] = "1"
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def ref(docs, extra_queries=(), **ctor):
    """The oracle's answers for `docs` and a fresh unsliced index's stats (Expect checks that index against the oracle)."""
    key = (len(docs), hash(tuple(docs[-400:])), tuple(extra_queries), tuple(sorted(ctor.items())))
    if key not in _ref:
        _ref[key] = unsliced(lambda: Expect(docs, extra_queries, **ctor))
    return _ref[key]


def force(monkeypatch, slices=None, parts=None):
    for k, v in zip(KNOBS, (slices, parts)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def commit_check(g, docs, first_block, shape, remapped=0, extra_queries=(), rows=True, **ctor):
    """Commit, then: which blocks, which shape, and everything else against the references."""
    g.commit()
    n_blocks = (len(docs) + BLOCK - 1) // BLOCK
    assert g.commit_inverted_blocks() == {"first_block": first_block, "n_blocks": n_blocks, "remapped": remapped}
    got = g.commit_inversion_shape()
    want = dict(zip(("slices", "scan_parts"), shape))
    assert {k: got[k] for k in want if want[k] is not None} == {k: v for k, v in want.items() if v is not None}, got
    ref(docs, extra_queries, **ctor).check(g, first_block, rows=rows)
    return got


def twice(docs, **ctor):
    g = ShardIndex(**ctor)
    add(g, docs)
    g.commit()
    g.commit()
    return g


# ---------------------------------------------------------------------------
# tails of 1 .. 316 added documents behind 16 500 (the tail block holds 116 more), each under another forced
# slice count (2 slices of 96 .. 32 of 48 .. 400 slices of which most are empty); SCAN_PARTS=4 on a row of < 16 384
# columns.  log2 10: R = 1, the range is 1024 slots; 17: R = 2; 19: R = 8.

TAILS = [(10, 1, 2, None), (10, 63, 3, 4), (10, 64, 7, None), (10, 65, 32, 4), (10, 193, 400, None), (10, 316, 2, 2),
         (17, 1, 400, 4), (17, 63, 32, None), (17, 64, 2, 4), (17, 65, 3, None), (17, 193, 7, 4), (17, 316, 32, None),
         (19, 316, 7, 4)]


@pytest.mark.parametrize("log2,tail,slices,parts", TAILS)
def test_incremental_tail_under_forced_slices(monkeypatch, log2, tail, slices, parts):
    ctor = dict(vocab_capacity_log2=log2)
    g = twice(DOCS[:16500], **ctor)
    docs = DOCS[:16500 + tail]
    add(g, docs[16500:])
    force(monkeypatch, slices, parts)
    shape = (min(slices, 256), parts or 1)
    commit_check(g, docs, 2, shape, **ctor)                          # blocks 0 and 1 kept, the tail block in slices
    commit_check(g, docs, 2, shape, rows=False, **ctor)              # the other snapshot
    g.close()


def test_plan_slices_a_lone_tail_block_by_itself():
    g = twice(DOCS[:16500])
    docs = DOCS[:16900]                                              # tail block: 516 documents
    add(g, docs[16500:])
    got = commit_check(g, docs, 2, (None, 1))                        # no knob: the plan's own choice
    assert got["slices"] > 1, got
    commit_check(g, docs, 2, (got["slices"], 1), rows=False)
    g.close()


def test_nothing_added_on_a_partial_tail(monkeypatch):
    g = twice(DOCS[:16500])
    force(monkeypatch, 3, 4)
    commit_check(g, DOCS[:16500], 2, (3, 4))                         # the 116-document tail again: 2 slices + 1 empty
    force(monkeypatch)
    commit_check(g, DOCS[:16500], 2, (1, 1), rows=False)             # 116 documents, 400 columns: the plan leaves them whole
    g.close()


def test_nothing_added_on_an_exact_multiple_of_the_block(monkeypatch):
    g = twice(DOCS[:2 * BLOCK])
    force(monkeypatch, 7, 4)
    commit_check(g, DOCS[:2 * BLOCK], 2, (1, 1))                     # no block to invert: no tile kernel, no row scan
    add(g, DOCS[2 * BLOCK:2 * BLOCK + 1])
    commit_check(g, DOCS[:2 * BLOCK + 1], 2, (7, 4))                 # a one-document block: six empty slices
    g.close()


def test_fresh_three_block_build_under_forced_slices(monkeypatch):
    force(monkeypatch, 7, 4)
    g = ShardIndex()
    docs = DOCS[:16700]
    add(g, docs)
    commit_check(g, docs, 0, (7, 4))                                 # 3 blocks x 4 ranges x 7 slices; the last block partial
    g.close()


def test_dead_documents_under_forced_slices(monkeypatch):
    g = twice(DOCS[:16700])
    dead = [DOCS[i][0] for i in (5, 8191, 8192, 9000, 16650)]
    assert g.delete_documents(dead) == len(dead)
    docs = [d for d in DOCS[:16700] if d[0] not in set(dead)]
    force(monkeypatch, 32, 4)
    g.commit()                                                       # a full build through live_map
    assert g.commit_inverted_blocks() == {"first_block": 0, "n_blocks": 3, "remapped": 0}
    assert g.commit_inversion_shape() == {"slices": 32, "scan_parts": 4}
    e = ref(docs)
    drop = ("text_bytes", "dead_docs", "dead_bytes")                 # the fresh index never held the dead text
    assert {k: v for k, v in published(g).items() if k not in drop} == {k: v for k, v in e.stats.items() if k not in drop}
    e.check(g, 0, stats=False)
    g.close()


def test_long_segments_escapes_and_new_terms_in_a_sliced_block(monkeypatch):
    """log2 10: one range of 1024 slots, so a document of 150 distinct words has more than 64 entries in its
    segment and its tail goes through the long-segment reservation (one in each slice, so several workgroups
    reserve in the same streams); tf 600 escapes the temp word's 9-bit field, tf 2100 and 2500 the posting's (two
    entries, in different slices: the sorted escape list decides their scores).  "zq", "tail" and "head" are new
    terms, so the kept rows are remapped while the tail is sliced."""
    ctor = dict(vocab_capacity_log2=10)
    rng = random.Random(77)
    long_doc = lambda: b" ".join(synth.word(j) for j in rng.sample(range(1, 401), 150))
    tail = list(TEXTS[16500:16700])
    for at in (3, 50, 100, 150, 199):
        tail[at] = long_doc()
    tail[10] = b"zq " * 600
    tail[60] = ESC_DOC + b"tail"
    tail[170] = b"head " + b"zq " * 2500
    docs = DOCS[:16500] + keyed(tail, 16500)
    extra = [b"zq", b"zq tail", b"head zq", b"head"]
    g = twice(DOCS[:16500], **ctor)
    add(g, docs[16500:])
    force(monkeypatch, 7, 2)                                         # 316 documents in slices of 48
    commit_check(g, docs, 2, (7, 2), remapped=1, extra_queries=extra, **ctor)
    assert g.doc_terms(16510) == {b"zq": 600} and g.doc_terms(16670) == {b"head": 1, b"zq": 2500}
    assert sorted(d for d, _ in g.search(b"zq", 0)) == [16510, 16560, 16670]
    force(monkeypatch, 3, None)
    commit_check(g, docs, 2, (3, 1), remapped=1, extra_queries=extra, rows=False, **ctor)   # the other snapshot
    commit_check(g, docs, 2, (3, 1), extra_queries=extra, rows=False, **ctor)               # nothing new: no remap
    g.close()


# ---------------------------------------------------------------------------
# The row scan in parts by the plan's own choice: 33 203 terms (not a multiple of 16), so a row has three parts;
# two blocks in a fresh build (block 0's row total, left by its last part, is block 1's base), then the tail block
# alone.  Every word as a query would take minutes: df of every word, and the hits of a seeded 300, the common
# words and the byte-wise last word.

def _wide():
    if "wide" not in _ref:
        rare = lambda i: b" ".join(synth.word(1000 + 4 * i + j) for j in range(4))
        texts = [rare(i) + b" " + synth.word(1 + i % 50) + b" " + synth.word(60 + i % 3) for i in range(8300)]
        texts += [synth.word(1 + i % 50) + b" " + synth.word(1000 + 7 * i) for i in range(60)]      # no new word
        docs = keyed(texts)
        o = O.OracleIndex()
        for k, t in docs[:8300]:
            o.add_doc(k, t)
        o.commit()
        o2 = O.OracleIndex()
        for k, t in docs:
            o2.add_doc(k, t)
        o2.commit()
        _ref["wide"] = (docs, o, o2)
    return _ref["wide"]


def _check_wide(g, o, n_docs):
    vocab = o.vocab()
    assert len(vocab) > 33000 and len(vocab) % 16
    s = g.stats()
    assert (s["num_docs"], s["doc_count"], s["sum_ttf"], s["num_terms"], s["nnz"]) == \
        (n_docs, o.doc_count, o.sum_ttf, o.num_terms, sum(vocab.values()))
    for t, df in vocab.items():
        assert g.df(t) == (df, df), t
    words = sorted(vocab)
    qs = random.Random(5).sample(words, 300) + [words[0], words[-1]] + [synth.word(j) for j in (1, 50, 60, 62)]
    qs += [words[-1] + b" " + synth.word(1), synth.word(60) + b" " + synth.word(2)]
    for q in qs:
        for k in (0, 10):
            assert_hits_equal(g.search(q, k), o.search(q, k))
    for d in list(range(BLOCK - 20, min(BLOCK + 120, n_docs))) + random.Random(6).sample(range(BLOCK), 100):
        assert g.doc_terms(d) == o.doc_terms(d), d
        assert g.doc_len(d) == (o.doc_len(d), o.doc_norm(d)), d


def test_row_scan_in_three_parts_by_the_plan():
    docs, o, o2 = _wide()
    ctor = dict(vocab_capacity_log2=17)
    f = unsliced(lambda: _fresh(docs[:8300], ctor))
    try:
        assert f.commit_inversion_shape() == {"slices": 1, "scan_parts": 1}
        _check_wide(f, o, 8300)                                     # the unsliced reference against the oracle
        want = published(f)
    finally:
        f.close()
    g = _fresh(docs[:8300], ctor)
    assert g.commit_inverted_blocks() == {"first_block": 0, "n_blocks": 2, "remapped": 0}
    assert g.commit_inversion_shape()["scan_parts"] == 3
    assert published(g) == want
    _check_wide(g, o, 8300)
    g.commit()                                                       # the other snapshot's first build
    add(g, docs[8300:])
    g.commit()
    assert g.commit_inverted_blocks() == {"first_block": 1, "n_blocks": 2, "remapped": 0}
    assert g.commit_inversion_shape()["scan_parts"] == 3            # the tail block's row alone
    _check_wide(g, o2, len(docs))
    g.close()


def _fresh(docs, ctor):
    g = ShardIndex(**ctor)
    add(g, docs)
    g.commit()
    return g
