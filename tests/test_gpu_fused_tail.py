"""A lone inverted block in one launch (k_df_fused; csrc/commit_plan.h
fuse_plan): when a commit inverts exactly one block in two or more slices, the
slices' counts go to a scratch row and the last slice of each range to finish
turns them into df, the row's offsets and the block's base, in place of
k_inv_zero, k_df_partial<true>, k_df_sum<true>, k_row_scan_parts and
k_block_scan.  tfidf_commit_inversion_fused says whether the last commit did.

Every state is compared bit for bit, as in test_gpu_incremental_inversion (its
helpers, DOCS and BLOCK), with the CPU oracle and with a fresh one-commit index
of the same documents built under TFIDF_INV_UNFUSED=1: tfidf_stats, df of every
word, all hits (k = 0) and the top 10 of every word and a few multi-word
queries, doc_terms / doc_len of the tail's documents.  Commits alternate between
two snapshots; both are committed and checked.  The accessor must say what the
rule predicts from the blocks inverted, the shape and the knobs.  The scratch is
cleaned by the kernel itself: one left dirty would double a df in the next
commit, so several cases commit again with nothing added.
"""
import os
import random

import pytest

from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_incremental_commit import add, keyed, published
from test_gpu_incremental_inversion import BLOCK, DOCS, ESC_DOC, TEXTS, Expect

pytestmark = pytest.mark.gpu

SHAPE_KNOBS = ("TFIDF_TEST_INV_SLICES", "TFIDF_TEST_SCAN_PARTS")
OFF_KNOBS = ("TFIDF_TEST_SCAN_PARTS", "TFIDF_DF_FROM_ROWS", "TFIDF_INV_UNFUSED")
_ref = {}


def ref(docs, extra_queries=(), **ctor):
    """The oracle's answers for `docs` and the stats of a fresh index built under TFIDF_INV_UNFUSED=1 with no
    forced shape (Expect holds that index to the oracle); the environment is put back."""
    key = (len(docs), hash(tuple(docs[-400:])), tuple(extra_queries), tuple(sorted(ctor.items())))
    if key not in _ref:
        names = SHAPE_KNOBS + ("TFIDF_DF_FROM_ROWS", "TFIDF_INV_UNFUSED")
        old = {k: os.environ.get(k) for k in names}
        try:
            for k in names:
                os.environ.pop(k, None)
            os.environ["TFIDF_INV_UNFUSED"] = "1"
            _ref[key] = Expect(docs, extra_queries, **ctor)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _ref[key]


def knob_on(name):
    return os.environ.get(name, "") not in ("", "0")


def predicted(g):
    """fuse_plan, from what the commit reports and the environment."""
    inv, shape = g.commit_inverted_blocks(), g.commit_inversion_shape()
    return (inv["n_blocks"] - inv["first_block"] == 1 and shape["slices"] >= 2 and
            not os.environ.get("TFIDF_TEST_SCAN_PARTS") and not knob_on("TFIDF_DF_FROM_ROWS") and
            not knob_on("TFIDF_INV_UNFUSED"))


def commit_check(g, docs, first_block, fused, remapped=0, slices=None, extra_queries=(), rows=True, stats=True, **ctor):
    g.commit()
    n_blocks = (len(docs) + BLOCK - 1) // BLOCK
    assert g.commit_inverted_blocks() == {"first_block": first_block, "n_blocks": n_blocks, "remapped": remapped}
    if slices is not None:
        assert g.commit_inversion_shape()["slices"] == slices
    assert g.commit_inversion_fused() is predicted(g)
    assert g.commit_inversion_fused() is fused, (g.commit_inversion_shape(), g.commit_inverted_blocks())
    e = ref(docs, extra_queries, **ctor)
    if stats:
        e.check(g, first_block, rows=rows)
    else:
        drop = ("text_bytes", "dead_docs", "dead_bytes")             # the fresh index never held the dead text
        assert {k: v for k, v in published(g).items() if k not in drop} == \
            {k: v for k, v in e.stats.items() if k not in drop}
        e.check(g, first_block, stats=False, rows=rows)


def twice(docs, **ctor):
    g = ShardIndex(**ctor)
    add(g, docs)
    g.commit()
    g.commit()
    return g


def force(monkeypatch, slices=None):
    if slices is None:
        monkeypatch.delenv("TFIDF_TEST_INV_SLICES", raising=False)
    else:
        monkeypatch.setenv("TFIDF_TEST_INV_SLICES", str(slices))


# ---------------------------------------------------------------------------

def test_tail_under_the_plans_own_slices():
    g = twice(DOCS[:16500])
    docs = DOCS[:16900]                                              # tail block: 516 documents
    add(g, docs[16500:])
    commit_check(g, docs, 2, True)
    assert g.commit_inversion_shape()["slices"] >= 2
    commit_check(g, docs, 2, True, rows=False)                       # the other snapshot
    g.close()


# log2 10: R = 1, the range is 1024 slots; 17: R = 2; 19: R = 8 (400 words: some ranges hold few columns).
# 400 slices: capped at 256, most of them without documents.
@pytest.mark.parametrize("log2", [10, 17, 19])
@pytest.mark.parametrize("slices,tail", [(2, 1), (7, 65), (32, 193), (400, 316)])
def test_tail_under_forced_slices(monkeypatch, log2, slices, tail):
    ctor = dict(vocab_capacity_log2=log2)
    g = twice(DOCS[:16500], **ctor)
    docs = DOCS[:16500 + tail]
    add(g, docs[16500:])
    force(monkeypatch, slices)
    commit_check(g, docs, 2, True, slices=min(slices, 256), **ctor)
    commit_check(g, docs, 2, True, slices=min(slices, 256), rows=False, **ctor)   # the other snapshot
    g.close()


def test_three_commits_that_add_nothing():
    docs = DOCS[:16900]
    g = twice(docs)
    for i in range(3):                                               # a scratch left dirty doubles a df
        commit_check(g, docs, 2, True, rows=i == 0)
    g.close()


def test_tail_filled_to_the_block_edge_then_nothing_then_one_document(monkeypatch):
    g = twice(DOCS[:16500])
    docs = DOCS[:3 * BLOCK]
    add(g, docs[16500:])
    commit_check(g, docs, 2, True, rows=False)                       # the tail block, full now: it joins the df base
    commit_check(g, docs, 2, True, rows=False)                       # the other snapshot
    commit_check(g, docs, 3, False, rows=False)                      # no block inverted
    commit_check(g, docs, 3, False, rows=False)
    docs = DOCS[:3 * BLOCK + 1]
    add(g, docs[3 * BLOCK:])
    commit_check(g, docs, 3, False, slices=1)                        # one document: the plan leaves it whole
    force(monkeypatch, 2)
    commit_check(g, docs, 3, True, slices=2)                         # the other snapshot: one slice of two has it
    commit_check(g, docs, 3, True, slices=2, rows=False)
    g.close()


def test_new_words_among_the_old_slots_in_the_same_commit(monkeypatch):
    ctor = dict(vocab_capacity_log2=10)
    rng = random.Random(50)
    fresh_words = [synth.word(1000 + j) for j in range(50)]          # absent before: 450 terms in 1024 slots
    later = [b" ".join([fresh_words[i % 50]] + [synth.word(rng.randint(1, 400)) for _ in range(rng.randint(2, 4))])
             for i in range(150)] + [fresh_words[3] + b" " + fresh_words[49]]
    base = DOCS[:16500]
    docs = base + keyed(later, 16500)
    extra = [fresh_words[0] + b" " + synth.word(7), fresh_words[49] + b" " + fresh_words[3], fresh_words[10]]
    g = twice(base, **ctor)
    force(monkeypatch, 3)
    commit_check(g, base, 2, True, slices=3, rows=False, **ctor)     # the scratch holds the old column count
    add(g, docs[16500:])
    commit_check(g, docs, 2, True, remapped=1, slices=3, extra_queries=extra, **ctor)       # more columns than before
    commit_check(g, docs, 2, True, remapped=1, slices=3, extra_queries=extra, rows=False, **ctor)
    commit_check(g, docs, 2, True, slices=3, extra_queries=extra, rows=False, **ctor)       # nothing new: no remap
    g.close()


def test_fresh_index_below_one_block(monkeypatch):
    force(monkeypatch, 7)
    g = ShardIndex()
    docs = DOCS[:3000]
    add(g, docs)
    commit_check(g, docs, 0, True, slices=7)                         # first_block 0: no base to trust, bbase[0] written
    commit_check(g, docs, 0, True, slices=7, rows=False)             # the other snapshot's first build
    docs = DOCS[:3100]
    add(g, docs[3000:])
    commit_check(g, docs, 0, True, slices=7)                         # incremental rows, the block from its first document
    g.close()


def test_posting_escapes_kept_and_rebuilt(monkeypatch):
    texts = list(TEXTS[:8400])
    texts[100] = ESC_DOC                                             # block 0
    texts[8250] = ESC_DOC + b"tail"                                  # block 1, the tail
    texts[8350] = b"head " + ESC_DOC
    docs = keyed(texts)
    extra = [b"zq", b"zq tail", b"head zq"]
    g = twice(docs[:8300])
    force(monkeypatch, 3)
    commit_check(g, docs[:8300], 1, True, slices=3, extra_queries=extra[:2])    # block 0's escape kept, the tail's rebuilt
    assert g.doc_terms(100) == {b"zq": 2100} and g.doc_terms(8250) == {b"zq": 2100, b"tail": 1}
    add(g, docs[8300:])                                              # ("head" is a new term: the kept rows move as well)
    commit_check(g, docs, 1, True, remapped=1, slices=3, extra_queries=extra)
    assert g.doc_terms(8350) == {b"head": 1, b"zq": 2100}
    assert sorted(d for d, _ in g.search(b"zq", 0)) == [100, 8250, 8350]
    commit_check(g, docs, 1, True, remapped=1, slices=3, extra_queries=extra, rows=False)
    commit_check(g, docs, 1, True, slices=3, extra_queries=extra, rows=False)
    g.close()


def test_delete_full_build_then_incremental_again(monkeypatch):
    g = twice(DOCS[:16700])
    force(monkeypatch, 32)
    commit_check(g, DOCS[:16700], 2, True, slices=32, rows=False)
    dead = [DOCS[i][0] for i in (5, 8191, 8192, 9000, 16650)]
    assert g.delete_documents(dead) == len(dead)
    docs = [d for d in DOCS[:16700] if d[0] not in set(dead)]
    commit_check(g, docs, 0, False, slices=32, stats=False)          # a full build through live_map: three blocks
    g.compact()
    commit_check(g, docs, 0, False, slices=32, stats=False, rows=False)
    commit_check(g, docs, 0, False, slices=32, stats=False, rows=False)         # the other snapshot
    docs = docs + DOCS[16700:16800]
    add(g, docs[-100:])
    commit_check(g, docs, 2, True, slices=32, stats=False)           # incremental again: the tail block alone
    commit_check(g, docs, 2, True, slices=32, stats=False, rows=False)
    g.close()


def test_knobs_that_keep_the_separate_kernels(monkeypatch):
    docs = DOCS[:16900]
    g = twice(docs)
    commit_check(g, docs, 2, True, rows=False)
    for name, value in zip(OFF_KNOBS, ("4", "1", "1")):
        monkeypatch.setenv(name, value)
        commit_check(g, docs, 2, False, rows=False)
        monkeypatch.delenv(name)
        commit_check(g, docs, 2, True, rows=False)                   # the next fused commit finds a clean scratch
    g.close()


def test_ranges_wider_than_one_scan_tile(monkeypatch):
    """33 203 terms at log2 17 (R = 2): each range holds more than 16 384 columns, so a range's last slice takes
    its columns in two tiles, neither range on a 16-column boundary (the documents, the oracles and the checks of
    test_gpu_inversion_slices: df of every word, the hits of a seeded 300)."""
    from test_gpu_inversion_slices import _check_wide, _fresh, _wide
    docs, _, o2 = _wide()
    g = _fresh(docs[:8300], dict(vocab_capacity_log2=17))
    g.commit()                                                       # the other snapshot's first build
    add(g, docs[8300:])
    force(monkeypatch, 3)
    for _ in range(3):                                               # both snapshots, and one again
        g.commit()
        assert g.commit_inverted_blocks() == {"first_block": 1, "n_blocks": 2, "remapped": 0}
        assert g.commit_inversion_fused() is True
        _check_wide(g, o2, len(docs))
    g.close()
